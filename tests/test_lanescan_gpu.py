"""Lane scan on the GPU (native/hip/gm_lanescan.hip): one block's raw signature against the host
table for every test (the test that catches a wrong lane model, a miscompiled register index or
an inexact transcendental), clean scans and their bookkeeping, attribution of an injected flip to
the CU, test, thread and word it was made in, the kernel's scratch use, and the command lines.
Nothing here is sized by the workload: a scan is one 256-thread block per CU per round, a
signature one block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpumounter_amd.ops import cuscan, lanescan  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
THREAD, WORD, MASK = 130, 2, 0x00010000


@pytest.fixture(scope="module")
def clean():
    """One clean scan at the default iters, shared by the tests that only read it."""
    return lanescan.scan(0)


def _check_clean(r):
    print({k: r[k] for k in ("cus_expected", "cus_seen", "rounds", "blocks_run", "xcc_cus",
                             "blocks_four_simds", "kernel_ms", "seconds")})
    assert r["ok"] and r["words_in_error"] == 0 and r["failed"] == [] and r["failed_cus"] == 0, r
    assert r["first_errors"] == []
    assert sum(c["runs"] for c in r["per_cu"]) == r["rounds"] * r["cus_expected"] == r["blocks_run"]
    assert sum(r["xcc_cus"]) == r["cus_seen"] == len(r["per_cu"])
    assert r["cus_seen"] == r["cus_expected"] and r["complete"], r["xcc_cus"]
    assert r["rounds"] <= 16
    ids = [c["id"] for c in r["per_cu"]]
    assert ids == sorted(set(ids))
    for c in r["per_cu"]:
        assert cuscan.decode_id(c["id"]) == {k: c[k] for k in ("xcc", "se", "sh", "cu")}
        assert c["xcc"] < 8 and c["simds_seen"] and c["failed_runs"] == 0


@pytest.mark.parametrize("iters", (1, 3, lanescan.MAX_ITERS))
@pytest.mark.parametrize("test", lanescan.ALL_TESTS)
def test_signature_equals_expected(test, iters):
    sig, where = lanescan.signature(test, SEED, iters)
    assert sig.shape == (256, 4) and sig.dtype == np.uint32
    want = lanescan.expected(test, SEED, iters)
    diff = sig != want
    print(test, iters, "words that differ:", int(diff.sum()), "per word:", diff.sum(axis=0).tolist(),
          "first threads:", np.flatnonzero(diff.any(axis=1))[:8].tolist())
    np.testing.assert_array_equal(sig, want)
    assert len(where["simds"]) == 4 and all(0 <= s < 4 for s in where["simds"]), where
    assert where["id"] < 4096 and where["xcc"] < 8, where


def test_signature_on_a_side_stream():
    s = torch.cuda.Stream()
    sig, _ = lanescan.signature("salu", 5, 2, stream=s)
    np.testing.assert_array_equal(sig, lanescan.expected("salu", 5, 2))


def test_clean_scan_at_iters_1():
    _check_clean(lanescan.scan(0, iters=1))


def test_clean_scan_at_the_default_iters(clean):
    assert clean["iters"] == lanescan.DEFAULT_ITERS
    assert clean["tests"] == list(lanescan.ALL_TESTS)
    _check_clean(clean)


@pytest.mark.parametrize("test", lanescan.ALL_TESTS)
def test_injected_flip_is_attributed_to_its_cu(clean, test):
    target = clean["per_cu"][len(clean["per_cu"]) // 2]["id"]
    r = lanescan.scan(0, _inject=(target, test, THREAD, WORD, MASK))
    assert not r["ok"] and r["failed_cus"] == 1
    (f,) = r["failed"]
    assert f["id"] == target and f["tests_failed"] == [test]
    assert f["failed_runs"] == f["runs"] >= 1
    assert r["words_in_error"] == f["runs"]
    rec = r["first_errors"][0]
    assert int(rec["expected"], 16) ^ int(rec["got"], 16) == MASK == int(rec["xor"], 16)
    assert (rec["id"], rec["test"], rec["thread"], rec["word"]) == (target, test, THREAD, WORD)
    assert rec["expected"] == f"{lanescan.expected(test)[THREAD, WORD]:#010x}"
    assert rec["simd"] in f["simds_failed"]
    assert len(r["first_errors"]) == min(16, f["runs"])
    for c in r["per_cu"]:
        assert c["failed_runs"] == (c["runs"] if c["id"] == target else 0), c
    assert sum(c["runs"] for c in r["per_cu"]) == r["rounds"] * r["cus_expected"]


def test_injection_anywhere_fails_every_cu():
    r = lanescan.scan(0, tests=("xlane", "packed"), iters=1, _inject=("any", "packed", 0, 3, 1))
    assert r["tests"] == ["xlane", "packed"]
    assert not r["ok"] and r["failed_cus"] == r["cus_seen"] == len(r["failed"])
    assert r["words_in_error"] == r["blocks_run"]
    assert all(f["tests_failed"] == ["packed"] for f in r["failed"])
    assert len(r["first_errors"]) == 16
    assert all(int(x["xor"], 16) == 1 and (x["thread"], x["word"]) == (0, 3)
               for x in r["first_errors"])


def test_kernel_uses_no_scratch():
    info = lanescan.kernel_info()
    print("lane-scan kernel:", info)      # num_regs is recorded, not asserted
    assert info["scratch_bytes"] == 0, info


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=180)


def test_probe_cli_lane_scan():
    res = _cli("probe", "--lane-scan")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["lanescan"]["ok"] is True and r["lanescan"]["complete"] and
                       r["lanescan"]["tests"] == list(lanescan.ALL_TESTS) for r in out), out


def test_probe_cli_lane_scan_inject_fails():
    res = _cli("probe", "--lane-scan", "--lane-scan-inject", "any:xlane:0:0:1")
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    out = json.loads(res.stdout)
    for r in out:
        c = r["lanescan"]
        assert c["ok"] is False and c["failed_cus"] == c["cus_seen"] == len(c["failed"])
        assert all(f["tests_failed"] == ["xlane"] for f in c["failed"])


def test_doctor_reports_the_failed_unit_and_test(clean):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    # the real amdsmi, as tests/test_gpu.py uses it: the mock's symbols, once loaded into this
    # process, would serve every later inventory of the session
    cfg = Config.load(env={})
    target = clean["per_cu"][len(clean["per_cu"]) // 2]
    (ok,) = [c for c in doctor.check_gpus(cfg, lane_scan=True) if c.name == "gpu0"]
    assert ok.status in ("ok", "warn") and "lane-scan 6 tests" in ok.detail, ok
    assert " 0 wrong words" in ok.detail, ok
    (bad,) = [c for c in doctor.check_gpus(
        cfg, lane_scan=True, lane_scan_inject=(target["id"], "regfile", THREAD, WORD, MASK))
        if c.name == "gpu0"]
    assert bad.status == "fail", bad
    assert (f"xcc {target['xcc']} se {target['se']} sh {target['sh']} cu {target['cu']} "
            f"(id {target['id']:#05x})") in bad.detail and bad.detail.endswith("regfile"), bad
