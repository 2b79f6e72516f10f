"""LDS scan on the GPU (native/hip/gm_ldsscan.hip): one block's raw signature against the host
table for every test, with and without a poked word (the test that catches a wrong schedule, a
wrong extension of a sub-dword load, a lost atomic, a wrong lane of the transposing read or a
global-to-LDS load that lands elsewhere), clean scans and their bookkeeping, attribution of an
injected flip, a data poke found by the real detection path, the kernel's scratch use, and the
command lines. Nothing here is sized by a workload: a scan is one 256-thread block per CU per
round, a signature one block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpumounter_amd.ops import cuscan, ldsscan  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
THREAD, WORD, MASK = 130, 2, 0x00010000
POKED = ("width", "bank", "tr16", "dma")


@pytest.fixture(scope="module")
def clean():
    """One clean scan at the default iters, shared by the tests that only read it."""
    return ldsscan.scan(0)


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


@pytest.mark.parametrize("iters", (1, 2, ldsscan.MAX_ITERS))
@pytest.mark.parametrize("test", ldsscan.ALL_TESTS)
def test_signature_equals_expected(test, iters):
    sig, where = ldsscan.signature(test, SEED, iters)
    assert sig.shape == (256, 4) and sig.dtype == np.uint32
    want = ldsscan.expected(test, SEED, iters)
    diff = sig != want
    print(test, iters, "words that differ:", int(diff.sum()), "per word:", diff.sum(axis=0).tolist(),
          "first threads:", np.flatnonzero(diff.any(axis=1))[:8].tolist())
    np.testing.assert_array_equal(sig, want)
    assert len(where["simds"]) == 4 and all(0 <= s < 4 for s in where["simds"]), where
    assert where["id"] < 4096 and where["xcc"] < 8, where


def test_signature_on_a_side_stream():
    s = torch.cuda.Stream()
    sig, _ = ldsscan.signature("dma", 5, 2, stream=s)
    np.testing.assert_array_equal(sig, ldsscan.expected("dma", 5, 2))


@pytest.mark.parametrize("where", ((100, 0x10), (40959, 1 << 31)))
@pytest.mark.parametrize("test", POKED)
def test_poked_signature_equals_the_poked_table(test, where):
    """The host model of a poked run is exact: the GPU's poked signature equals it bit for bit,
    and differs from the clean table."""
    poke, iters = (test, *where), 2
    clean_table = ldsscan.expected(test, SEED, iters)
    sig, _ = ldsscan.signature(test, SEED, iters, poke=poke)
    want = ldsscan.expected(test, SEED, iters, poke=poke)
    print(poke, "differ from the poked table:", int((sig != want).sum()), "from the clean one:",
          int((sig != clean_table).sum()))
    np.testing.assert_array_equal(sig, want)
    assert (sig != clean_table).any()


def test_clean_scan_at_iters_1():
    _check_clean(ldsscan.scan(0, iters=1))


def test_clean_scan_at_the_default_iters(clean):
    assert clean["iters"] == ldsscan.DEFAULT_ITERS
    assert clean["tests"] == list(ldsscan.ALL_TESTS)
    _check_clean(clean)


@pytest.mark.parametrize("test", ldsscan.ALL_TESTS)
def test_injected_flip_is_attributed_to_its_cu(clean, test):
    target = clean["per_cu"][len(clean["per_cu"]) // 2]["id"]
    r = ldsscan.scan(0, _inject=(target, test, THREAD, WORD, MASK))
    assert not r["ok"] and r["failed_cus"] == 1
    (f,) = r["failed"]
    assert f["id"] == target and f["tests_failed"] == [test]
    assert f["failed_runs"] == f["runs"] >= 1
    assert r["words_in_error"] == f["runs"]
    rec = r["first_errors"][0]
    assert int(rec["expected"], 16) ^ int(rec["got"], 16) == MASK == int(rec["xor"], 16)
    assert (rec["id"], rec["test"], rec["thread"], rec["word"]) == (target, test, THREAD, WORD)
    assert rec["expected"] == f"{ldsscan.expected(test)[THREAD, WORD]:#010x}"
    assert rec["simd"] in f["simds_failed"]
    assert len(r["first_errors"]) == min(16, f["runs"])
    for c in r["per_cu"]:
        assert c["failed_runs"] == (c["runs"] if c["id"] == target else 0), c
    assert sum(c["runs"] for c in r["per_cu"]) == r["rounds"] * r["cus_expected"]


def test_injection_anywhere_fails_every_cu():
    r = ldsscan.scan(0, tests=("atomic", "dma"), iters=1, _inject=("any", "dma", 0, 3, 1))
    assert r["tests"] == ["atomic", "dma"]
    assert not r["ok"] and r["failed_cus"] == r["cus_seen"] == len(r["failed"])
    assert r["words_in_error"] == r["blocks_run"]
    assert all(f["tests_failed"] == ["dma"] for f in r["failed"])
    assert len(r["first_errors"]) == 16
    assert all(int(x["xor"], 16) == 1 and (x["thread"], x["word"]) == (0, 3)
               for x in r["first_errors"])


def test_a_poke_of_bank_fails_every_cu_with_bank_and_no_other_test():
    poke = ("bank", 4099, 0x10)
    r = ldsscan.scan(0, _poke=poke)
    assert not r["ok"] and r["failed_cus"] == r["cus_seen"] == len(r["failed"])
    assert all(f["tests_failed"] == ["bank"] for f in r["failed"])
    diff = ldsscan.expected("bank", poke=poke) != ldsscan.expected("bank")
    assert diff.any() and r["words_in_error"] == int(diff.sum()) * r["blocks_run"]
    threads, words = np.nonzero(diff)
    assert {(x["test"], x["thread"], x["word"]) for x in r["first_errors"]} <= {
        ("bank", int(t), int(w)) for t, w in zip(threads, words)}


def test_kernel_uses_no_scratch():
    info = ldsscan.kernel_info()
    print("lds-scan kernel:", info)      # num_regs is recorded, not asserted
    assert info["scratch_bytes"] == 0, info


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=180)


def test_probe_cli_lds_scan():
    res = _cli("probe", "--lds-scan")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["ldsscan"]["ok"] is True and r["ldsscan"]["complete"] and
                       r["ldsscan"]["tests"] == list(ldsscan.ALL_TESTS) for r in out), out


def test_probe_cli_lds_scan_inject_fails():
    res = _cli("probe", "--lds-scan", "--lds-scan-inject", "any:atomic:0:0:1")
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    for r in json.loads(res.stdout):
        c = r["ldsscan"]
        assert c["ok"] is False and c["failed_cus"] == c["cus_seen"] == len(c["failed"])
        assert all(f["tests_failed"] == ["atomic"] for f in c["failed"])


def test_probe_cli_lds_scan_poke_fails():
    res = _cli("probe", "--lds-scan", "--lds-scan-poke", "tr16:4099:0x10")
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    for r in json.loads(res.stdout):
        c = r["ldsscan"]
        assert c["ok"] is False and c["failed_cus"] == c["cus_seen"] == len(c["failed"])
        assert all(f["tests_failed"] == ["tr16"] for f in c["failed"])


def test_doctor_reports_the_failed_unit_and_test(clean):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    # the real amdsmi, as tests/test_gpu.py uses it: the mock's symbols, once loaded into this
    # process, would serve every later inventory of the session
    cfg = Config.load(env={})
    target = clean["per_cu"][len(clean["per_cu"]) // 2]
    (ok,) = [c for c in doctor.check_gpus(cfg, lds_scan=True) if c.name == "gpu0"]
    assert ok.status in ("ok", "warn") and "lds-scan 5 tests" in ok.detail, ok
    assert " 0 wrong words" in ok.detail, ok
    (bad,) = [c for c in doctor.check_gpus(
        cfg, lds_scan=True, lds_scan_inject=(target["id"], "tr16", THREAD, WORD, MASK))
        if c.name == "gpu0"]
    assert bad.status == "fail", bad
    assert (f"xcc {target['xcc']} se {target['se']} sh {target['sh']} cu {target['cu']} "
            f"(id {target['id']:#05x})") in bad.detail and bad.detail.endswith("tr16"), bad
