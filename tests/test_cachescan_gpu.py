"""Cache scan on the GPU (native/hip/gm_cachescan.hip): one block's raw signature against the host
table for every test, with and without a poked word (the test that catches a wrong permutation
stride, a dropped inversion, a changed literal of the icache body or a table index off by one),
clean scans and their bookkeeping, attribution of an injected flip, a data poke found by the real
detection path, the kernel's scratch use and the icache body's span, the timing report, and the
command lines. Nothing here is sized by the workload: a scan is one 256-thread block per CU per
round, a signature one block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpumounter_amd.ops import cachescan, cuscan  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
THREAD, WORD, MASK = 130, 2, 0x00010000


@pytest.fixture(scope="module")
def clean():
    """One clean scan at the default iters, shared by the tests that only read it."""
    return cachescan.scan(0)


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


def _check_timing(r):
    """Present, nonzero, printed; nothing about its size is asserted."""
    timing = r["timing"]
    print("timing:", json.dumps(timing))
    assert timing["blocks"] == r["cus_expected"]
    for test in r["tests"]:
        for which in ("first", "last"):
            counts = timing[test][which]
            assert set(counts) == {"min", "median", "max"}
            assert all(isinstance(v, int) and v > 0 for v in counts.values()), (test, which, counts)


@pytest.mark.parametrize("iters", (1, 2, cachescan.MAX_ITERS))
@pytest.mark.parametrize("test", cachescan.ALL_TESTS)
def test_signature_equals_expected(test, iters):
    sig, where = cachescan.signature(test, SEED, iters)
    assert sig.shape == (256, 4) and sig.dtype == np.uint32
    want = cachescan.expected(test, SEED, iters)
    diff = sig != want
    print(test, iters, "words that differ:", int(diff.sum()), "per word:", diff.sum(axis=0).tolist(),
          "first threads:", np.flatnonzero(diff.any(axis=1))[:8].tolist())
    np.testing.assert_array_equal(sig, want)
    assert len(where["simds"]) == 4 and all(0 <= s < 4 for s in where["simds"]), where
    assert where["id"] < 4096 and where["xcc"] < 8, where


def test_signature_on_a_side_stream():
    s = torch.cuda.Stream()
    sig, _ = cachescan.signature("l1", 5, 2, stream=s)
    np.testing.assert_array_equal(sig, cachescan.expected("l1", 5, 2))


@pytest.mark.parametrize("poke", (("l2", 4099, 0x10), ("l1", 4099, 0x10), ("l1", 100, 1 << 31),
                                  ("scalar", None, 1)))
def test_poked_signature_equals_the_poked_table(poke):
    """The host model of a poked run is exact: the GPU's poked signature equals it bit for bit,
    and differs from the clean table."""
    test, offset, mask = poke
    iters = 2
    clean_table = cachescan.expected(test, SEED, iters)
    if offset is None:
        # a table word that a chain reads: wave 0's first index, i = H(0x411, 0) % 8192, found
        # here as the first word whose flip changes the host table
        offset = next(o for o in range(cachescan.TABLE_WORDS)
                      if (cachescan.expected(test, SEED, iters, poke=(test, o, mask))
                          != clean_table).any())
    poke = (test, offset, mask)
    sig, _ = cachescan.signature(test, SEED, iters, poke=poke)
    want = cachescan.expected(test, SEED, iters, poke=poke)
    print(poke, "differ from the poked table:", int((sig != want).sum()), "from the clean one:",
          int((sig != clean_table).sum()))
    np.testing.assert_array_equal(sig, want)
    assert (sig != clean_table).any()


def test_clean_scan_at_iters_1():
    r = cachescan.scan(0, iters=1)
    _check_clean(r)
    _check_timing(r)


def test_clean_scan_at_the_default_iters(clean):
    assert clean["iters"] == cachescan.DEFAULT_ITERS
    assert clean["tests"] == list(cachescan.ALL_TESTS)
    _check_clean(clean)
    _check_timing(clean)


@pytest.mark.parametrize("test", cachescan.ALL_TESTS)
def test_injected_flip_is_attributed_to_its_cu(clean, test):
    target = clean["per_cu"][len(clean["per_cu"]) // 2]["id"]
    r = cachescan.scan(0, _inject=(target, test, THREAD, WORD, MASK))
    assert not r["ok"] and r["failed_cus"] == 1
    (f,) = r["failed"]
    assert f["id"] == target and f["tests_failed"] == [test]
    assert f["failed_runs"] == f["runs"] >= 1
    assert r["words_in_error"] == f["runs"]
    rec = r["first_errors"][0]
    assert int(rec["expected"], 16) ^ int(rec["got"], 16) == MASK == int(rec["xor"], 16)
    assert (rec["id"], rec["test"], rec["thread"], rec["word"]) == (target, test, THREAD, WORD)
    assert rec["expected"] == f"{cachescan.expected(test)[THREAD, WORD]:#010x}"
    assert rec["simd"] in f["simds_failed"]
    assert len(r["first_errors"]) == min(16, f["runs"])
    for c in r["per_cu"]:
        assert c["failed_runs"] == (c["runs"] if c["id"] == target else 0), c
    assert sum(c["runs"] for c in r["per_cu"]) == r["rounds"] * r["cus_expected"]


def test_injection_anywhere_fails_every_cu():
    r = cachescan.scan(0, tests=("l2", "icache"), iters=1, _inject=("any", "icache", 0, 3, 1))
    assert r["tests"] == ["l2", "icache"]
    assert not r["ok"] and r["failed_cus"] == r["cus_seen"] == len(r["failed"])
    assert r["words_in_error"] == r["blocks_run"]
    assert all(f["tests_failed"] == ["icache"] for f in r["failed"])
    assert len(r["first_errors"]) == 16
    assert all(int(x["xor"], 16) == 1 and (x["thread"], x["word"]) == (0, 3)
               for x in r["first_errors"])


def test_a_poke_of_l1_fails_every_cu_with_l1_and_no_other_test():
    poke = ("l1", 4099, 0x10)
    r = cachescan.scan(0, _poke=poke)
    assert not r["ok"] and r["failed_cus"] == r["cus_seen"] == len(r["failed"])
    assert all(f["tests_failed"] == ["l1"] for f in r["failed"])
    # the words the host model says: s0, s1 and s3 of the thread that reads the word
    diff = cachescan.expected("l1", poke=poke) != cachescan.expected("l1")
    assert r["words_in_error"] == int(diff.sum()) * r["blocks_run"]
    threads, words = np.nonzero(diff)
    assert {(x["test"], x["thread"], x["word"]) for x in r["first_errors"]} <= {
        ("l1", int(t), int(w)) for t, w in zip(threads, words)}


def test_kernel_uses_no_scratch_and_the_icache_body_is_large_enough():
    info = cachescan.kernel_info()
    print("cache-scan kernel:", info)      # num_regs is recorded, not asserted
    assert info["scratch_bytes"] == 0, info
    assert info["icache_body_bytes"] >= 131072, info     # read from the program counter


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=180)


def test_probe_cli_cache_scan():
    res = _cli("probe", "--cache-scan")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["cachescan"]["ok"] is True and r["cachescan"]["complete"] and
                       r["cachescan"]["tests"] == list(cachescan.ALL_TESTS) and
                       r["cachescan"]["timing"]["blocks"] > 0 for r in out), out


def test_probe_cli_cache_scan_inject_fails():
    res = _cli("probe", "--cache-scan", "--cache-scan-inject", "any:l2:0:0:1")
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    out = json.loads(res.stdout)
    for r in out:
        c = r["cachescan"]
        assert c["ok"] is False and c["failed_cus"] == c["cus_seen"] == len(c["failed"])
        assert all(f["tests_failed"] == ["l2"] for f in c["failed"])


def test_probe_cli_cache_scan_poke_fails():
    res = _cli("probe", "--cache-scan", "--cache-scan-poke", "l1:4099:0x10")
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    out = json.loads(res.stdout)
    for r in out:
        c = r["cachescan"]
        assert c["ok"] is False and c["failed_cus"] == c["cus_seen"] == len(c["failed"])
        assert all(f["tests_failed"] == ["l1"] for f in c["failed"])


def test_doctor_reports_the_failed_unit_and_test(clean):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    # the real amdsmi, as tests/test_gpu.py uses it: the mock's symbols, once loaded into this
    # process, would serve every later inventory of the session
    cfg = Config.load(env={})
    target = clean["per_cu"][len(clean["per_cu"]) // 2]
    (ok,) = [c for c in doctor.check_gpus(cfg, cache_scan=True) if c.name == "gpu0"]
    assert ok.status in ("ok", "warn") and "cache-scan 4 tests" in ok.detail, ok
    assert " 0 wrong words" in ok.detail, ok
    (bad,) = [c for c in doctor.check_gpus(
        cfg, cache_scan=True, cache_scan_inject=(target["id"], "scalar", THREAD, WORD, MASK))
        if c.name == "gpu0"]
    assert bad.status == "fail", bad
    assert (f"xcc {target['xcc']} se {target['se']} sh {target['sh']} cu {target['cu']} "
            f"(id {target['id']:#05x})") in bad.detail and bad.detail.endswith("scalar"), bad
