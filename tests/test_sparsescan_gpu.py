"""Sparse and 32x32 matrix-core scan on the GPU (native/hip/gm_sparsescan.hip): one block's raw
signature against the host table for every format, single instructions on constructed operands
against the numpy model of tests/sparse_operands.py (the test of the model's premises: which B
element a kept element meets for every index pair and set selector, the lane maps, the C/D maps),
clean scans and their bookkeeping, attribution of an injected flip, and the command lines. Nothing
here is sized by the workload: a scan is one 256-thread block per CU per round, a signature or an
``apply`` one block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sparse_operands as so  # noqa: E402
from gpumounter_amd.ops import cuscan, sparsescan  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
THREAD, WORD, MASK = 130, 2, 0x00010000


@pytest.fixture(scope="module")
def clean():
    """One clean scan at the default iters, shared by the tests that only read it."""
    return sparsescan.scan(0)


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


@pytest.mark.parametrize("iters", (1, 3, sparsescan.MAX_ITERS))
@pytest.mark.parametrize("fmt", sparsescan.ALL_FORMATS)
def test_signature_equals_expected(fmt, iters):
    sig, where = sparsescan.signature(fmt, SEED, iters)
    assert sig.shape == (256, 4) and sig.dtype == np.uint32
    want = sparsescan.expected(fmt, SEED, iters)
    print(fmt, iters, "words that differ:", int((sig != want).sum()))
    np.testing.assert_array_equal(sig, want)
    assert len(where["simds"]) == 4 and all(0 <= s < 4 for s in where["simds"]), where
    assert where["id"] < 4096 and where["xcc"] < 8, where


def test_signature_on_a_side_stream():
    s = torch.cuda.Stream()
    sig, _ = sparsescan.signature("bf16-32x32", 5, 2, stream=s)
    np.testing.assert_array_equal(sig, sparsescan.expected("bf16-32x32", 5, 2))


@pytest.mark.parametrize("fmt", sparsescan.ALL_FORMATS)
def test_apply_selects_the_b_element_the_index_names(fmt):
    """One launch per index pair and set selector (12 for a 16-bit form, 6 for an 8-bit one). Each
    row of A holds a single 1 in a kept slot that differs from row to row and B holds (k mod m) +
    1 at dense position k (m: sparse_operands.b_modulus, the format's run of exact integers), so
    row i of the output is the k its kept element was paired with, in every column."""
    size = so.FORMS[fmt][0]
    regs = 16 if size == 32 else 4
    for pair in range(6):
        for abid in range(so.sets(fmt)):
            a, b, idx, selected = so.one_hot_case(fmt, pair, abid)
            got = sparsescan.apply(fmt, abid, a, b, idx)
            c, unit = so.product(fmt, a, b, idx, abid)
            want = so.accumulators(fmt, c, unit)
            # the model's own answer is the closed form: row i reads (k_i mod m) + 1
            assert (c == ((selected % so.b_modulus(fmt)) + 1)[None, :, None] * unit).all()
            if (got != want).any():
                word = got[:64, :regs]
                vals = word.view(np.int32) if "i8" in fmt else word.view(np.float32)
                print(fmt, "pair", so.PAIRS[pair], "abid", abid, "wave 0 lane 0 registers:",
                      vals[0].tolist(), "lane 32:", vals[32].tolist(),
                      "model rows select k:", selected.tolist())
            np.testing.assert_array_equal(got, want, err_msg=f"{fmt} pair {so.PAIRS[pair]} "
                                                             f"abid {abid}")
            assert (got[:, regs:] == 0).all()


@pytest.mark.parametrize("fmt", sparsescan.ALL_FORMATS)
def test_apply_on_dense_random_operands(fmt):
    a, b, idx = so.random_case(fmt, seed=len(fmt) + sparsescan.FORMATS[fmt])
    abid = so.sets(fmt) - 1           # the second set where there is one
    got = sparsescan.apply(fmt, abid, a, b, idx)
    c, unit = so.product(fmt, a, b, idx, abid)
    want = so.accumulators(fmt, c, unit)
    print(fmt, "words that differ:", int((got != want).sum()), "of", want.size)
    np.testing.assert_array_equal(got, want)


def test_apply_refuses_before_the_gpu():
    a, b, idx = so.random_case("i8", 1)
    with pytest.raises(sparsescan.ProbeError, match="one index set"):
        sparsescan.apply("i8", 1, a, b, idx)
    with pytest.raises(sparsescan.ProbeError, match=r"A must be uint32\[4, 64, 4\]"):
        sparsescan.apply("i8", 0, a[:, :, :2], b, idx)
    with pytest.raises(sparsescan.ProbeError, match="must be uint32"):
        sparsescan.apply("i8", 0, a, b.astype(np.int64), idx)


def test_clean_scan_at_iters_1():
    _check_clean(sparsescan.scan(0, iters=1))


def test_clean_scan_at_the_default_iters(clean):
    assert clean["iters"] == sparsescan.DEFAULT_ITERS
    assert clean["formats"] == list(sparsescan.ALL_FORMATS)
    _check_clean(clean)


@pytest.mark.parametrize("fmt", sparsescan.ALL_FORMATS)
def test_injected_flip_is_attributed_to_its_cu(clean, fmt):
    target = clean["per_cu"][len(clean["per_cu"]) // 2]["id"]
    r = sparsescan.scan(0, _inject=(target, fmt, THREAD, WORD, MASK))
    assert not r["ok"] and r["failed_cus"] == 1
    (f,) = r["failed"]
    assert f["id"] == target and f["formats_failed"] == [fmt]
    assert f["failed_runs"] == f["runs"] >= 1
    assert r["words_in_error"] == f["runs"]
    rec = r["first_errors"][0]
    assert int(rec["expected"], 16) ^ int(rec["got"], 16) == MASK == int(rec["xor"], 16)
    assert (rec["id"], rec["format"], rec["thread"], rec["word"]) == (target, fmt, THREAD, WORD)
    assert rec["expected"] == f"{sparsescan.expected(fmt)[THREAD, WORD]:#010x}"
    assert rec["simd"] in f["simds_failed"]
    assert len(r["first_errors"]) == min(16, f["runs"])
    for c in r["per_cu"]:
        assert c["failed_runs"] == (c["runs"] if c["id"] == target else 0), c
    assert sum(c["runs"] for c in r["per_cu"]) == r["rounds"] * r["cus_expected"]


def test_injection_anywhere_fails_every_cu():
    r = sparsescan.scan(0, formats=("i8", "fp8-32x32"), iters=1,
                        _inject=("any", "fp8-32x32", 0, 3, 1))
    assert r["formats"] == ["i8", "fp8-32x32"]
    assert not r["ok"] and r["failed_cus"] == r["cus_seen"] == len(r["failed"])
    assert r["words_in_error"] == r["blocks_run"]
    assert all(f["formats_failed"] == ["fp8-32x32"] for f in r["failed"])
    assert len(r["first_errors"]) == 16
    assert all(int(x["xor"], 16) == 1 and (x["thread"], x["word"]) == (0, 3)
               for x in r["first_errors"])


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=180)


def test_probe_cli_sparse_scan():
    res = _cli("probe", "--sparse-scan")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["sparsescan"]["ok"] is True and r["sparsescan"]["complete"] and
                       r["sparsescan"]["formats"] == list(sparsescan.ALL_FORMATS)
                       for r in out), out


def test_probe_cli_sparse_scan_inject_fails():
    res = _cli("probe", "--sparse-scan", "--sparse-scan-inject", "any:i8-32x32:0:0:1")
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    out = json.loads(res.stdout)
    for r in out:
        c = r["sparsescan"]
        assert c["ok"] is False and c["failed_cus"] == c["cus_seen"] == len(c["failed"])
        assert all(f["formats_failed"] == ["i8-32x32"] for f in c["failed"])


def test_doctor_reports_the_failed_unit_and_format(clean):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    # the real amdsmi, as tests/test_gpu.py uses it: the mock's symbols, once loaded into this
    # process, would serve every later inventory of the session
    cfg = Config.load(env={})
    target = clean["per_cu"][len(clean["per_cu"]) // 2]
    (ok,) = [c for c in doctor.check_gpus(cfg, sparse_scan=True) if c.name == "gpu0"]
    assert ok.status in ("ok", "warn") and "sparse-scan 11 formats" in ok.detail, ok
    assert " 0 wrong words" in ok.detail, ok
    (bad,) = [c for c in doctor.check_gpus(
        cfg, sparse_scan=True, sparse_scan_inject=(target["id"], "bf8fp8", THREAD, WORD, MASK))
        if c.name == "gpu0"]
    assert bad.status == "fail", bad
    assert (f"xcc {target['xcc']} se {target['se']} sh {target['sh']} cu {target['cu']} "
            f"(id {target['id']:#05x})") in bad.detail and bad.detail.endswith("bf8fp8"), bad
