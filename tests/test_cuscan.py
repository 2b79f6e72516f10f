"""CU scan, host side (gpumounter_amd/ops/cuscan.py): the four signature functions against an
independent numpy reference written here from the formulas in native/include/gm_probe.h, the
parsers, and the argument validation that happens before any HIP call. No GPU needed; the kernel
is covered by tests/test_cuscan_gpu.py."""
import ctypes as C
import inspect

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import cuscan
from gpumounter_amd.ops.probe import ProbeError

SEEDS = (0, 0x0123456789ABCDEF)
ITERS = (1, 3, cuscan.DEFAULT_ITERS)
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------- the reference (uint64 & 2^32 - 1)
def u(v):
    return np.asarray(v, dtype=np.uint64) & M32


def rotl(v, s):
    return ((v << np.uint64(s)) | (v >> np.uint64(32 - s))) & M32


def H(seed, test, idx):
    h = u(seed & 0xFFFFFFFF) ^ u(u(idx) * np.uint64(0x9E3779B1))
    h ^= h >> np.uint64(16)
    h = u(h * np.uint64(0x85EBCA6B))
    h ^= h >> np.uint64(13)
    h = u(h + np.uint64((seed >> 32) ^ (test * 0xC2B2AE35 & 0xFFFFFFFF)))
    h ^= h >> np.uint64(16)
    h = u(h * np.uint64(0xC2B2AE35))
    h ^= h >> np.uint64(13)
    h = u(h * np.uint64(0x27D4EB2F))
    h ^= h >> np.uint64(16)
    return h


def ref_int(seed, iters):
    t = np.arange(256, dtype=np.uint64)
    ks = [np.uint64(k) for k in (0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F)]
    out = np.empty((256, 4), dtype=np.uint32)
    for chain in range(2):
        x, y = H(seed, 1, 4 * t + 2 * chain), H(seed, 1, 4 * t + 2 * chain + 1)
        for s in range(128 * iters):
            x = u(rotl(x, 24) + y) ^ ks[s & 3]
            y = rotl(y, 3) ^ x
            m = x * (y | np.uint64(1))                   # < 2^64: exact in uint64
            x = x ^ (m >> np.uint64(32))
            y = u(y + (m & M32))
        out[:, 2 * chain], out[:, 2 * chain + 1] = x, y
    return out


def ref_f32(seed, iters):
    q = np.arange(1024, dtype=np.uint64)                  # 4 t + j
    h1, h2 = H(seed, 2, q), H(seed, 2, 1024 + q)
    x = (1.0 + (h1 >> np.uint64(9)).astype(np.float64) / 2**23).astype(np.float32)
    a = 1.0 + (h2 >> np.uint64(20)).astype(np.float64) / 2**12
    b = (h2 & np.uint64(0xFFFFFF)).astype(np.float64) / 2**24
    for _ in range(64 * iters):
        r = (x.astype(np.float64) * a + b).astype(np.float32)     # exact, rounded once
        x = (r.astype(np.float64) - np.floor(r.astype(np.float64)) + 1.0).astype(np.float32)
    return x.view(np.uint32).reshape(256, 4)


def ref_mfma(seed, iters):
    out = np.empty((256, 4), dtype=np.uint32)
    r, k, c = np.arange(16)[:, None], np.arange(32)[None, :], np.arange(16)[None, :]
    kk = np.arange(32)[:, None]
    for w in range(4):
        acc = np.zeros((16, 16), dtype=np.int64)
        for s in range(4 * iters):
            base = ((4 * s + w) * 2) * 64
            ha = H(seed, 4, base + r + 16 * (k >> 3))                       # [16, 32]
            hb = H(seed, 4, base + 64 + c + 16 * (kk >> 3))                 # [32, 16]
            A = ((ha >> (4 * (k & 7)).astype(np.uint64)) & np.uint64(15)) % np.uint64(9)
            B = ((hb >> (4 * (kk & 7)).astype(np.uint64)) & np.uint64(15)) % np.uint64(9)
            acc += (A.astype(np.int64) - 4) @ (B.astype(np.int64) - 4)
        assert np.abs(acc).max() < 2**24
        lane = np.arange(64)
        for i in range(4):
            out[64 * w:64 * w + 64, i] = acc[4 * (lane >> 4) + i, lane & 15].astype(
                np.float32).view(np.uint32)
    return out


def ref_lds(seed, iters):
    t = np.arange(256, dtype=np.uint64)
    s0 = np.zeros(256, dtype=np.uint64)
    s1, s2 = s0.copy(), s0.copy()
    for r in range(iters):
        for i in range(160):
            a = ((256 * i + t) * np.uint64(12347) + np.uint64(7)) % np.uint64(40960)
            s0 = u(rotl(s0, 5) + H(seed, 8, 65536 * r + a))
        for k in range(40):
            v = 256 * k + ((t + np.uint64(64)) % np.uint64(256))
            for c in range(4):
                g = H(seed, 8, 65536 * r + 4 * v + c) ^ M32
                s1 = rotl(s1, 7) ^ g
                s2 = u(s2 + g)
    return np.stack([s0, s1, s2, np.zeros(256, dtype=np.uint64)], axis=1).astype(np.uint32)


REFS = {"int": ref_int, "f32": ref_f32, "mfma": ref_mfma, "lds": ref_lds}


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("test", cuscan.ALL_TESTS)
def test_expected_equals_the_numpy_reference(test, seed, iters):
    got = cuscan.expected(test, seed, iters)
    assert got.shape == (256, 4) and got.dtype == np.uint32
    np.testing.assert_array_equal(got, REFS[test](seed, iters))


def test_expected_accepts_the_bit_as_well_as_the_name():
    for name, bit in cuscan.TESTS.items():
        np.testing.assert_array_equal(cuscan.expected(bit, 5, 1), cuscan.expected(name, 5, 1))


@pytest.mark.parametrize("seed", SEEDS)
def test_f32_chains_do_not_converge(seed):
    """A chain that converged would make the fp32 test useless: nearly all 1024 words differ, and
    every one is a normal number in [1, 2)."""
    e = cuscan.expected("f32", seed, cuscan.DEFAULT_ITERS)
    assert len(np.unique(e)) >= 1000
    f = e.view(np.float32)
    assert np.all((f >= 1.0) & (f < 2.0))


def test_signatures_depend_on_seed_iters_and_test():
    tables = {t: cuscan.expected(t, 7, 2) for t in cuscan.ALL_TESTS}
    for t, e in tables.items():
        assert not np.array_equal(e, cuscan.expected(t, 8, 2)), t
        assert not np.array_equal(e, cuscan.expected(t, 7, 3)), t
    assert np.all(tables["lds"][:, 3] == 0)              # the in-flight mismatch count


def test_mfma_step_bound():
    """32 products of magnitude <= 16 per step and 4 steps per unit of iters: the sums stay exact
    fp32 integers while 32 * 16 * 4 * iters < 2^24."""
    lim = cuscan.MFMA_MAX_ITERS
    assert 32 * 16 * 4 * lim < 2**24 <= 32 * 16 * 4 * (lim + 1)
    e = cuscan.expected("mfma", 3, lim)                  # accepted at the limit
    f = e.view(np.float32)
    assert np.all(f == np.round(f)) and np.abs(f).max() < 2**24
    with pytest.raises(ProbeError, match="exact only up to"):
        cuscan.expected("mfma", 3, lim + 1)
    with pytest.raises(ProbeError, match="exact only up to"):
        cuscan.scan(0, tests=("mfma",), iters=lim + 1)
    out = (C.c_uint32 * 1024)()
    lib = _native.probe()
    assert lib.gm_probe_cuscan_expected(4, 3, lim + 1, out) == 1
    assert lib.gm_probe_cuscan_expected(1, 3, lim + 1, out) == 0     # the bound is the MFMA's own


def test_decode_id_round_trips():
    for cu_id in range(4096):
        d = cuscan.decode_id(cu_id)
        assert cuscan.encode_id(**d) == cu_id
    assert cuscan.decode_id(0x7FF) == {"xcc": 7, "se": 7, "sh": 1, "cu": 15}
    assert cuscan.decode_id(0x123) == {"xcc": 1, "se": 1, "sh": 0, "cu": 3}
    for bad in (-1, 4096, 1.0, "3", True):
        with pytest.raises(ProbeError, match="CU id"):
            cuscan.decode_id(bad)
    with pytest.raises(ProbeError, match="no CU id"):
        cuscan.encode_id(16, 0, 0, 0)


def test_parsers():
    assert cuscan.parse_tests("int,f32,mfma,lds") == cuscan.ALL_TESTS
    assert cuscan.parse_tests(" lds , int ") == ("lds", "int")
    with pytest.raises(ProbeError, match="unknown cu-scan test 'fp64'"):
        cuscan.parse_tests("int,fp64")
    with pytest.raises(ProbeError, match="at least one test"):
        cuscan.parse_tests(" , ")
    assert cuscan.parse_inject("any:mfma:0:0:1") == ("any", "mfma", 0, 0, 1)
    assert cuscan.parse_inject("0x123:lds:130:2:0x00010000") == (0x123, "lds", 130, 2, 0x10000)
    assert cuscan.parse_inject(" ANY : int : 255 : 3 : 0xffffffff ") == (
        "any", "int", 255, 3, 0xFFFFFFFF)
    for bad, msg in (("any:mfma:0:0", "ID|any:TEST:THREAD:WORD:MASK"),
                     ("any:mfma:0:0:1:2", "ID|any:TEST:THREAD:WORD:MASK"),
                     ("any:mfma:x:0:1", "not an integer"), ("some:mfma:0:0:1", "not an integer"),
                     ("any:fp64:0:0:1", "unknown cu-scan test"),
                     ("4096:mfma:0:0:1", "CU id"), ("-1:mfma:0:0:1", "CU id"),
                     ("any:mfma:256:0:1", "injection thread"),
                     ("any:mfma:0:4:1", "injection word"), ("any:mfma:0:0:0", "injection mask"),
                     ("any:mfma:0:0:0x100000000", "injection mask")):
        with pytest.raises(ProbeError, match=msg.replace("|", r"\|")):
            cuscan.parse_inject(bad)


def test_scan_validates_before_any_hip_call(monkeypatch):
    """Every refusal below is made in Python with the native library unreachable: none of them
    can have touched HIP."""
    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    for kw in (dict(tests=()), dict(tests=("int", "fp64")), dict(tests=16), dict(iters=0),
               dict(iters=1.5), dict(iters=True), dict(iters=cuscan.MAX_ITERS + 1),
               dict(iters=cuscan.MFMA_MAX_ITERS + 1), dict(seed=-1), dict(seed=1 << 64),
               dict(min_rounds=0), dict(min_rounds=3, max_rounds=2),
               dict(max_rounds=cuscan.MAX_ROUNDS + 1),
               dict(_inject=("any", "mfma", 0, 0, 0)), dict(_inject=("any", "mfma", 256, 0, 1)),
               dict(_inject=("any", "mfma", 0, 4, 1)), dict(_inject=(4096, "mfma", 0, 0, 1)),
               dict(_inject=("any", "mfma", 0, 0)),
               dict(tests=("int",), _inject=("any", "mfma", 0, 0, 1))):
        with pytest.raises(ProbeError):
            cuscan.scan(0, **kw)
    with pytest.raises(ProbeError):
        cuscan.scan(-1)
    for call in (lambda: cuscan.expected("fp64", 0, 1), lambda: cuscan.expected("int", 0, 0),
                 lambda: cuscan.signature("int", 0, 0), lambda: cuscan.signature(3, 0, 1)):
        with pytest.raises(ProbeError):
            call()
    with pytest.raises(AssertionError):                  # a good call does get there
        cuscan.scan(0)


def test_native_entry_points_validate_before_selecting_a_device():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    res, n = _native.CuscanResult(), C.c_int(7)
    cus = (_native.CuscanCu * 4)()
    out = (C.c_uint32 * 1024)()
    P, W = C.c_void_p(4096), C.c_void_p(8192)   # never dereferenced: every call is refused first
    for test, iters in ((0, 1), (3, 1), (16, 1), (1, 0), (1, 65536), (4, 8192)):
        assert lib.gm_probe_cuscan_expected(test, 0, iters, out) == 1
        assert lib.gm_probe_cuscan_signature(test, 0, iters, P, W, None) == 1
    assert lib.gm_probe_cuscan_expected(1, 0, 1, None) == 1
    for o, w in ((None, W), (P, None), (C.c_void_p(4096 + 4), W), (P, C.c_void_p(8194))):
        assert lib.gm_probe_cuscan_signature(1, 0, 1, o, w, None) == 1

    def scan(mask=15, iters=1, lo=1, hi=1, inj=None, cap=4, table=cus):
        return lib.gm_probe_cuscan(0, mask, iters, 0, lo, hi,
                                   C.byref(inj) if inj is not None else None, C.byref(res),
                                   table, cap, C.byref(n))
    assert scan(mask=0) == 1 and n.value == 0
    assert scan(mask=16) == 1
    assert scan(iters=0) == 1 and scan(iters=8192) == 1 and scan(mask=1, iters=65536) == 1
    assert scan(lo=0) == 1 and scan(lo=2, hi=1) == 1 and scan(hi=1025) == 1
    assert scan(cap=-1) == 1 and scan(cap=4, table=None) == 1
    inject = _native.CuscanInject
    for inj in (inject(0, 4, 0, 0, 0), inject(0, 6, 0, 0, 1), inject(0, 4, 256, 0, 1),
                inject(0, 4, 0, 4, 1), inject(4096, 4, 0, 0, 1)):
        assert scan(inj=inj) == 1
    assert scan(mask=1, inj=inject(0, 4, 0, 0, 1)) == 1          # a test that is not run
    assert lib.gm_probe_cuscan(0, 15, 1, 0, 1, 1, None, None, cus, 4, C.byref(n)) == 1


def test_structs_mirror_the_header():
    """Field-for-field mirrors of gm_cuscan_record_t, _inject_t, _cu_t and _result_t."""
    assert C.sizeof(_native.CuscanRecord) == 32
    assert C.sizeof(_native.CuscanInject) == 20
    assert C.sizeof(_native.CuscanCu) == 40
    assert _native.CuscanResult.blocks_run.offset == 16
    assert _native.CuscanResult.failed_cus.offset == 40
    assert _native.CuscanResult.xcc_cus.offset == 48
    assert _native.CuscanResult.records.offset == 48 + 64
    assert _native.CuscanResult.seconds.offset == 112 + 16 * 32
    assert C.sizeof(_native.CuscanResult) == 112 + 512 + 16


def test_command_lines_parse_the_cu_scan_options():
    from gpumounter_amd.cli import build_parser, cmd_probe

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.cu_scan is False and a.cu_scan_inject is None and a.cu_scan_rounds == 1
    assert tuple(a.cu_scan_tests) == cuscan.ALL_TESTS
    a = ap.parse_args(["probe", "--cu-scan", "--cu-scan-tests", "mfma,lds", "--cu-scan-rounds",
                       "3", "--cu-scan-inject", "any:mfma:0:0:1"])
    assert a.cu_scan and tuple(a.cu_scan_tests) == ("mfma", "lds") and a.cu_scan_rounds == 3
    assert a.cu_scan_inject == ("any", "mfma", 0, 0, 1)
    for bad in (["--cu-scan-tests", "int,fp64"], ["--cu-scan-inject", "any:mfma:0:0"],
                ["--cu-scan-inject", "any:mfma:0:0:0"], ["--cu-scan-rounds", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--cu-scan", *bad])
    # usage errors (2), not a failed scan (1), before any GPU work
    assert cmd_probe(ap.parse_args(["probe", "--cu-scan-inject", "any:mfma:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--cu-scan", "--cu-scan-tests", "int",
                                    "--cu-scan-inject", "any:mfma:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--cu-scan", "--cu-scan-rounds", "0"])) == 2
    assert ap.parse_args(["doctor", "--gpu", "--cu-scan"]).cu_scan is True
    assert ap.parse_args(["doctor", "--gpu"]).cu_scan is False


def test_doctor_passes_the_scan_on_and_names_the_unit(monkeypatch):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["cu_scan"].default is False and sig["cu_scan"].kind is sig["cu_scan"].KEYWORD_ONLY
    assert sig["cu_scan_inject"].default is None
    assert inspect.signature(doctor.run).parameters["cu_scan"].default is False

    calls = []

    def fake_scan(dev, _inject=None):
        calls.append((dev, _inject))
        bad = _inject is not None
        failed = [{"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "runs": 1, "failed_runs": 1,
                   "tests_failed": ["mfma"], "simds_failed": [2]}] if bad else []
        return {"cus_seen": 250, "cus_expected": 256, "complete": False, "rounds": 16,
                "kernel_ms": 1.0, "words_in_error": int(bad), "ok": not bad, "failed": failed}
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(cuscan, "scan", fake_scan)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "cu-scan" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, cu_scan=True) if c.name == "gpu0"]
    # an incomplete scan is stated and does not fail the check
    assert ok.status == "ok" and "cu-scan 250/256 CUs" in ok.detail and "incomplete" in ok.detail
    inj = (0x123, "mfma", 130, 2, 0x10000)
    (bad,) = [c for c in doctor.check_gpus(cfg, cu_scan=True, cu_scan_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail" and "xcc 1 se 1 sh 0 cu 3 (id 0x123) simd 2 mfma" in bad.detail
    assert calls == [(0, None), (0, inj)]


def test_describe_failed_names_four_units_and_counts_the_rest():
    unit = {"xcc": 2, "se": 1, "sh": 0, "cu": 5, "simds_failed": [1, 3],
            "tests_failed": ["int", "lds"]}
    six = [dict(unit, id=cuscan.encode_id(2, 1, 0, 5) + i, cu=5 + i) for i in range(6)]
    assert cuscan.describe_failed({"failed": six[:1]}) == (
        "xcc 2 se 1 sh 0 cu 5 (id 0x225) simd 1,3 int+lds")
    text = cuscan.describe_failed({"failed": six})
    assert text.count("xcc 2") == 4 and text.endswith("; and 2 more")
    assert cuscan.describe_failed({"failed": []}) == ""
