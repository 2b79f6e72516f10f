"""HBM pattern test, host side (gpumounter_amd/ops/memtest.py): the pattern function against an
independent numpy re-implementation of the formulas in native/include/gm_probe.h, argument
validation before any device call, sizing, and the command-line plumbing. No GPU needed; the
kernels are covered by tests/test_memtest_gpu.py."""
import inspect

import numpy as np
import pytest
import torch

from gpumounter_amd.ops import memtest
from gpumounter_amd.ops.probe import ProbeError

U32 = np.uint32
U64 = np.uint64
SEEDS = (0, 0x9E3779B97F4A7C15)
PASSES = (0, 1, 63)
BASES = (0, 2**32 - 64, 2**35 - 64)


def _rotl32(v, s):
    return (v << U32(s)) | (v >> U32(32 - s))


def reference(pattern: str, seed: int, pass_: int, base_offset: int, n_words: int):
    """The formulas of gm_probe.h in wrapping uint64 / uint32 numpy arithmetic."""
    o = U64(base_offset) + U64(8) * np.arange(n_words, dtype=U64)
    w = o >> U64(3)
    if pattern == "addr":
        return o ^ U64(seed)
    if pattern == "solid":
        return np.zeros(n_words, dtype=U64)
    if pattern == "checker":
        return np.full(n_words, 0x5555555555555555, dtype=U64)
    if pattern == "walk":
        return U64(1) << ((w + U64(pass_)) & U64(63))
    assert pattern == "random"
    k = (pass_ * 0x9E3779B9) & 0xFFFFFFFF
    v = w ^ U64(seed) ^ (U64(k) << U64(32))
    x = (v & U64(0xFFFFFFFF)).astype(U32)
    y = (v >> U64(32)).astype(U32)
    for c in (0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F):
        x = (_rotl32(x, 24) + y) ^ U32(c)
        y = _rotl32(y, 3) ^ x
    return (y.astype(U64) << U64(32)) | x.astype(U64)


@pytest.mark.parametrize("pattern", memtest.ALL_PATTERNS)
def test_expected_matches_the_documented_formulas(pattern):
    for seed in SEEDS:
        for pass_ in PASSES:
            for base in BASES:
                got = memtest.expected(pattern, seed, pass_, base, 32)
                assert got.dtype == np.uint64 and got.shape == (32,)
                np.testing.assert_array_equal(got, reference(pattern, seed, pass_, base, 32),
                                              err_msg=f"{pattern} {seed:#x} {pass_} {base:#x}")
    # by bit as well as by name
    np.testing.assert_array_equal(memtest.expected(memtest.PATTERNS[pattern], 5, 1, 64, 4),
                                  memtest.expected(pattern, 5, 1, 64, 4))


def test_random_pattern_uses_the_whole_word_index_and_every_data_bit():
    # offsets that differ only in bit 35 (word index bit 32): 32-bit word arithmetic aliases them
    a = memtest.expected("random", 7, 0, 4096, 1)[0]
    b = memtest.expected("random", 7, 0, 4096 + 2**35, 1)[0]
    assert a != b
    for base in (0, 2**35 - 64):
        v = memtest.expected("random", 7, 2, base, 4096)
        assert np.bitwise_or.reduce(v) == U64(0xFFFFFFFFFFFFFFFF)   # every bit is 1 somewhere
        assert np.bitwise_and.reduce(v) == U64(0)                   # and 0 somewhere
        assert len(np.unique(v)) == 4096                            # the mix is a bijection
    assert not np.array_equal(memtest.expected("random", 7, 0, 0, 64),
                              memtest.expected("random", 7, 1, 0, 64))
    assert not np.array_equal(memtest.expected("random", 7, 0, 0, 64),
                              memtest.expected("random", 8, 0, 0, 64))


def test_expected_refuses_bad_arguments():
    for bad in ("stripes", 3, 0, 32, None, True):
        with pytest.raises(ProbeError):
            memtest.expected(bad, 0, 0, 0, 4)
    with pytest.raises(ProbeError):
        memtest.expected("addr", 0, 0, 12, 4)           # not a word boundary
    with pytest.raises(ProbeError):
        memtest.expected("addr", -1, 0, 0, 4)
    with pytest.raises(ProbeError):
        memtest.expected("addr", 0, 2**32, 0, 4)


def test_memtest_validates_before_touching_the_gpu():
    """Every refusal below happens on the host, before a device is selected: none of them
    depends on a GPU being there."""
    for kw in (dict(nbytes=0), dict(nbytes=24), dict(nbytes=-16),
               dict(nbytes=1 << 20, patterns=("addr", "stripes")),
               dict(nbytes=1 << 20, patterns=()),
               dict(nbytes=1 << 20, passes=0), dict(nbytes=1 << 20, passes=1.5),
               dict(nbytes=1 << 20, chunk_bytes=100),
               dict(nbytes=1 << 20, _flip=(4, 1)),           # not a word boundary
               dict(nbytes=1 << 20, _flip=(1 << 20, 1))):    # outside the region
        with pytest.raises(ProbeError):
            memtest.memtest(0, **kw)


@pytest.mark.parametrize("fn", [memtest.fill, memtest.verify])
def test_fill_and_verify_validate_their_tensor(fn):
    cases = [
        torch.zeros(64, dtype=torch.uint8),                          # on the CPU
        torch.zeros(64, dtype=torch.float32),                        # dtype
        torch.zeros(16, 16, dtype=torch.uint8).t(),                  # not contiguous
        torch.zeros(128, dtype=torch.uint8)[::2],                    # not contiguous
        torch.zeros(24, dtype=torch.uint8),                          # size % 16
        torch.zeros(3, dtype=torch.int64),                           # size % 16
        torch.zeros(0, dtype=torch.uint8),                           # empty
    ]
    for t in cases:
        with pytest.raises(ProbeError):
            fn(t, "addr")
    with pytest.raises(ProbeError):
        fn(torch.zeros(64, dtype=torch.uint8), "stripes")
    with pytest.raises(ProbeError):
        fn(torch.zeros(64, dtype=torch.uint8), "addr", base_offset=4)
    with pytest.raises(ProbeError):
        fn([0] * 16, "addr")


def test_native_entry_points_validate_before_selecting_a_device():
    """Like the GEMM entry points, the C functions refuse bad arguments with
    hipErrorInvalidValue (1) before any HIP call, so this passes on a host without a GPU."""
    import ctypes as C

    from gpumounter_amd import _native

    lib = _native.probe()
    res = _native.MemtestResult()
    assert lib.gm_probe_memtest_fill(None, 64, 1, 0, 0, 0, 0, None) == 1
    assert lib.gm_probe_memtest_fill(C.c_void_p(4096 + 8), 64, 1, 0, 0, 0, 0, None) == 1
    assert lib.gm_probe_memtest_fill(C.c_void_p(4096), 24, 1, 0, 0, 0, 0, None) == 1
    assert lib.gm_probe_memtest_fill(C.c_void_p(4096), 0, 1, 0, 0, 0, 0, None) == 1
    assert lib.gm_probe_memtest_fill(C.c_void_p(4096), 64, 3, 0, 0, 0, 0, None) == 1
    assert lib.gm_probe_memtest_verify(C.c_void_p(4096), 24, 1, 0, 0, 0, 0, 0, None,
                                       C.byref(res)) == 1
    assert lib.gm_probe_memtest_verify(C.c_void_p(4096), 64, 32, 0, 0, 0, 0, 0, None,
                                       C.byref(res)) == 1
    for args in ((0, 0, 31, 1), (24, 0, 31, 1), (64, 8, 31, 1), (64, 0, 0, 1), (64, 0, 32, 1),
                 (64, 0, 31, 0)):
        assert lib.gm_probe_memtest(0, args[0], args[1], args[2], args[3], 0, 0, 0,
                                    C.byref(res)) == 1, args
    assert lib.gm_probe_memtest(0, 64, 0, 31, 1, 0, 64, 1, C.byref(res)) == 1    # flip outside
    out = (C.c_uint64 * 4)()
    assert lib.gm_probe_memtest_expected(3, 0, 0, 0, 4, out) == 1
    assert lib.gm_probe_memtest_expected(1, 0, 0, 4, 4, out) == 1


def test_result_struct_mirrors_the_header():
    """Field-for-field mirror of gm_memtest_result_t: 4 × u64, 2 × u32, 16 records of 32 bytes,
    4 doubles."""
    import ctypes as C

    from gpumounter_amd import _native

    assert C.sizeof(_native.MemtestRecord) == 32
    assert C.sizeof(_native.MemtestResult) == 4 * 8 + 2 * 4 + 16 * 32 + 4 * 8
    assert _native.MemtestResult.records.offset == 40
    assert _native.MemtestResult.seconds.offset == 40 + 512


def test_plan_bytes():
    assert memtest.plan_bytes(1000, 2000) == 896                   # 900 rounded down to 16
    assert memtest.plan_bytes(1 << 30, 1 << 31, 0.5) == 1 << 29
    assert memtest.plan_bytes(100, 100, 1.0) == 96
    assert memtest.plan_bytes(288 * 10**9, 288 * 10**9) % 16 == 0
    assert memtest.plan_bytes(18, 100) == 16
    for free, total, frac in ((1000, 2000, 1.5), (1000, 2000, 0.0), (1000, 2000, -0.1),
                              (15, 2000, 1.0), (17, 2000, 0.9), (0, 2000, 0.9),
                              (3000, 2000, 0.9)):
        with pytest.raises(ProbeError):
            memtest.plan_bytes(free, total, frac)


def test_parse_size():
    assert memtest.parse_size("123456") == 123456
    assert memtest.parse_size("64M") == 64 << 20
    assert memtest.parse_size("8G") == 8 << 30
    assert memtest.parse_size("16k") == 16 << 10
    assert memtest.parse_size(" 1T ") == 1 << 40
    for bad in ("12Q", "", "G", "1.5G", "-4M", "0x10"):
        with pytest.raises(ProbeError):
            memtest.parse_size(bad)


def test_probe_command_line_parses_the_memtest_options():
    from gpumounter_amd.cli import build_parser

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.memtest is None and a.memtest_flip is None and a.memtest_passes == 1
    assert tuple(a.memtest_patterns) == memtest.ALL_PATTERNS
    a = ap.parse_args(["probe", "--memtest"])
    assert a.memtest == -1                               # automatic size
    a = ap.parse_args(["probe", "--memtest", "64M", "--memtest-flip", "4096:0x10",
                       "--memtest-patterns", "addr,random", "--memtest-passes", "3"])
    assert a.memtest == 64 << 20 and a.memtest_flip == (4096, 0x10)
    assert tuple(a.memtest_patterns) == ("addr", "random") and a.memtest_passes == 3
    for bad in (["--memtest", "12Q"], ["--memtest-flip", "4096"], ["--memtest-flip", "a:b"],
                ["--memtest-patterns", "addr,stripes"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", *bad])
    a = ap.parse_args(["doctor", "--gpu", "--memtest", "1G"])
    assert a.memtest == 1 << 30
    assert ap.parse_args(["doctor", "--gpu"]).memtest is None


def test_doctor_keeps_its_behaviour_without_the_new_arguments(monkeypatch):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    assert inspect.signature(doctor.run).parameters["memtest_bytes"].default == 0
    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["memtest_bytes"].default == 0 and sig["memtest_bytes"].kind is sig[
        "memtest_bytes"].KEYWORD_ONLY
    assert list(sig)[:2] == ["cfg", "burn_in_s"] and sig["burn_in_s"].default == 0.0

    calls = []
    for name in ("check_inventory", "check_cgroup", "check_devnodes", "check_pidns",
                 "check_systemd"):
        monkeypatch.setattr(doctor, name, lambda cfg: [])

    def fake_check_gpus(cfg, burn_in_s=0.0, **kw):
        calls.append((burn_in_s, kw))
        return []
    monkeypatch.setattr(doctor, "check_gpus", fake_check_gpus)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    doctor.run(cfg, skip_cluster=True)
    assert calls == []                                   # --gpu not given: no GPU check at all
    doctor.run(cfg, skip_cluster=True, gpu=True, burn_in_s=2.0)
    assert calls == [(2.0, {"memtest_bytes": 0})]
    doctor.run(cfg, skip_cluster=True, gpu=True, memtest_bytes=1 << 20)
    assert calls[-1] == (0.0, {"memtest_bytes": 1 << 20})


def test_doctor_memtest_fails_cleanly_without_a_gpu(monkeypatch):
    """On a host whose GPUs HIP cannot see, asking for the memtest changes nothing: one failed
    ``gpu`` check, no exception. (Where a GPU is present, HIP is made to report none; the
    passing case runs in tests/test_memtest_gpu.py.)"""
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    if torch.cuda.is_available():
        monkeypatch.setattr(probe, "device_count", lambda: 0)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    checks = doctor.check_gpus(cfg, memtest_bytes=1 << 20)
    assert len(checks) == 1 and checks[0].name == "gpu" and checks[0].status == "fail", checks
