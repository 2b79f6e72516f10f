"""Host side of the caller-owned-buffer probe entry points (gpumounter_amd/ops/probe.py,
native/include/gm_probe.h): argument validation before any HIP call, the ``--burn-in-flip``
parser and its plumbing into ``probe`` and ``doctor``, and the liveness probe's expected table
and verdict (native/include/gm_quick_ref.h). No GPU needed; what the kernels do to data
is covered by tests/test_probe_data_gpu.py."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from gpumounter_amd import _native
from gpumounter_amd.ops import probe

P = C.c_void_p(4096)          # never dereferenced: every call below is refused first
Q = C.c_void_p(8192)


def test_new_entry_points_validate_before_any_hip_call():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    n = C.c_uint64(7)
    for a, b, nbytes in ((None, Q, 64), (P, None, 64), (C.c_void_p(4096 + 8), Q, 64),
                         (P, C.c_void_p(8192 + 4), 64), (P, Q, 0), (P, Q, 24)):
        assert lib.gm_probe_count_diff(a, b, nbytes, None, C.byref(n)) == 1
        assert n.value == 0
    assert lib.gm_probe_count_diff(P, Q, 64, None, None) == 1
    assert lib.gm_probe_fill_bf16(None, 8, 1, None) == 1
    assert lib.gm_probe_fill_bf16(C.c_void_p(4097), 8, 1, None) == 1
    assert lib.gm_probe_fill_bf16(P, 0, 1, None) == 1
    for variant, src, dst, nbytes, bpc in ((7, P, Q, 64, 8), (-1, P, Q, 64, 8), (2, P, Q, 24, 8),
                                           (2, P, Q, 0, 8), (2, P, Q, 64, 0), (2, None, Q, 64, 8),
                                           (2, P, None, 64, 8), (2, C.c_void_p(4100), Q, 64, 8),
                                           (2, P, C.c_void_p(4096 + 48), 64, 8)):   # overlap
        assert lib.gm_probe_copy(variant, src, dst, nbytes, bpc, None) == 1
    for src, sink, nbytes, bpc in ((None, Q, 64, 2), (P, None, 64, 2), (P, C.c_void_p(8194), 64, 2),
                                   (P, Q, 24, 2), (P, Q, 0, 2), (P, Q, 64, 0)):
        assert lib.gm_probe_read(src, sink, nbytes, bpc, None) == 1
    g = C.c_double(5)
    for variant in (7, -1):
        assert lib.gm_probe_hbm_copy_variant(0, variant, 1 << 20, 1, 8, C.byref(g)) == 1
        assert g.value == 0


def test_burn_in_flip_validates_before_selecting_a_device():
    lib = _native.probe()
    tf, bad, it = C.c_double(0), C.c_uint64(0), C.c_int(0)
    out = (C.byref(tf), C.byref(bad), C.byref(it))
    one = (C.c_uint64 * 1)(0), (C.c_uint16 * 1)(1)
    assert lib.gm_probe_burn_in_flip(0, 300, 1.0, 1, *one, *out) == 1          # n % 256
    assert lib.gm_probe_burn_in_flip(0, 256, 0.0, 1, *one, *out) == 1
    assert lib.gm_probe_burn_in_flip(0, 256, 1.0, -1, None, None, *out) == 1
    assert lib.gm_probe_burn_in_flip(0, 256, 1.0, 1, None, None, *out) == 1
    for elems, masks in (([256 * 256], [1]), ([0], [0]), ([9, 9], [1, 2])):
        fe, fm = (C.c_uint64 * len(elems))(*elems), (C.c_uint16 * len(elems))(*masks)
        assert lib.gm_probe_burn_in_flip(0, 256, 1.0, len(elems), fe, fm, *out) == 1
    for flips in ([(256 * 256, 1)], [(0, 0)], [(0, 1 << 16)], [(-1, 1)], [(0, 1.0)],
                  [(3, 1), (3, 4)]):
        with pytest.raises(probe.ProbeError):
            probe.burn_in(0, 1.0, 256, _flips=flips)


def test_wrappers_validate_their_tensors():
    z = torch.zeros(64, dtype=torch.uint8)                       # on the CPU
    sink = torch.zeros(probe.READ_SINK_WORDS, dtype=torch.int32)
    for call in (lambda: probe.count_diff(z, z), lambda: probe.copy(2, z, z.clone()),
                 lambda: probe.read(z, sink),
                 lambda: probe.fill_bf16(torch.zeros(8, dtype=torch.bfloat16), 1),
                 lambda: probe.fill_bf16(torch.zeros(8, dtype=torch.float32), 1),
                 lambda: probe.fill_bf16([0] * 8, 1), lambda: probe.count_diff([0] * 16, z)):
        with pytest.raises(probe.ProbeError):
            call()


# ------------------------------------------------------------------ liveness probe verdict
QUICK_SALTS = (0, 1, 0x9E3779B9, 0x9E3779B9 ^ 3, 0xFFFFFFFF, 0x80000001)


def _quick_reference(salt: int) -> np.ndarray:
    """gm_probe.h's formula in numpy: uint64 arithmetic reduced mod 2^32 at the end."""
    lanes = ((np.arange(64, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) \
        ^ np.uint64(salt)
    return np.concatenate([lanes, [lanes.sum() & np.uint64(0xFFFFFFFF)], [64]]).astype(np.uint32)


def _check_of(word: int) -> int:
    return (probe.QUICK_BAD_LANES if word < 64 else
            probe.QUICK_BAD_SUM if word == 64 else probe.QUICK_BAD_BALLOT)


@pytest.mark.parametrize("salt", QUICK_SALTS)
def test_quick_expected_table_is_the_documented_formula(salt):
    want = _quick_reference(salt)
    got = probe.quick_expected(salt)
    assert len(got) == probe.QUICK_WORDS == 66
    np.testing.assert_array_equal(np.array(got, dtype=np.uint32), want)
    assert probe.quick_verdict(got, salt) == 0
    assert probe.quick_verdict([int(w) for w in want], salt) == 0


@pytest.mark.parametrize("salt", QUICK_SALTS[:3])
def test_quick_verdict_fails_every_single_bit_flip_and_names_the_check(salt):
    lib = _native.probe()
    want = probe.quick_expected(salt)
    buf, failed = (C.c_uint32 * 66)(*want), C.c_uint32(0)
    for word in range(66):
        for bit in range(32):
            buf[word] = want[word] ^ (1 << bit)
            failed.value = 0
            assert lib.gm_probe_quick_verdict(buf, salt, C.byref(failed)) == 0
            assert failed.value == _check_of(word), (word, bit, failed.value)
        buf[word] = want[word]
    assert lib.gm_probe_quick_verdict(buf, salt, C.byref(failed)) == 0 and failed.value == 0


def test_quick_verdict_fails_a_wave32_ballot_and_another_salts_table():
    salt = 0x9E3779B9
    want = probe.quick_expected(salt)
    assert probe.quick_verdict(want[:65] + [32], salt) == probe.QUICK_BAD_BALLOT
    assert probe.quick_verdict(want[:65] + [0], salt) == probe.QUICK_BAD_BALLOT
    # a sum that agrees with wrong lane words is still wrong lane words, and a right sum over
    # them is a wrong sum only if it differs from the table's
    other = probe.quick_expected(salt ^ 1)          # device 1's table judged as device 0's
    assert other[:64] != want[:64]
    assert probe.quick_verdict(other, salt) & probe.QUICK_BAD_LANES
    assert probe.quick_verdict(other, salt ^ 1) == 0
    for s2 in (0, 0x12345678, salt ^ 0x80000000):
        o = probe.quick_expected(s2)
        bad = probe.quick_verdict(o, salt)
        assert bad & probe.QUICK_BAD_LANES and not bad & probe.QUICK_BAD_BALLOT
        assert bool(bad & probe.QUICK_BAD_SUM) == (o[64] != want[64])
    # lane 63 alone, and the three at once
    assert probe.quick_verdict(want[:63] + [want[63] ^ 1] + want[64:], salt) \
        == probe.QUICK_BAD_LANES
    assert probe.quick_verdict([w ^ 0x100 for w in want], salt) == 7
    with pytest.raises(probe.ProbeError):
        probe.quick_verdict(want[:65], salt)


def test_quick_entry_points_refuse_before_any_hip_call():
    """hipErrorInvalidValue (1) with no device selected: a HIP call would have failed otherwise."""
    lib = _native.probe()
    ok, failed, us = C.c_int(7), C.c_uint32(7), C.c_double(0)
    out = (C.byref(ok), C.byref(failed), C.byref(us))
    for word, mask in ((66, 1), (67, 0x8000), (0xFFFFFFFF, 1), (0, 0), (65, 0)):
        assert lib.gm_probe_quick_flip(0, word, mask, *out) == 1, (word, mask)
        assert ok.value == 0 and failed.value == 0
        with pytest.raises(probe.ProbeError, match="hip error 1 "):
            probe.quick(0, _flip=(word, mask))
    assert lib.gm_probe_quick_flip(0, 0, 1, None, C.byref(failed), C.byref(us)) == 1
    for flip in ((-1, 1), (0, 1 << 32), (0.0, 1), (0, True)):
        with pytest.raises(probe.ProbeError, match="flip"):
            probe.quick(0, _flip=flip)
    buf = (C.c_uint32 * 66)()
    assert lib.gm_probe_quick_expected(0, None) == 1
    assert lib.gm_probe_quick_verdict(None, 0, C.byref(failed)) == 1
    assert lib.gm_probe_quick_verdict(buf, 0, None) == 1
    assert lib.gm_probe_quick_words(0, None, C.byref(failed)) == 1
    assert lib.gm_probe_quick_words(0, buf, None) == 1
    assert inspect.signature(probe.quick).parameters["_flip"].default is None


# ------------------------------------------------------------------ MFMA peak values, 64² GEMM
def test_mfma_peak_values_refuses_before_any_hip_call():
    lib = _native.probe()
    for variant, iters, blocks, ptr in ((3, 1, 1, P), (-1, 1, 1, P), (0, 0, 1, P), (1, -5, 1, P),
                                        (2, 1, 0, P), (2, 1, -1, P), (0, 1, 1, None),
                                        (0, 1, 1, C.c_void_p(4096 + 4)),
                                        (1, 1, 1, C.c_void_p(4096 + 8))):
        assert lib.gm_probe_mfma_peak_values(variant, iters, 1.0, blocks, ptr, None) == 1
    cpu = torch.zeros(3 * 256 * 16, dtype=torch.float32)
    for call in (lambda: probe.mfma_peak_values(3, 1, 1.0, 3),
                 lambda: probe.mfma_peak_values(1, 1, 1.0, 0),
                 lambda: probe.mfma_peak_values(1, 1, 1.0, 3, out=cpu),                 # device
                 lambda: probe.mfma_peak_values(0, 1, 1.0, 3, out=cpu),                 # size
                 lambda: probe.mfma_peak_values(1, 1, 1.0, 3, out=cpu.to(torch.int32))):
        with pytest.raises(probe.ProbeError):
            call()


def test_gemm_bf16_validates_out_before_any_hip_call():
    """Operands on the CPU: anything but the refusal would need a device."""
    bf = torch.bfloat16
    a, b = torch.zeros(64, 32, dtype=bf), torch.zeros(32, 128, dtype=bf)
    for out in (torch.zeros(64, 128, dtype=bf),                      # half the bytes the kernel writes
                torch.zeros(64, 128, dtype=torch.float64),
                torch.zeros(64, 64, dtype=torch.float32),            # undersized
                torch.zeros(128, 64, dtype=torch.float32),           # transposed shape
                torch.zeros(64 * 128, dtype=torch.float32),          # right size, wrong rank
                torch.zeros(128, 64, dtype=torch.float32).t(),       # right shape, not contiguous
                torch.zeros(64, 256, dtype=torch.float32)[:, ::2],
                torch.empty(64, 128, dtype=torch.float32, device="meta"),   # another device
                [0.0] * (64 * 128)):
        with pytest.raises(probe.ProbeError, match="out must be"):
            probe.gemm_bf16(a, b, out=out)
    with pytest.raises(probe.ProbeError, match="A on"):
        probe.gemm_bf16(a, torch.empty(32, 128, dtype=bf, device="meta"))
    assert list(inspect.signature(probe.gemm_bf16).parameters) == ["a", "b", "out", "stream"]


def test_parse_burn_in_flip():
    assert probe.parse_burn_in_flip("0:0x1") == (0, 1)
    assert probe.parse_burn_in_flip("4096:0x8000") == (4096, 0x8000)
    assert probe.parse_burn_in_flip(" 12 : 65535 ") == (12, 0xFFFF)
    for bad in ("4096", "a:b", "1:2:3", "-1:1", "0:0", "0:0x10000", "", "1.5:1"):
        with pytest.raises(probe.ProbeError):
            probe.parse_burn_in_flip(bad)


def test_probe_command_line_parses_burn_in_flip():
    from gpumounter_amd.cli import build_parser, cmd_probe

    ap = build_parser()
    assert ap.parse_args(["probe", "--burn-in", "1"]).burn_in_flip is None
    a = ap.parse_args(["probe", "--burn-in", "1", "--burn-in-flip", "0:0x1",
                       "--burn-in-flip", "8:0x8000"])
    assert a.burn_in == 1.0 and a.burn_in_flip == [(0, 1), (8, 0x8000)]
    for bad in ("4096", "a:b", "0:0", "0:0x10000"):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--burn-in", "1", "--burn-in-flip", bad])
    # without --burn-in the flip is a usage error (2), not a failed burn-in (1), before any GPU work
    assert cmd_probe(ap.parse_args(["probe", "--burn-in-flip", "0:1"])) == 2


def test_burn_in_and_doctor_pass_the_flips_on(monkeypatch):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["burn_in_flip"].default is None
    assert sig["burn_in_flip"].kind is sig["burn_in_flip"].KEYWORD_ONLY
    assert inspect.signature(probe.burn_in).parameters["_flips"].default is None

    calls = []

    def fake_burn_in(dev, seconds=10.0, n=8192, _flips=None):
        calls.append((dev, seconds, _flips))
        bad = 16 if _flips else 0
        return {"device": dev, "n": n, "seconds": seconds, "iterations": 16, "tflops": 1000.0,
                "mismatches": bad, "ok": bad == 0}
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(probe, "burn_in", fake_burn_in)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (ok,) = [c for c in doctor.check_gpus(cfg, 2.0) if c.name == "gpu0"]
    assert ok.status == "ok" and " 0 mismatching words" in ok.detail
    (bad,) = [c for c in doctor.check_gpus(cfg, 2.0, burn_in_flip=[(0, 1)]) if c.name == "gpu0"]
    assert bad.status == "fail" and " 16 mismatching words" in bad.detail
    assert calls == [(0, 2.0, None), (0, 2.0, [(0, 1)])]
