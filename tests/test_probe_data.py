"""Host side of the caller-owned-buffer probe entry points (gpumounter_amd/ops/probe.py,
native/include/gm_probe.h): argument validation before any HIP call, the ``--burn-in-flip``
parser and its plumbing into ``probe`` and ``doctor``. No GPU needed; what the kernels do to data
is covered by tests/test_probe_data_gpu.py."""
import ctypes as C
import inspect

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
