"""The block-scaled (MX) GEMM burn-in without a GPU (gpumounter_amd/ops/mxgemm.py; formulas in
native/include/gm_probe.h): the fills and the GEMM's definition written again in numpy from that
text, against ``mxgemm.expected`` bit for bit; the exactness conditions of the ``exact`` and
``blocks`` classes for the shapes tests/test_mxgemm_gpu.py runs; the ``random`` class's codes; the
refusals, all raised before the native call; the command lines; and the probe / doctor / validate
wiring with the burn-ins stubbed."""
import inspect
import json

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import mxgemm, probe
from gpumounter_amd.ops.probe import ProbeError

# ------------------------------------------------------------------ the model, again, in numpy
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
E4M3_OF_E2M1 = np.array([0x00, 0x30, 0x38, 0x3C, 0x40, 0x44, 0x48, 0x4C], np.uint32)
BLOCKS_NIBBLES = np.array([0, 2, 4, 10, 12], np.uint32)          # 0, 1, 2, -1, -2
SCALE_SALT = 0x5CA1E5CA


def h(i, seed):
    with np.errstate(over="ignore"):
        x = (np.asarray(i).astype(np.uint32) * np.uint32(2654435761)) ^ np.uint32(seed)
        x ^= x >> np.uint32(15)
        x = x * np.uint32(2246822519)
        x ^= x >> np.uint32(13)
    return x


def codes(fmt, cls, seed, rows, k):
    """Element codes [rows, k]: nibbles (mxfp4) or e4m3 bytes (mxfp8)."""
    H = h(np.arange(rows * k, dtype=np.uint64), seed).reshape(rows, k)
    if cls == "random" and fmt == "mxfp8":
        b = H >> 24
        return np.where((b & 0x7F) == 0x7F, (b & 0x80) | ((H >> 8) & 0x7E), b)
    n = BLOCKS_NIBBLES[(H >> 8) % 5] if cls == "blocks" else H >> 28
    return n if fmt == "mxfp4" else E4M3_OF_E2M1[n & 7] | (n & 8) << 4


def decode(fmt, c):
    """Codes → float64, from the formats' definitions (e2m1; OCP e4m3: bias 7, subnormals)."""
    c = c.astype(np.int64)
    if fmt == "mxfp4":
        return np.where(c & 8, -1.0, 1.0) * E2M1[c & 7]
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    return np.where(c & 0x80, -1.0, 1.0) * mag


def scales(cls, seed, rows, kblocks):
    s = seed ^ SCALE_SALT
    if cls == "exact":
        return np.repeat(125 + (h(np.arange(rows), s) >> 30)[:, None], kblocks, axis=1)
    H = h(np.arange(rows * kblocks), s).reshape(rows, kblocks)
    return 127 + (H >> 31) if cls == "blocks" else 123 + (H >> 29)


def values(fmt, cls, seed, rows, k):
    """The scaled operand, float64 [rows, k] (every entry exact)."""
    sc = scales(cls, seed, rows, k // 32).astype(np.float64)
    return decode(fmt, codes(fmt, cls, seed, rows, k)) * np.repeat(2.0 ** (sc - 127), 32, axis=1)


def bf16_bits(x):
    """float64 that is exact in fp32 → bf16 bits, rounded to nearest even."""
    f = x.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), x)
    u = f.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def model(fmt, cls, seed_a, seed_b, m, n, k):
    a, b = values(fmt, cls, seed_a, m, k), values(fmt, cls, seed_b, n, k)
    if cls != "random":
        return bf16_bits(a @ b.T + 0.0)              # exact in float64; -0.0 + 0.0 = +0.0
    ref, s = np.zeros((m, n)), np.zeros((m, n))
    for kk in range(k):                              # the sum in k order
        p = a[:, kk, None] * b[None, :, kk]
        ref += p
        s += np.abs(p)
    return ref, s


SEEDS = ((0x5151, 0xA3A3), (7, 0xDEADBEEF))
# the shapes of tests/test_mxgemm_gpu.py: M, N, K-tiles
GPU_EXACT_SHAPES = ((256, 256, 1), (256, 256, 2), (256, 256, 3), (512, 768, 4), (2304, 256, 2))


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
@pytest.mark.parametrize("cls", mxgemm.CLASSES)
def test_expected_equals_the_numpy_model_bit_for_bit(fmt, cls):
    for sa, sb in SEEDS:
        got, want = mxgemm.expected(fmt, cls, sa, sb, 64, 64, 512), model(fmt, cls, sa, sb, 64, 64,
                                                                          512)
        if cls == "random":
            for g, w in zip(got, want):
                assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64),
                                                                w.view(np.uint64))
            assert np.all(got[1] >= np.abs(got[0])) and np.any(got[0] != 0)
        else:
            assert got.dtype == np.uint16 and np.array_equal(got, want)
            assert len(np.unique(got)) > 64          # not a constant
    a = mxgemm.expected(fmt, cls, 1, 2, 32, 32, 64)
    b = mxgemm.expected(fmt, cls, 1, 3, 32, 32, 64)
    assert not np.array_equal(a[0] if cls == "random" else a, b[0] if cls == "random" else b)


def test_the_classes_hold_what_the_header_says():
    for fmt in mxgemm.FORMATS:
        for sa, _ in SEEDS:
            ex = decode(fmt, codes(fmt, "exact", sa, 64, 512))
            assert set(np.unique(np.abs(ex))) == set(E2M1)         # all 16 values: both signs
            assert np.any(ex < 0) and np.any(np.signbit(ex) & (ex == 0))
            bl = decode(fmt, codes(fmt, "blocks", sa, 64, 512))
            assert set(np.unique(bl)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
            s = scales("exact", sa, 64, 16)
            assert set(np.unique(s)) == {125, 126, 127, 128} and np.all(s == s[:, :1])
            s = scales("blocks", sa, 64, 16)
            assert set(np.unique(s)) == {127, 128} and np.any(s != s[:, :1])
            s = scales("random", sa, 64, 16)
            assert set(np.unique(s)) == set(range(123, 131))
    # the random class: every nibble; every e4m3 byte but the two NaN codes, about uniformly
    c4 = codes("mxfp4", "random", 0x5151, 256, 1024)
    assert set(np.unique(c4)) == set(range(16))
    c8 = codes("mxfp8", "random", 0x5151, 256, 1024)
    assert set(np.unique(c8)) == set(range(256)) - {0x7F, 0xFF}
    count = np.bincount(c8.ravel().astype(np.int64), minlength=256)
    assert count[[0x7F, 0xFF]].sum() == 0 and np.delete(count, [0x7F, 0xFF]).min() > 700
    assert np.isfinite(decode("mxfp8", c8)).all() and np.abs(decode("mxfp8", c8)).max() == 448


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
def test_exact_and_blocks_sum_exactly_at_the_gpu_tests_shapes(fmt):
    """In units of 2^-6 (the smallest product of the smallest scales) every product is an
    integer, and for one output the sum of their magnitudes stays below 2^24: every partial sum,
    in any order, is then an integer of at most 24 bits, i.e. an exact fp32. For `blocks` also
    what the header states: products span 4 bits, a 128-term sum 11."""
    tk = mxgemm.TILE_K[fmt]
    for cls in ("exact", "blocks"):
        for m, n, tiles in GPU_EXACT_SHAPES:
            k = tiles * tk
            a, b = values(fmt, cls, 0x5151, m, k) * 8, values(fmt, cls, 0xA3A3, n, k) * 8
            assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b))
            total = np.abs(a) @ np.abs(b).T                # units of 2^-6, exact in float64
            assert total.max() < 2 ** 24, (cls, m, n, k, total.max())
            if cls == "blocks":
                assert np.abs(a).max() == 32 and np.abs(b).max() == 32     # 4 in units of 2^-3
                per_step = np.abs(a[:, :128]) @ np.abs(b[:, :128]).T / 64
                assert per_step.max() <= 2048 and (np.abs(a) / 8).max() ** 2 == 16


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
def test_random_is_finite_at_k_8192(fmt):
    ref, s = mxgemm.expected(fmt, "random", 0x5151, 0xA3A3, 16, 16, 8192)
    assert np.isfinite(ref).all() and np.isfinite(s).all() and np.all(s > 0)
    assert np.abs(ref).max() < 3.0e38 / 2 ** 16            # far from fp32's and bf16's range
    if fmt == "mxfp8":
        c = codes(fmt, "random", 0x5151, 16, 8192)
        assert not np.any((c & 0x7F) == 0x7F)


# ------------------------------------------------------------------ refusals, parsers, wiring
def test_every_refusal_comes_before_the_native_call(monkeypatch):
    import torch

    def no_native():
        raise AssertionError("the native library was called")
    monkeypatch.setattr(_native, "probe", no_native)
    for bad in ("fp8", "mxfp6", 0, None):
        with pytest.raises(ProbeError):
            mxgemm.expected(bad, "exact", 1, 2, 32, 32, 32)
        with pytest.raises(ProbeError):
            mxgemm.burn_in(0, 1.0, bad, n=256)
        with pytest.raises(ProbeError):
            mxgemm.kernel_info(bad)
        with pytest.raises(ProbeError):
            mxgemm.fill(bad, "exact", 1, 256, 256)
    for bad in ("exactly", 2, None):
        with pytest.raises(ProbeError):
            mxgemm.expected("mxfp8", bad, 1, 2, 32, 32, 32)
        with pytest.raises(ProbeError):
            mxgemm.fill("mxfp8", bad, 1, 256, 256)
    for m, n, k in ((32, 32, 48), (0, 32, 32), (32, -1, 32), (32, 32, 0), (32.0, 32, 32)):
        with pytest.raises(ProbeError):
            mxgemm.expected("mxfp4", "blocks", 1, 2, m, n, k)
    for seed in (-1, 1 << 32, 1.5, True):
        with pytest.raises(ProbeError):
            mxgemm.expected("mxfp4", "blocks", seed, 2, 32, 32, 32)
    # the kernel's shapes: M, N multiples of 256, K of 128 (fp8) or 256 (fp4)
    for fmt, m, n, k in (("mxfp8", 128, 256, 128), ("mxfp8", 256, 384, 128),
                         ("mxfp8", 256, 256, 64), ("mxfp8", 256, 256, 192),
                         ("mxfp4", 256, 256, 128), ("mxfp4", 256, 256, 384),
                         ("mxfp4", 300, 256, 256)):
        with pytest.raises(ProbeError):
            mxgemm.check_shape(fmt, m, n, k)
        a = torch.zeros((m, mxgemm.row_bytes(fmt, k)), dtype=torch.uint8)
        bt = torch.zeros((n, mxgemm.row_bytes(fmt, k)), dtype=torch.uint8)
        sa = torch.zeros((m, k // 32), dtype=torch.uint8)
        sb = torch.zeros((n, k // 32), dtype=torch.uint8)
        with pytest.raises(ProbeError):
            mxgemm.gemm_nt(fmt, a, sa, bt, sb)
    mxgemm.check_shape("mxfp8", 256, 512, 384)
    mxgemm.check_shape("mxfp4", 2304, 256, 512)
    cpu = [torch.zeros((256, 128), dtype=torch.uint8), torch.zeros((256, 4), dtype=torch.uint8)]
    with pytest.raises(ProbeError):                        # not on a HIP device
        mxgemm.gemm_nt("mxfp8", cpu[0], cpu[1], cpu[0], cpu[1])
    with pytest.raises(ProbeError):
        mxgemm.gemm_nt("mxfp8", cpu[0].numpy(), cpu[1], cpu[0], cpu[1])
    for n in (0, 128, 384, 8192 + 128):
        with pytest.raises(ProbeError):
            mxgemm.burn_in(0, 1.0, "mxfp4", n=n)
    for seconds in (0, -1.0, None):
        with pytest.raises(ProbeError):
            mxgemm.burn_in(0, seconds, "mxfp8", n=256)
    for flips in ([(256 * 256, 1)], [(-1, 1)], [(0, 0)], [(0, 1 << 16)], [(0, 1), (0, 2)],
                  [(0.0, 1)]):
        with pytest.raises(ProbeError):
            mxgemm.burn_in(0, 1.0, "mxfp8", n=256, _flips=flips)


def test_native_entry_points_validate_before_selecting_a_device():
    import ctypes as C

    lib = _native.probe()
    out = (C.byref(C.c_double()), C.byref(C.c_uint64()), C.byref(C.c_int()))
    one = ((C.c_uint64 * 1)(0), (C.c_uint16 * 1)(1))
    invalid = 1                                            # hipErrorInvalidValue
    assert lib.gm_probe_mx_burn_in_flip(0, 1, 256, 1.0, 0, None, None, *out) == invalid
    assert lib.gm_probe_mx_burn_in_flip(0, 0, 300, 1.0, 0, None, None, *out) == invalid
    assert lib.gm_probe_mx_burn_in_flip(0, 4, 128, 1.0, 0, None, None, *out) == invalid
    assert lib.gm_probe_mx_burn_in_flip(0, 4, 256, 0.0, 1, *one, *out) == invalid
    assert lib.gm_probe_mx_burn_in_flip(0, 0, 256, 1.0, 1, None, None, *out) == invalid
    bad = ((C.c_uint64 * 1)(256 * 256), (C.c_uint16 * 1)(1))
    assert lib.gm_probe_mx_burn_in_flip(0, 0, 256, 1.0, 1, *bad, *out) == invalid
    p = C.c_void_p(4096)                                   # never dereferenced: refused first
    assert lib.gm_probe_mxgemm_nt(0, p, p, p, p, p, 256, 256, 64, None) == invalid
    assert lib.gm_probe_mxgemm_nt(4, p, p, p, p, p, 256, 256, 128, None) == invalid
    assert lib.gm_probe_mxgemm_nt(0, p, p, p, p, p, 128, 256, 128, None) == invalid
    assert lib.gm_probe_mxgemm_nt(2, p, p, p, p, p, 256, 256, 256, None) == invalid
    assert lib.gm_probe_mxgemm_nt(0, C.c_void_p(4100), p, p, p, p, 256, 256, 128, None) == invalid
    assert lib.gm_probe_mxgemm_nt(0, p, None, p, p, p, 256, 256, 128, None) == invalid
    assert lib.gm_probe_mx_fill(0, 3, 1, 256, 256, p, p, None) == invalid
    assert lib.gm_probe_mx_fill(0, 0, 1, 256, 48, p, p, None) == invalid
    assert lib.gm_probe_mx_fill(0, 0, 1, 256, 64, None, p, None) == invalid
    assert lib.gm_probe_mxgemm_expected(0, 0, 1, 2, 32, 32, 32, None, None, None) == invalid
    assert lib.gm_probe_mxgemm_expected(0, 2, 1, 2, 32, 32, 32, p, None, None) == invalid
    assert lib.gm_probe_mxgemm_kernel_info(1, C.byref(C.c_int()), C.byref(C.c_int())) == invalid


def test_parse_burn_in_formats():
    assert mxgemm.BURN_IN_FORMATS == ("bf16", "mxfp8", "mxfp4")
    assert mxgemm.parse_burn_in_formats("bf16") == ("bf16",)
    assert mxgemm.parse_burn_in_formats("mxfp4, bf16") == ("bf16", "mxfp4")
    assert mxgemm.parse_burn_in_formats("mxfp8,mxfp4,mxfp8") == ("mxfp8", "mxfp4")
    for bad in ("", "fp8", "bf16,", "mxfp6"):
        with pytest.raises(ProbeError):
            mxgemm.parse_burn_in_formats(bad)
    assert [mxgemm.burn_in_key(f) for f in mxgemm.BURN_IN_FORMATS] == [
        "burn_in", "burn_in_mxfp8", "burn_in_mxfp4"]


def test_command_lines_parse_the_formats_and_refuse_them_without_a_burn_in(capsys):
    from gpumounter_amd.cli import build_parser, cmd_doctor, cmd_probe
    from gpumounter_amd.parallel import validate

    ap = build_parser()
    for tool in ("probe", "doctor"):
        assert ap.parse_args([tool, "--burn-in", "1"]).burn_in_format is None
        a = ap.parse_args([tool, "--burn-in", "1", "--burn-in-format", "mxfp4,bf16",
                           "--burn-in-flip", "0:0x1"])
        assert a.burn_in_format == ("bf16", "mxfp4") and a.burn_in_flip == [(0, 1)]
        with pytest.raises(SystemExit) as e:
            ap.parse_args([tool, "--burn-in", "1", "--burn-in-format", "fp8"])
        assert e.value.code == 2
    # without --burn-in: a usage error (2) before any GPU work, not a failed burn-in (1)
    assert cmd_probe(ap.parse_args(["probe", "--burn-in-format", "mxfp8"])) == 2
    assert "--burn-in-format needs --burn-in" in capsys.readouterr().err
    assert cmd_doctor(ap.parse_args(["doctor", "--skip-cluster", "--burn-in-format",
                                     "mxfp8"])) == 2
    assert cmd_doctor(ap.parse_args(["doctor", "--skip-cluster", "--burn-in-flip", "0:1"])) == 2
    for argv in (["--burn-in-format", "mxfp8"], ["--burn-in-flip", "0:1"],
                 ["--burn-in", "1", "--burn-in-format", "fp4"],
                 ["--burn-in", "1", "--burn-in-flip", "0:0"]):
        with pytest.raises(SystemExit) as e:
            validate.main(argv)
        assert e.value.code == 2


def _fake_burn_ins(monkeypatch, calls):
    def report(dev, seconds, n, flips, **more):
        bad = 16 * len(flips) if flips else 0
        return dict({"device": dev, "n": n, "seconds": seconds, "iterations": 16,
                     "tflops": 1000.0, "mismatches": bad, "ok": bad == 0}, **more)

    def fake_bf16(dev, seconds=10.0, n=8192, _flips=None):
        calls.append(("bf16", dev, seconds, _flips))
        return report(dev, seconds, n, _flips)

    def fake_mx(dev, seconds, fmt, n=8192, _flips=None):
        calls.append((fmt, dev, seconds, _flips))
        return report(dev, seconds, n, _flips, format=fmt)
    monkeypatch.setattr(probe, "burn_in", fake_bf16)
    monkeypatch.setattr(mxgemm, "burn_in", fake_mx)
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)


def test_probe_wiring(monkeypatch, capsys):
    from gpumounter_amd import cli

    class Verified:
        def to_dict(self):
            return {"device": 0}
    calls = []
    _fake_burn_ins(monkeypatch, calls)
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Verified()])
    ap = cli.build_parser()
    base = ["probe", "--bdf", "0000:05:00.0", "--burn-in", "2"]
    assert cli.cmd_probe(ap.parse_args(base)) == 0
    (r,) = json.loads(capsys.readouterr().out)
    assert sorted(r) == ["burn_in", "device"] and "format" not in r["burn_in"]
    assert calls == [("bf16", 0, 2.0, None)]               # the default: what it ran before
    del calls[:]
    assert cli.cmd_probe(ap.parse_args(base + ["--burn-in-format", "mxfp4,mxfp8"])) == 0
    (r,) = json.loads(capsys.readouterr().out)
    assert sorted(r) == ["burn_in_mxfp4", "burn_in_mxfp8", "device"]
    assert r["burn_in_mxfp8"]["format"] == "mxfp8" and r["burn_in_mxfp4"]["format"] == "mxfp4"
    assert calls == [("mxfp8", 0, 2.0, None), ("mxfp4", 0, 2.0, None)]
    del calls[:]
    assert cli.cmd_probe(ap.parse_args(base + ["--burn-in-format", "bf16,mxfp8,mxfp4",
                                               "--burn-in-flip", "0:0x1"])) == 1
    (r,) = json.loads(capsys.readouterr().out)
    assert [r[k]["ok"] for k in ("burn_in", "burn_in_mxfp8", "burn_in_mxfp4")] == [False] * 3
    assert calls == [(f, 0, 2.0, [(0, 1)]) for f in ("bf16", "mxfp8", "mxfp4")]


def test_doctor_wiring(monkeypatch):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["burn_in_formats"].default == ("bf16",)
    assert sig["burn_in_formats"].kind is sig["burn_in_formats"].KEYWORD_ONLY
    assert inspect.signature(doctor.run).parameters["burn_in_formats"].default is None
    calls = []
    _fake_burn_ins(monkeypatch, calls)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg, 2.0) if c.name == "gpu0"]
    assert plain.status == "ok" and "mxfp" not in plain.detail
    assert calls == [("bf16", 0, 2.0, None)]
    del calls[:]
    every = mxgemm.BURN_IN_FORMATS
    (ok,) = [c for c in doctor.check_gpus(cfg, 2.0, burn_in_formats=every) if c.name == "gpu0"]
    assert ok.status == "ok" and "burn-in mxfp8 2 s 1000 TF/s 0 mismatching words" in ok.detail
    assert "burn-in mxfp4 2 s" in ok.detail and "burn-in 2 s 1000 TF/s" in ok.detail
    (bad,) = [c for c in doctor.check_gpus(cfg, 2.0, burn_in_formats=("mxfp4",),
                                           burn_in_flip=[(9, 4)]) if c.name == "gpu0"]
    assert bad.status == "fail" and "failed: mxfp4 burn-in" in bad.detail
    assert " 16 mismatching words" in bad.detail
    assert calls == [(f, 0, 2.0, None) for f in every] + [("mxfp4", 0, 2.0, [(9, 4)])]
    (none,) = [c for c in doctor.check_gpus(cfg, burn_in_formats=every) if c.name == "gpu0"]
    assert "burn-in" not in none.detail                    # no seconds: no burn-in at all

    # doctor.run and the command line pass both on; exit 1 on a failed format
    from gpumounter_amd import cli

    seen = []
    for name in ("check_inventory", "check_cgroup", "check_devnodes", "check_pidns",
                 "check_systemd"):
        monkeypatch.setattr(doctor, name, lambda cfg: [])
    real = doctor.check_gpus

    def spy(cfg, burn_in_s=0.0, **kw):
        seen.append((burn_in_s, kw))
        return real(cfg, burn_in_s, **kw)
    monkeypatch.setattr(doctor, "check_gpus", spy)
    ap = cli.build_parser()
    argv = ["doctor", "--skip-cluster", "--burn-in", "2", "--burn-in-format", "mxfp8,mxfp4"]
    assert cli.cmd_doctor(ap.parse_args(argv)) == 0
    assert seen[-1] == (2.0, {"memtest_bytes": 0, "burn_in_formats": ("mxfp8", "mxfp4")})
    del calls[:]
    assert cli.cmd_doctor(ap.parse_args(argv + ["--burn-in-flip", "9:4"])) == 1
    assert seen[-1][1]["burn_in_flip"] == [(9, 4)]
    assert calls == [("mxfp8", 0, 2.0, [(9, 4)]), ("mxfp4", 0, 2.0, [(9, 4)])]


def test_validate_wiring(monkeypatch, capsys):
    from gpumounter_amd.parallel import validate

    calls = []
    _fake_burn_ins(monkeypatch, calls)
    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2 * numel}])
    assert validate.main(["--burn-in", "2"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert rep["ok"] and len(rep["burn_in"]) == 1 and "burn_in_mxfp8" not in rep
    assert calls == [("bf16", 0, 2.0, None)]
    del calls[:]
    assert validate.main(["--burn-in", "2", "--burn-in-format", "bf16,mxfp8,mxfp4"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert rep["ok"] and rep["burn_in_mxfp8"][0]["format"] == "mxfp8"
    assert rep["burn_in_mxfp4"][0]["ok"] and "format" not in rep["burn_in"][0]
    assert [c[0] for c in calls] == ["bf16", "mxfp8", "mxfp4"]
    del calls[:]
    assert validate.main(["--burn-in", "2", "--burn-in-format", "mxfp8,mxfp4", "--burn-in-flip",
                          "0:0x1", "--burn-in-flip", "9:0x8000"]) == 1
    rep = json.loads(capsys.readouterr().out)
    assert rep["ok"] is False and "burn_in" not in rep
    assert not rep["burn_in_mxfp8"][0]["ok"] and not rep["burn_in_mxfp4"][0]["ok"]
    assert calls == [(f, 0, 2.0, [(0, 1), (9, 0x8000)]) for f in ("mxfp8", "mxfp4")]
