"""The matrix-core format scan without a GPU: the host table against an independent numpy
reference with its own decoders, the code tables, the caps, the parsers, the refusals and the
command lines."""
import ctypes as C
import inspect

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import cuscan, mfmascan
from gpumounter_amd.ops.probe import ProbeError

SEEDS = (0, 0x0123456789ABCDEF)
ITERS = (1, 3, 63)
M32 = 0xFFFFFFFF
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])
# elements per lane, bits per element, (exponent bits, mantissa bits, bias) or None
GEOMETRY = {"f16": (8, 16, (5, 10, 15)), "fp8": (8, 8, (4, 3, 7)), "bf8": (8, 8, (5, 2, 15)),
            "i8": (16, 8, None), "f32": (1, 32, None), "f64": (1, 64, None),
            "mxfp8": (32, 8, (4, 3, 7)), "mxbf8": (32, 8, (5, 2, 15)), "mxfp6": (32, 6, (2, 3, 1)),
            "mxbf6": (32, 6, (3, 2, 3)), "mxfp4": (32, 4, (2, 1, 1))}


# ---------------------------------------------------------------- the independent reference
def H(seed, test, idx):
    """The CU scan's hash (gm_probe.h), vectorised over idx."""
    idx = np.asarray(idx, np.uint64)
    h = (np.uint64(seed & M32) ^ (idx * np.uint64(0x9E3779B1))) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h + np.uint64((seed >> 32) ^ ((test * 0xC2B2AE35) & M32))) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0x27D4EB2F)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h


def minifloat(code, ebits, mbits, bias):
    """sign | exponent | mantissa → float64; subnormal when the exponent field is 0."""
    code = np.asarray(code, np.int64)
    m = code & ((1 << mbits) - 1)
    e = (code >> mbits) & ((1 << ebits) - 1)
    s = np.where((code >> (ebits + mbits)) & 1, -1.0, 1.0)
    frac = m / float(1 << mbits)
    return s * np.where(e == 0, frac * 2.0 ** (1 - bias), (1 + frac) * 2.0 ** (e - bias))


def elements(fmt, img):
    """Register images uint32[..., 8] → element values float64[..., elems], by the packing the
    header comment states: element e is bits [width e, width (e + 1)) of the little-endian string
    of the lane's dwords."""
    elems, width, mini = GEOMETRY[fmt]
    bits = ((img[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(*img.shape[:-1], 256)
    if fmt == "f32":
        return img[..., :1].copy().view(np.float32).astype(np.float64)
    if fmt == "f64":
        return np.ascontiguousarray(img[..., :2]).view(np.float64)
    field = bits[..., :elems * width].reshape(*img.shape[:-1], elems, width).astype(np.int64)
    code = (field << np.arange(width)).sum(-1)
    if fmt == "i8":
        return np.where(code >= 128, code - 256, code).astype(np.float64)
    return minifloat(code, *mini)


def operand_hashes(fmt, seed, step):
    """h_q for every wave, operand, lane: uint64[4, 2, 64, 4]."""
    f = mfmascan.ALL_FORMATS.index(fmt)
    w, m, l, q = np.meshgrid(np.arange(4), np.arange(2), np.arange(64), np.arange(4),
                             indexing="ij")
    return H(seed, 0x200 + f, ((((4 * step + w) * 2 + m) * 64 + l) * 4 + q))


def matrices(fmt, seed, step):
    """A [4 waves, 16, K] and B [4, K, 16] of one step from the register images, with lane l
    holding row / column l & 15 and k = elems * (l >> 4) + e."""
    img, _ = mfmascan.images(fmt, seed, step)
    v = elements(fmt, img)                                     # [4, 2, 64, elems]
    elems = v.shape[-1]
    v = v.reshape(4, 2, 4, 16, elems)                          # [w, m, h, r, e]
    a = v[:, 0].transpose(0, 2, 1, 3).reshape(4, 16, 4 * elems)
    b = v[:, 1].transpose(0, 1, 3, 2).reshape(4, 4 * elems, 16)
    return a, b


def reference(fmt, seed, iters_list):
    """{iters: uint32[256, 4]} for a set of iteration counts (each a prefix of the longest)."""
    f = mfmascan.ALL_FORMATS.index(fmt)
    c = np.zeros((4, 16, 16))
    out = {}
    for s in range(max(iters_list)):
        a, b = matrices(fmt, seed, s)
        c = c + a @ b                                          # exact: all sums < 2^53
        if s + 1 in iters_list:
            v = c.copy()
            if fmt.startswith("mx"):
                r = np.arange(16)
                sa = 127 + (H(seed, 0x220 + f, (2 * np.arange(4)[:, None] + 0) * 16 + r)
                            .astype(np.int64) & 3) - 2
                sb = 127 + (H(seed, 0x220 + f, (2 * np.arange(4)[:, None] + 1) * 16 + r)
                            .astype(np.int64) & 3) - 2
                v = v * 2.0 ** (sa[:, :, None] + sb[:, None, :] - 254)
            v = v + 0.0                                        # a sum of zero is +0.0
            words = np.zeros((4, 64, 4), np.uint32)
            for l in range(64):
                for r in range(4):
                    row = (l >> 4) + 4 * r if fmt == "f64" else 4 * (l >> 4) + r
                    x = v[:, row, l & 15]
                    if fmt == "i8":
                        words[:, l, r] = x.astype(np.int64).astype(np.int32).view(np.uint32)
                    elif fmt == "f64":
                        u = x.astype(np.float64).view(np.uint64)
                        lo, hi = u & np.uint64(M32), u >> np.uint64(32)
                        rot = ((hi << np.uint64(16)) | (hi >> np.uint64(16))) & np.uint64(M32)
                        words[:, l, r] = (lo ^ rot).astype(np.uint32)
                    else:
                        x32 = x.astype(np.float32)
                        assert (x32.astype(np.float64) == x).all()
                        words[:, l, r] = x32.view(np.uint32)
            out[s + 1] = words.reshape(256, 4)
    return out


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fmt", mfmascan.ALL_FORMATS)
def test_expected_equals_the_numpy_reference(fmt, seed):
    ref = reference(fmt, seed, ITERS)
    for iters in ITERS:
        got = mfmascan.expected(fmt, seed, iters)
        assert got.shape == (256, 4) and got.dtype == np.uint32
        assert np.array_equal(got, ref[iters]), (fmt, seed, iters)


def test_expected_accepts_the_bit_as_well_as_the_name():
    for name, bit in mfmascan.FORMATS.items():
        assert np.array_equal(mfmascan.expected(bit, 5, 1), mfmascan.expected(name, 5, 1))
    assert list(mfmascan.FORMATS.values()) == [1 << i for i in range(11)]
    assert mfmascan.DEFAULT_ITERS == 16 and mfmascan.MAX_ITERS == 63


@pytest.mark.parametrize("fmt", [f for f in mfmascan.ALL_FORMATS if GEOMETRY[f][2]])
def test_code_tables_decode_to_the_e2m1_values(fmt):
    """Every element of an image, decoded by the format's definition, is the e2m1 value of the
    hash nibble it was made from; all 16 nibbles occur, -0 among them."""
    seed = SEEDS[1]
    img, _ = mfmascan.images(fmt, seed, 2)
    got = elements(fmt, img)                                   # [4, 2, 64, elems]
    h = operand_hashes(fmt, seed, 2)
    e = np.arange(GEOMETRY[fmt][0])
    nib = (h[..., e >> 3] >> (4 * (e & 7)).astype(np.uint64)).astype(np.int64) & 15
    want = E2M1[nib]
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))   # -0 is encoded as -0
    assert set(np.unique(nib)) == set(range(16))
    if fmt == "mxfp4":                                         # the image is the hash itself
        assert np.array_equal(img[..., :4], h.astype(np.uint32)) and not img[..., 4:].any()
    if fmt in ("mxfp6", "mxbf6"):
        assert not img[..., 6:].any()


def test_plain_operands_are_in_range():
    h = operand_hashes("i8", 7, 0)
    img, sc = mfmascan.images("i8", 7, 0)
    assert np.array_equal(img[..., :4], h.astype(np.uint32)) and (sc == 127).all()
    v = elements("i8", img)
    assert v.min() == -128 and v.max() == 127                  # full range
    v = elements("f32", mfmascan.images("f32", 7, 0)[0])
    assert np.array_equal(v[..., 0], (operand_hashes("f32", 7, 0)[..., 0] % 511).astype(float) - 255)
    v = elements("f64", mfmascan.images("f64", 7, 0)[0])
    assert np.array_equal(v[..., 0], (operand_hashes("f64", 7, 0)[..., 0]
                                      & ((1 << 23) - 1)).astype(float) - (1 << 22))
    _, sc = mfmascan.images("mxfp6", 7, 0)
    assert set(np.unique(sc)) == {125, 126, 127, 128}


def test_caps_hold_at_the_largest_iters():
    it = mfmascan.MAX_ITERS
    for fmt, k in mfmascan.K_PER_STEP.items():
        assert k == 4 * GEOMETRY[fmt][0]
        if GEOMETRY[fmt][2]:
            assert 144 * k * it < 2 ** 24                      # quarter units, exact in fp32
    assert 144 * 128 * 910 < 2 ** 24 <= 144 * 128 * 911
    assert 2 ** 14 * 64 * it < 2 ** 31
    assert 4 * 255 ** 2 * it < 2 ** 24 <= 4 * 255 ** 2 * (it + 2)   # f32 sets the common cap
    assert 4 * 2 ** 44 * it < 2 ** 53
    # and the tables at the cap stay inside them
    for fmt in ("f16", "mxfp4", "f32"):
        v = np.abs(mfmascan.expected(fmt, 3, it).view(np.float32))
        assert v.max() < 2.0 ** 24 and np.isfinite(v).all()
    assert np.abs(mfmascan.expected("i8", 3, it).view(np.int32).astype(np.int64)).max() < 2 ** 31


def test_tables_depend_on_format_seed_and_iters():
    base = {f: mfmascan.expected(f, 11, 3) for f in mfmascan.ALL_FORMATS}
    names = list(base)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(base[a], base[b]), (a, b)
        assert not np.array_equal(base[a], mfmascan.expected(a, 12, 3))
        assert not np.array_equal(base[a], mfmascan.expected(a, 11, 4))
    # the scales make the scaled forms' exponent fields vary more than the plain ones'
    assert len(np.unique(base["mxfp8"] >> 23)) > len(np.unique(base["fp8"] >> 23))


# ---------------------------------------------------------------- parsing and refusals
def test_parsers():
    assert mfmascan.parse_formats("fp8, mxfp4") == ("fp8", "mxfp4")
    assert mfmascan.parse_formats(",".join(mfmascan.ALL_FORMATS)) == mfmascan.ALL_FORMATS
    assert mfmascan.mask_of(mfmascan.ALL_FORMATS) == 2047 and mfmascan.mask_of("f64") == 32
    for bad in ("", "bf16", "fp8,,fp9", "mfma"):
        with pytest.raises(ProbeError):
            mfmascan.parse_formats(bad)
    assert mfmascan.parse_inject("any:mxfp4:0:0:1") == ("any", "mxfp4", 0, 0, 1)
    assert mfmascan.parse_inject("0x123:f64:130:2:0x10000") == (0x123, "f64", 130, 2, 0x10000)
    for bad in ("any:mxfp4:0:0", "any:mxfp4:0:0:0", "any:bf16:0:0:1", "any:fp8:256:0:1",
                "any:fp8:0:4:1", "4096:fp8:0:0:1", "x:fp8:0:0:1", "any:fp8:0:0:1:2"):
        with pytest.raises(ProbeError):
            mfmascan.parse_inject(bad)


def test_scan_validates_before_any_hip_call(monkeypatch):
    """Every refusal below is made in Python with the native library unreachable."""
    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    for kw in (dict(formats=()), dict(formats=("fp8", "bf16")), dict(formats=2048),
               dict(iters=0), dict(iters=64), dict(iters=1.5), dict(iters=True), dict(seed=-1),
               dict(seed=1 << 64), dict(min_rounds=0), dict(min_rounds=3, max_rounds=2),
               dict(max_rounds=1025), dict(_inject=("any", "fp8", 0, 0, 0)),
               dict(_inject=("any", "fp8", 256, 0, 1)), dict(_inject=("any", "fp8", 0, 4, 1)),
               dict(_inject=(4096, "fp8", 0, 0, 1)), dict(_inject=("any", "fp8", 0, 0)),
               dict(formats=("f16",), _inject=("any", "fp8", 0, 0, 1))):
        with pytest.raises(ProbeError):
            mfmascan.scan(0, **kw)
    with pytest.raises(ProbeError):
        mfmascan.scan(-1)
    for call in (lambda: mfmascan.expected("bf16", 0, 1), lambda: mfmascan.expected("fp8", 0, 0),
                 lambda: mfmascan.expected("fp8", 0, 64), lambda: mfmascan.signature("fp8", 0, 0),
                 lambda: mfmascan.signature(3, 0, 1), lambda: mfmascan.images("fp8", 0, 63)):
        with pytest.raises(ProbeError):
            call()
    with pytest.raises(AssertionError):                  # a good call does get there
        mfmascan.scan(0)


def test_native_entry_points_validate_before_selecting_a_device():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    res, n = _native.CuscanResult(), C.c_int(7)
    cus = (_native.CuscanCu * 4)()
    out = (C.c_uint32 * 1024)()
    P, W = C.c_void_p(4096), C.c_void_p(8192)   # never dereferenced: every call is refused first
    for fmt, iters in ((0, 1), (3, 1), (2048, 1), (1, 0), (1, 64), (1024, 64)):
        assert lib.gm_probe_mfmascan_expected(fmt, 0, iters, out) == 1
        assert lib.gm_probe_mfmascan_signature(fmt, 0, iters, P, W, None) == 1
    assert lib.gm_probe_mfmascan_expected(1, 0, 1, None) == 1
    for o, w in ((None, W), (P, None), (C.c_void_p(4096 + 4), W), (P, C.c_void_p(8194))):
        assert lib.gm_probe_mfmascan_signature(1, 0, 1, o, w, None) == 1
    img, sc = (C.c_uint32 * 4096)(), (C.c_uint32 * 128)()
    assert lib.gm_probe_mfmascan_images(64, 0, 0, img, sc) == 0
    for fmt, step, i, s in ((0, 0, img, sc), (3, 0, img, sc), (64, 63, img, sc),
                            (64, 0, None, sc), (64, 0, img, None)):
        assert lib.gm_probe_mfmascan_images(fmt, 0, step, i, s) == 1

    def scan(mask=2047, iters=1, lo=1, hi=1, inj=None, cap=4, table=cus):
        return lib.gm_probe_mfmascan(0, mask, iters, 0, lo, hi,
                                     C.byref(inj) if inj is not None else None, C.byref(res),
                                     table, cap, C.byref(n))
    assert scan(mask=0) == 1 and n.value == 0
    assert scan(mask=2048) == 1
    assert scan(iters=0) == 1 and scan(iters=64) == 1
    assert scan(lo=0) == 1 and scan(lo=2, hi=1) == 1 and scan(hi=1025) == 1
    assert scan(cap=-1) == 1 and scan(cap=4, table=None) == 1
    inject = _native.CuscanInject
    for inj in (inject(0, 1024, 0, 0, 0), inject(0, 6, 0, 0, 1), inject(0, 1024, 256, 0, 1),
                inject(0, 1024, 0, 4, 1), inject(4096, 1024, 0, 0, 1), inject(0, 2048, 0, 0, 1)):
        assert scan(inj=inj) == 1
    assert scan(mask=1, inj=inject(0, 1024, 0, 0, 1)) == 1       # a format that is not selected
    assert lib.gm_probe_mfmascan(0, 2047, 1, 0, 1, 1, None, None, cus, 4, C.byref(n)) == 1


# ---------------------------------------------------------------- command lines
def test_command_lines_parse_the_mfma_scan_options():
    from gpumounter_amd.cli import build_parser, cmd_probe

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.mfma_scan is False and a.mfma_scan_inject is None and a.mfma_scan_formats is None
    assert a.mfma_scan_iters is None and a.mfma_scan_rounds is None
    a = ap.parse_args(["probe", "--mfma-scan", "--mfma-scan-formats", "fp8,mxfp4",
                       "--mfma-scan-iters", "3", "--mfma-scan-rounds", "2", "--mfma-scan-inject",
                       "any:mxfp4:0:0:1"])
    assert a.mfma_scan and tuple(a.mfma_scan_formats) == ("fp8", "mxfp4")
    assert a.mfma_scan_iters == 3 and a.mfma_scan_rounds == 2
    assert a.mfma_scan_inject == ("any", "mxfp4", 0, 0, 1)
    for bad in (["--mfma-scan-formats", "fp8,bf16"], ["--mfma-scan-inject", "any:mxfp4:0:0"],
                ["--mfma-scan-inject", "any:mxfp4:0:0:0"], ["--mfma-scan-iters", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--mfma-scan", *bad])
    # usage errors (2), not a failed scan (1), before any GPU work
    assert cmd_probe(ap.parse_args(["probe", "--mfma-scan-inject", "any:mxfp4:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--mfma-scan-iters", "3"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--mfma-scan", "--mfma-scan-formats", "fp8",
                                    "--mfma-scan-inject", "any:mxfp4:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--mfma-scan", "--mfma-scan-iters", "64"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--mfma-scan", "--mfma-scan-rounds", "0"])) == 2
    d = ap.parse_args(["doctor", "--gpu", "--mfma-scan", "--mfma-scan-inject", "any:f64:1:2:4"])
    assert d.mfma_scan is True and d.mfma_scan_inject == ("any", "f64", 1, 2, 4)
    assert ap.parse_args(["doctor", "--gpu"]).mfma_scan is False


def test_probe_passes_the_options_on(monkeypatch, capsys):
    from gpumounter_amd.cli import build_parser, cmd_probe
    from gpumounter_amd.ops import probe

    class Res:
        def to_dict(self):
            return {"device": 0}
    calls = []

    def fake_scan(dev, **kw):
        calls.append((dev, kw))
        return {"ok": kw["_inject"] is None}
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Res()])
    monkeypatch.setattr(mfmascan, "scan", fake_scan)
    ap = build_parser()
    assert cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--mfma-scan"])) == 0
    assert calls[-1] == (0, dict(formats=mfmascan.ALL_FORMATS, iters=16, min_rounds=1,
                                 max_rounds=16, _inject=None))
    assert cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--mfma-scan",
                                    "--mfma-scan-formats", "mxfp4", "--mfma-scan-iters", "63",
                                    "--mfma-scan-rounds", "20", "--mfma-scan-inject",
                                    "any:mxfp4:0:0:1"])) == 1
    assert calls[-1] == (0, dict(formats=("mxfp4",), iters=63, min_rounds=20, max_rounds=20,
                                 _inject=("any", "mxfp4", 0, 0, 1)))
    assert '"mfmascan"' in capsys.readouterr().out


def test_validate_parses_the_mfma_scan_options():
    from gpumounter_amd.parallel import validate

    with pytest.raises(SystemExit):
        validate.main(["--mfma-scan-inject", "any:mxfp4:0:0:1"])       # needs --mfma-scan
    with pytest.raises(SystemExit):
        validate.main(["--mfma-scan", "--mfma-scan-inject", "any:bf16:0:0:1"])


def test_doctor_passes_the_scan_on_and_names_the_unit_and_format(monkeypatch):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["mfma_scan"].default is False and sig["mfma_scan"].kind is sig["mfma_scan"].KEYWORD_ONLY
    assert sig["mfma_scan_inject"].default is None
    assert inspect.signature(doctor.run).parameters["mfma_scan"].default is False

    calls = []

    def fake_scan(dev, _inject=None):
        calls.append((dev, _inject))
        bad = _inject is not None
        failed = [{"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "runs": 1, "failed_runs": 1,
                   "formats_failed": ["mxfp4"], "simds_failed": [2]}] if bad else []
        return {"formats": list(mfmascan.ALL_FORMATS), "cus_seen": 250, "cus_expected": 256,
                "complete": False, "rounds": 16, "kernel_ms": 1.0, "words_in_error": int(bad),
                "ok": not bad, "failed": failed}
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(mfmascan, "scan", fake_scan)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "mfma-scan" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, mfma_scan=True) if c.name == "gpu0"]
    assert ok.status == "ok" and "mfma-scan 11 formats 250/256 CUs" in ok.detail
    assert "incomplete" in ok.detail
    inj = (0x123, "mxfp4", 130, 2, 0x10000)
    (bad,) = [c for c in doctor.check_gpus(cfg, mfma_scan=True, mfma_scan_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail" and "xcc 1 se 1 sh 0 cu 3 (id 0x123) simd 2 mxfp4" in bad.detail
    assert calls == [(0, None), (0, inj)]


def test_the_result_decoder_is_shared_with_the_cu_scan():
    unit = {"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "simds_failed": [1, 3],
            "formats_failed": ["fp8", "mxfp6"]}
    assert mfmascan.describe_failed({"failed": [unit]}) == (
        "xcc 2 se 1 sh 0 cu 5 (id 0x225) simd 1,3 fp8+mxfp6")
    assert cuscan.describe_failed({"failed": [unit]}, "formats") == (
        mfmascan.describe_failed({"failed": [unit]}))
