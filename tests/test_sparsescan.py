"""The sparse and 32x32 matrix-core scan above its kernel (gpumounter_amd/ops/sparsescan.py): the
host tables against the numpy model of tests/sparse_operands.py, what the operand images cover,
the descriptor, the refusals, its place behind the pinned scans, the result decoder, and the
command lines of probe, doctor and validate. No GPU."""
import ctypes as C
import inspect
import json

import numpy as np
import pytest

import sparse_operands as so
from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe, sparsescan
from gpumounter_amd.ops.probe import ProbeError

SCAN = sparsescan.SCAN
GPU_TEST_SEED = 0x0123456789ABCDEF        # tests/test_sparsescan_gpu.py SEED


def test_descriptor_agrees_with_the_module_and_the_header():
    assert list(sparsescan.FORMATS.items()) == [
        ("f16", 1), ("bf16", 2), ("i8", 4), ("fp8", 8), ("bf8", 16), ("fp8bf8", 32),
        ("bf8fp8", 64), ("f16-32x32", 128), ("bf16-32x32", 256), ("i8-32x32", 512),
        ("fp8-32x32", 1024)]
    assert (SCAN.label, SCAN.key, SCAN.stem, SCAN.selection) == (
        "sparse-scan", "sparsescan", "sparse_scan", "formats")
    assert SCAN.module is sparsescan and SCAN.bits is sparsescan.FORMATS
    assert SCAN.all == sparsescan.ALL_FORMATS == tuple(so.FORMS)
    assert (SCAN.default_iters, SCAN.max_iters) == (16, 63) == (sparsescan.DEFAULT_ITERS,
                                                                sparsescan.MAX_ITERS)
    assert tuple(SCAN.controls) == ("inject",) and not SCAN.plain_cli
    assert sparsescan.K_PER_STEP == {f: so.geometry(f)[4] for f in so.FORMS}
    assert sparsescan.parse_formats("bf16, i8-32x32") == ("bf16", "i8-32x32")
    # the bit table is the header's GM_SPARSESCAN_ALL: every bit accepted, the next one refused
    expected = _native.probe().gm_probe_sparsescan_expected
    out = (C.c_uint32 * 1024)()
    for bit in sparsescan.FORMATS.values():
        assert expected(bit, 0, 1, out) == 0
    assert expected(2048, 0, 1, out) == 1 and expected(3, 0, 1, out) == 1
    assert expected(1, 0, 0, out) == 1 and expected(1, 0, 64, out) == 1
    assert expected(1, 0, 63, out) == 0 and expected(1, 0, 1, None) == 1


@pytest.mark.parametrize("fmt", sparsescan.ALL_FORMATS)
def test_expected_equals_the_numpy_model_over_the_images(fmt):
    """Bit for bit at iters 1, 3 and 63: the model multiplies what images() returns, so a packing
    or index-word error on either side shows."""
    total = None
    for step in range(sparsescan.MAX_ITERS):
        a, b, idx, abid = sparsescan.images(fmt, GPU_TEST_SEED, step)
        assert (a.shape, b.shape, idx.shape) == ((4, 64, 4), (4, 64, 8), (4, 64))
        assert abid == (step % 2 if so.sets(fmt) == 2 else 0)
        c, unit = so.product(fmt, a, b, idx, abid)
        total = c if total is None else total + c
        if step + 1 in (1, 3, sparsescan.MAX_ITERS):
            want = so.signature(fmt, so.accumulators(fmt, total, unit))
            got = sparsescan.expected(fmt, GPU_TEST_SEED, step + 1)
            assert got.shape == (256, 4) and got.dtype == np.uint32
            np.testing.assert_array_equal(got, want, err_msg=f"{fmt} iters {step + 1}")
    # exactness at the cap: every sum is an integer below 2^24 quarter units (int32 for i8)
    assert np.abs(total).max() < (1 << 31 if "i8" in fmt else 1 << 24)


@pytest.mark.parametrize("seed", (cuframe.DEFAULT_SEED, GPU_TEST_SEED))
@pytest.mark.parametrize("fmt", sparsescan.ALL_FORMATS)
def test_the_images_cover_what_the_scan_claims(fmt, seed):
    _, bits, kind_a, kind_b = so.FORMS[fmt]
    groups = so.geometry(fmt)[2]
    legal = {i0 | i1 << 2 for i0, i1 in so.PAIRS}
    abids = []
    for step in (0, 1):
        a, b, idx, abid = sparsescan.images(fmt, seed, step)
        abids.append(abid)
        nibbles = (idx[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & 15     # [4, 64, 8]
        assert set(nibbles.reshape(-1).tolist()) == legal        # ascending pairs only
        for j in range(8):      # all six pairs in every group position (of both sets)
            assert set(nibbles[:, :, j].reshape(-1).tolist()) == legal, (step, j)
        pos = so.positions(fmt, idx, abid)
        assert pos.shape == (4, 64, groups, 2) and (pos[..., 0] < pos[..., 1]).all()
        for kind, img in ((kind_a, a), (kind_b, b)):
            codes = so.elements(img, bits)
            if kind == "i8":
                assert len(set(codes.reshape(-1).tolist())) > 200        # raw hash bytes
                continue
            values = so.decode(kind, codes)
            seen = {(abs(v), bool(np.signbit(v))) for v in values.reshape(-1).tolist()}
            assert seen == {(m, s) for m in so.NIBBLE_VALUES for s in (False, True)}, kind
        assert sparsescan.expected(fmt, seed, step + 1).any()
    assert abids == ([0, 1] if so.sets(fmt) == 2 else [0, 0])
    # the two sets of a 16-bit form are filled independently
    if so.sets(fmt) == 2:
        idx = sparsescan.images(fmt, seed, 0)[2]
        assert ((idx & 0xFFFF) != (idx >> 16)).mean() > 0.9


def test_images_and_expected_are_functions_of_their_arguments():
    for fmt in ("bf16", "fp8bf8", "i8-32x32"):
        a, b, idx, _ = sparsescan.images(fmt)
        a2, b2, idx2, _ = sparsescan.images(fmt)
        assert (a == a2).all() and (b == b2).all() and (idx == idx2).all()
        a3, b3, idx3, _ = sparsescan.images(fmt, seed=1)
        assert (a != a3).any() and (b != b3).any() and (idx != idx3).any()
        a4, _, idx4, _ = sparsescan.images(fmt, step=1)
        assert (a != a4).any() and (idx != idx4).any()
        table = sparsescan.expected(fmt, iters=1)
        assert (sparsescan.expected(fmt, iters=1) == table).all()
        assert (sparsescan.expected(fmt, seed=1, iters=1) != table).any()
        assert (sparsescan.expected(fmt, iters=2) != table).any()
    # the mixed forms differ from the plain ones in one operand's codes
    assert (sparsescan.expected("fp8bf8", iters=1) != sparsescan.expected("bf8fp8", iters=1)).any()


def test_the_helpers_constructed_cases_are_what_they_say():
    for fmt in so.FORMS:
        size, slices, groups, dense, k_total = so.geometry(fmt)
        assert k_total == sparsescan.K_PER_STEP[fmt] and so.b_modulus(fmt) <= k_total
        slots = {so.one_hot_slot(fmt, row) for row in range(size)}
        assert len(slots) == min(size, slices * groups * 2)
        assert all(so.one_hot_slot(fmt, r) != so.one_hot_slot(fmt, r + 1) for r in range(size - 1))
        for pair in range(6):
            for abid in range(so.sets(fmt)):
                a, b, idx, selected = so.one_hot_case(fmt, pair, abid)
                c, unit = so.product(fmt, a, b, idx, abid)
                assert (c == ((selected % so.b_modulus(fmt)) + 1)[None, :, None] * unit).all()
                if so.sets(fmt) == 2:       # the other set would select other elements
                    other, _ = so.product(fmt, a, b, idx, 1 - abid)
                    assert (other != c).any()
        a, b, idx = so.random_case(fmt, 3)
        assert (a.shape, b.shape, idx.shape) == ((4, 64, 4), (4, 64, 8), (4, 64))
        assert a.dtype == b.dtype == idx.dtype == np.uint32


def test_refusals_are_made_before_the_library_is_reached(monkeypatch):
    def reached():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", reached)
    with pytest.raises(ProbeError, match="^unknown sparse-scan format 'f32'"):
        sparsescan.expected("f32")
    with pytest.raises(ProbeError, match="^unknown sparse-scan format 'nope'"):
        sparsescan.scan(0, formats=("f16", "nope"))
    for bad in (0, 64, -1, 1.5, True):
        with pytest.raises(ProbeError, match="iters must be an integer in \\[1, 63\\]"):
            sparsescan.scan(0, iters=bad)
        with pytest.raises(ProbeError, match="iters"):
            sparsescan.expected("f16", iters=bad)
    with pytest.raises(ProbeError, match="step must be an integer in \\[0, 62\\]"):
        sparsescan.images("f16", step=63)
    with pytest.raises(ProbeError, match="injection into 'bf8', which is not run"):
        sparsescan.scan(0, formats=("f16", "i8"), _inject=("any", "bf8", 0, 0, 1))
    with pytest.raises(ProbeError, match="at least one format"):
        sparsescan.scan(0, formats=())
    with pytest.raises(ProbeError, match="max_rounds"):
        sparsescan.scan(0, min_rounds=4, max_rounds=2)
    with pytest.raises(ProbeError, match="abid must be an integer in \\[0, 1\\]"):
        sparsescan.apply("f16", 2, None, None, None)
    with pytest.raises(ProbeError, match="has one index set, abid must be 0"):
        sparsescan.apply("fp8-32x32", 1, None, None, None)
    a, b, idx = so.random_case("f16", 1)
    with pytest.raises(ProbeError, match=r"B must be uint32\[4, 64, 8\]"):
        sparsescan.apply("f16", 1, a, a, idx)
    with pytest.raises(ProbeError, match=r"the index words must be uint32\[4, 64\]"):
        sparsescan.apply("f16", 1, a, b, idx.astype(np.int32))


def test_the_frames_malformed_injections_are_refused():
    t = "i8-32x32"
    for bad in (f"any:{t}:0:0", "any:nope:0:0:1", f"any:{t}:256:0:1", f"any:{t}:0:4:1",
                f"any:{t}:0:0:0", f"4096:{t}:0:0:1", f"any:{t}:x:0:1", f"any:{t}:0:0:0x100000000",
                "", "any"):
        with pytest.raises(ProbeError, match="sparse-scan|CU id"):
            sparsescan.parse_inject(bad)
    assert sparsescan.parse_inject("any:i8-32x32:0:0:1") == ("any", "i8-32x32", 0, 0, 1)
    assert sparsescan.parse_inject("0x123:fp8bf8:130:2:0x10000") == (0x123, "fp8bf8", 130, 2,
                                                                   0x10000)


def test_the_native_entry_points_refuse_the_same():
    lib = _native.probe()
    res, n, cus = _native.CuscanResult(), C.c_int(7), (_native.CuscanCu * 4)()
    assert lib.gm_probe_sparsescan(0, 2048, 1, 0, 1, 1, None, C.byref(res), cus, 4,
                                   C.byref(n)) == 1 and n.value == 0
    assert lib.gm_probe_sparsescan(0, 1, 64, 0, 1, 1, None, C.byref(res), cus, 4, C.byref(n)) == 1
    inj = _native.CuscanInject(_native.CUSCAN_ANY, 2, 0, 0, 1)       # bf16 is not run
    assert lib.gm_probe_sparsescan(0, 1, 1, 0, 1, 1, C.byref(inj), C.byref(res), cus, 4,
                                   C.byref(n)) == 1
    u32 = (C.c_uint32 * 2048)()
    one = C.c_uint32(0)
    assert lib.gm_probe_sparsescan_images(1, 0, 63, u32, u32, u32, C.byref(one)) == 1
    assert lib.gm_probe_sparsescan_images(3, 0, 0, u32, u32, u32, C.byref(one)) == 1
    assert lib.gm_probe_sparsescan_images(1, 0, 0, u32, u32, u32, None) == 1
    # apply: a null or misaligned buffer, abid 2, abid 1 with an 8-bit form; no HIP call is made
    assert lib.gm_probe_sparsescan_apply(1, 0, None, None, None, None, None) == 1
    assert lib.gm_probe_sparsescan_apply(1, 2, 16, 16, 16, 16, None) == 1
    assert lib.gm_probe_sparsescan_apply(4, 1, 16, 16, 16, 16, None) == 1
    assert lib.gm_probe_sparsescan_apply(1, 0, 16, 24, 16, 16, None) == 1
    assert lib.gm_probe_sparsescan_apply(2048, 0, 16, 16, 16, 16, None) == 1


def test_all_scans_is_the_pinned_scans_followed_by_this_one():
    from gpumounter_amd import cli
    from gpumounter_amd.ops import ldsscan

    assert cuframe.LATER_MODULES == ("sparsescan",)
    assert cuframe.all_scans() == cuframe.scans() + (SCAN,)
    assert [s.key for s in cuframe.all_scans()] == ["cuscan", "mfmascan", "lanescan", "cachescan",
                                                    "ldsscan", "sparsescan"]
    # what the earlier tests pin stays as it was
    assert cuframe.MORE_MODULES == ("ldsscan",)
    assert cuframe.scans() == cuframe.registry() + (ldsscan.SCAN,)
    assert len(cuframe.registry()) == 4 and SCAN not in cuframe.scans()
    assert cli._scans() == cuframe.scans() and cli._all_scans() == cuframe.all_scans()


def test_scan_over_a_fake_native_entry_decodes_to_the_exact_dict(monkeypatch):
    a, b = "f16", "bf16"
    seen = []

    def entry(*args):
        seen.append(args[:6])
        def behind(kind):          # what a byref argument refers to
            return [x._obj for x in args if isinstance(getattr(x, "_obj", None), kind)]
        (res,), (n,) = behind(_native.CuscanResult), behind(C.c_int)
        assert args[6] is None and len(args) == 11      # no inject
        cus = next(x for x in args if isinstance(x, C.Array))
        res.cus_expected, res.cus_seen, res.complete, res.rounds = 256, 2, 0, 3
        res.blocks_run, res.words_in_error, res.blocks_four_simds, res.failed_cus = 768, 2, 700, 1
        res.xcc_cus[0] = res.xcc_cus[2] = 1
        res.seconds, res.kernel_ms = 0.5, 1.25
        res.records_filled = 1
        res.records[0] = _native.CuscanRecord(0x225, 2, 2, 130, 2, 0x10, 0x10010, 0)
        cus[0] = _native.CuscanCu(0x001, 0, 0, 0, 1, 3, 0, 0, 0b1111, 0)
        cus[1] = _native.CuscanCu(0x225, 2, 1, 0, 5, 3, 2, 3, 0b0111, 0b0100)
        n.value = 2
        return 0

    class Lib:
        gm_probe_sparsescan = staticmethod(entry)
    monkeypatch.setattr(_native, "probe", lambda: Lib())
    got = sparsescan.scan(0)
    assert seen == [(0, 2047, sparsescan.DEFAULT_ITERS, cuframe.DEFAULT_SEED, 1, 16)]
    good = {"id": 1, "xcc": 0, "se": 0, "sh": 0, "cu": 1, "runs": 3, "failed_runs": 0,
            "formats_failed": [], "simds_seen": [0, 1, 2, 3], "simds_failed": []}
    bad = {"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "runs": 3, "failed_runs": 2,
           "formats_failed": [a, b], "simds_seen": [0, 1, 2], "simds_failed": [2]}
    assert got == {
        "device": 0, "formats": list(sparsescan.ALL_FORMATS), "iters": sparsescan.DEFAULT_ITERS,
        "cus_expected": 256, "cus_seen": 2, "complete": False, "rounds": 3, "blocks_run": 768,
        "words_in_error": 2, "failed_cus": 1, "blocks_four_simds": 700,
        "xcc_cus": [1, 0, 1] + [0] * 13, "seconds": 0.5, "kernel_ms": 1.25,
        "first_errors": [{"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "simd": 2,
                          "format": b, "thread": 130, "word": 2, "expected": "0x00000010",
                          "got": "0x00010010", "xor": "0x00010000"}],
        "failed": [{k: v for k, v in bad.items() if k != "simds_seen"}],
        "per_cu": [good, bad], "ok": False}
    assert sparsescan.describe_failed(got) == "xcc 2 se 1 sh 0 cu 5 (id 0x225) simd 2 f16+bf16"


def test_command_lines_parse_the_sparse_scan_options():
    from gpumounter_amd.cli import build_parser, cmd_doctor, cmd_probe
    from gpumounter_amd.parallel import validate

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.sparse_scan is False and a.sparse_scan_inject is None
    assert a.sparse_scan_formats is None and a.sparse_scan_iters is None
    assert a.sparse_scan_rounds is None
    a = ap.parse_args(["probe", "--sparse-scan", "--sparse-scan-formats", "bf16,i8-32x32",
                       "--sparse-scan-iters", "3", "--sparse-scan-rounds", "2",
                       "--sparse-scan-inject", "any:i8-32x32:0:0:1"])
    assert a.sparse_scan and tuple(a.sparse_scan_formats) == ("bf16", "i8-32x32")
    assert a.sparse_scan_iters == 3 and a.sparse_scan_rounds == 2
    assert a.sparse_scan_inject == ("any", "i8-32x32", 0, 0, 1)
    for bad in (["--sparse-scan-formats", "bf16,nope"], ["--sparse-scan-inject", "any:bf16:0:0"],
                ["--sparse-scan-iters", "x"], ["--sparse-scan-inject", "any:f32:0:0:1"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--sparse-scan", *bad])
    # usage errors (2), not a failed scan (1), before any GPU work
    for opt in (["--sparse-scan-inject", "any:bf16:0:0:1"], ["--sparse-scan-iters", "3"],
                ["--sparse-scan-formats", "bf16"], ["--sparse-scan-rounds", "2"]):
        assert cmd_probe(ap.parse_args(["probe", *opt])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--sparse-scan", "--sparse-scan-formats", "f16",
                                    "--sparse-scan-inject", "any:bf16:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--sparse-scan", "--sparse-scan-iters", "64"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--sparse-scan", "--sparse-scan-iters", "0"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--sparse-scan", "--sparse-scan-rounds", "0"])) == 2
    d = ap.parse_args(["doctor", "--gpu", "--sparse-scan", "--sparse-scan-inject",
                       "any:fp8bf8:1:2:4"])
    assert d.sparse_scan is True and d.sparse_scan_inject == ("any", "fp8bf8", 1, 2, 4)
    assert ap.parse_args(["doctor", "--gpu"]).sparse_scan is False
    assert cmd_doctor(ap.parse_args(["doctor", "--sparse-scan-inject", "any:fp8bf8:1:2:4"])) == 2
    for bad in (["--sparse-scan-inject", "any:bf16:0:0:1"],
                ["--sparse-scan", "--sparse-scan-inject", "any:nope:0:0:1"]):
        with pytest.raises(SystemExit):
            validate.main(bad)


def _fake_gpu(monkeypatch):
    from gpumounter_amd.ops import probe
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)


def test_probe_runs_the_scan_after_the_lds_scan(monkeypatch, capsys):
    from gpumounter_amd.cli import build_parser, cmd_probe
    from gpumounter_amd.ops import ldsscan, probe

    order = []

    def fake(name):
        def scan(dev, **kw):
            order.append((name, dev, kw))
            return {"ok": True, "failed": []}
        return scan
    class Verified:
        def to_dict(self):
            return {"device": 0, "ok": True}
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Verified()])
    monkeypatch.setattr(ldsscan, "scan", fake("lds"))
    monkeypatch.setattr(sparsescan, "scan", fake("sparse"))
    code = cmd_probe(build_parser().parse_args(
        ["probe", "--bdf", "0000:05:00.0", "--sparse-scan", "--lds-scan", "--sparse-scan-formats", "bf8",
         "--sparse-scan-iters", "2", "--sparse-scan-rounds", "20"]))
    out = json.loads(capsys.readouterr().out)
    assert code == 0 and out[0]["sparsescan"] == {"ok": True, "failed": []}
    assert [o[0] for o in order] == ["lds", "sparse"]
    assert order[1][1:] == (0, {"formats": ("bf8",), "iters": 2, "min_rounds": 20,
                                "max_rounds": 20, "_inject": None})


def test_doctor_passes_the_scan_on_and_names_the_unit_and_format(monkeypatch):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    for fn in (doctor.check_gpus, doctor.run):
        sig = inspect.signature(fn).parameters
        assert sig["sparse_scan"].default is False
        assert sig["sparse_scan"].kind is sig["sparse_scan"].KEYWORD_ONLY
        assert sig["sparse_scan_inject"].default is None
        assert sig["sparse_scan_inject"].kind is sig["sparse_scan_inject"].KEYWORD_ONLY
    calls = []

    def fake_scan(dev, _inject=None):
        calls.append((dev, _inject))
        bad = _inject is not None
        failed = [{"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "runs": 1, "failed_runs": 1,
                   "formats_failed": ["bf16-32x32"], "simds_failed": [2]}] if bad else []
        return {"formats": list(sparsescan.ALL_FORMATS), "cus_seen": 250, "cus_expected": 256,
                "complete": False, "rounds": 16, "kernel_ms": 1.0, "words_in_error": int(bad),
                "ok": not bad, "failed": failed}
    _fake_gpu(monkeypatch)
    monkeypatch.setattr(sparsescan, "scan", fake_scan)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "sparse-scan" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, sparse_scan=True) if c.name == "gpu0"]
    assert ok.status == "ok" and "sparse-scan 11 formats 250/256 CUs" in ok.detail
    assert "incomplete" in ok.detail and " 0 wrong words" in ok.detail
    inj = (0x123, "bf16-32x32", 130, 2, 0x10000)
    (bad,) = [c for c in doctor.check_gpus(cfg, sparse_scan=True, sparse_scan_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail"
    assert bad.detail.endswith("xcc 1 se 1 sh 0 cu 3 (id 0x123) simd 2 bf16-32x32")
    assert calls == [(0, None), (0, inj)]


def test_doctor_run_forwards_only_what_is_set(monkeypatch):
    from gpumounter_amd.utils import doctor

    calls = []
    for name in ("check_inventory", "check_cgroup", "check_devnodes", "check_pidns",
                 "check_systemd"):
        monkeypatch.setattr(doctor, name, lambda cfg: [])
    monkeypatch.setattr(doctor, "check_gpus", lambda cfg, burn_in_s=0.0, **kw: calls.append(kw) or [])
    doctor.run(None, skip_cluster=True, gpu=True)
    doctor.run(None, skip_cluster=True, gpu=True, sparse_scan=True)
    doctor.run(None, skip_cluster=True, gpu=True, sparse_scan=True,
               sparse_scan_inject=("any", "i8", 0, 3, 1))
    doctor.run(None, skip_cluster=True, gpu=True, sparse_scan_inject=("any", "i8", 0, 3, 1))
    base = {"memtest_bytes": 0}
    assert calls == [base, dict(base, sparse_scan=True),
                     dict(base, sparse_scan=True, sparse_scan_inject=("any", "i8", 0, 3, 1)), base]


def test_validate_runs_the_scan_on_every_gpu(monkeypatch, capsys):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.parallel import validate

    calls = []

    def fake_scan(dev, **kw):
        calls.append((dev, kw))
        return {"ok": not any(v is not None for v in kw.values()), "failed": [],
                "per_cu": [{"id": 1}]}
    _fake_gpu(monkeypatch)
    monkeypatch.setattr(probe, "device_count", lambda: 2)
    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2 * numel}] * world)
    monkeypatch.setattr(sparsescan, "scan", fake_scan)

    def run(*opts):
        del calls[:]
        code = validate.main(["--no-p2p", "--sparse-scan", *opts])
        return code, json.loads(capsys.readouterr().out)

    code, report = run()
    assert code == 0 and report["ok"] is True
    assert report["sparsescan"] == [{"ok": True, "failed": []}] * 2          # per_cu is gone
    assert sorted(calls, key=lambda c: c[0]) == [(0, {"_inject": None}), (1, {"_inject": None})]
    assert not any(s.key in report for s in cuframe.scans())
    code, report = run("--sparse-scan-inject", "any:bf8:0:0:1")
    assert code == 1 and report["ok"] is False and report["sparsescan"][0]["ok"] is False
    assert "per_cu" not in report["sparsescan"][0]
    want = {"_inject": ("any", "bf8", 0, 0, 1)}
    assert sorted(calls, key=lambda c: c[0]) == [(0, want), (1, want)]
