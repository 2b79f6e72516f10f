"""The attributed burn-in without a GPU: the rotated block → tile map as the host evaluates it
(the function the traced kernels evaluate on the device), the rotation's step, the blame rule on
synthetic logs, every refusal before the native call, and the options' way down to
``probe.burn_in`` / ``mxgemm.burn_in`` with exactly the keywords that were asked for."""
import inspect
import json
from math import gcd

import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import mxgemm, probe
from gpumounter_amd.ops.probe import ProbeError

SIZES = ((256, 1), (768, 9), (1536, 36), (2048, 64), (8192, 1024))


def plain_map(block, grid, n):
    """The map the burn-in GEMMs have always used, written out again: block ids dealt over 8
    XCDs, each XCD a contiguous range of tiles, tile rows grouped 8 deep."""
    q, rem, xcd = grid // 8, grid % 8, block % 8
    wgid = block // 8 + sum(q + 1 if x < rem else q for x in range(xcd))
    nt = n // 256
    group, within = divmod(wgid, 8 * nt)
    rows = min(nt - group * 8, 8)
    return (group * 8 + within % rows) * nt + within // rows


@pytest.mark.parametrize("n,tiles", SIZES)
def test_the_rotated_map_is_a_bijection_and_r0_is_todays_map(n, tiles):
    for r in sorted({0, 1, 7, 8, tiles - 1}):
        if r >= tiles:
            with pytest.raises(ProbeError):
                probe.burn_in_tile_map(n, r)
            continue
        got, step = probe.burn_in_tile_map(n, r)
        assert sorted(got) == list(range(tiles)), (n, r)
        assert got == [plain_map((b + r) % tiles, tiles, n) for b in range(tiles)], (n, r)
    assert gcd(step, tiles) == 1 and (tiles <= 8 or step % 8 != 0), (n, step)
    assert len({i * step % tiles for i in range(1, tiles + 1)}) == tiles


def test_the_map_moves_every_tile_to_another_xcd_when_r_is_no_multiple_of_8():
    at0, _ = probe.burn_in_tile_map(2048, 0)
    block_of = {t: b for b, t in enumerate(at0)}
    for r in (1, 7, 63):
        at, _ = probe.burn_in_tile_map(2048, r)
        assert all(b % 8 != block_of[t] % 8 for b, t in enumerate(at)), r
    at8, _ = probe.burn_in_tile_map(2048, 8)
    assert all(b % 8 == block_of[t] % 8 for b, t in enumerate(at8))


def test_tile_map_refusals():
    lib = _native.probe()
    out = [_native.C.byref(_native.C.c_int(0)) for _ in range(3)]
    for m, n, b, r in ((300, 256, 0, 0), (256, 0, 0, 0), (512, 512, 4, 0), (512, 512, 0, 4),
                       (512, 512, -1, 0), (512, 512, 0, -1)):
        assert lib.gm_probe_burn_in_tile_map(m, n, b, r, *out) == 1
    for bad in (0, 100, "768", True):
        with pytest.raises(ProbeError):
            probe.burn_in_tile_map(bad)


# ---------------------------------------------------------------------------- the blame rule
def ids(r):
    return [b["id"] for b in r["blamed"]]


def test_a_transient_worker_fault_on_an_exonerated_tile_blames_the_worker():
    r = probe.burn_in_blame([(5, 3, 0x123, 0x045, 2)], [1] * 64)
    (b,) = r["blamed"]
    assert b == {"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "events": 1, "words": 2,
                 "as_worker": 1, "as_reference": 0}
    assert r["events"] == r["logged"] == 1 and not r["log_overflow"]
    assert r["tiles_exonerated"] == 64
    assert r["first_events"] == [{"iteration": 5, "tile": 3, "worker": 0x123,
                                  "reference": 0x045, "words": 2}]
    json.dumps(r)


def test_a_reference_tile_that_never_matches_blames_the_reference():
    ex = [1] * 64
    ex[7] = 0
    r = probe.burn_in_blame([(i, 7, 0x200 + i, 0x045, 1) for i in range(1, 41)], ex)
    (b,) = r["blamed"]
    assert b["id"] == 0x045 and b["as_reference"] == 40 and b["as_worker"] == 0
    assert b["events"] == 40 and b["words"] == 40 and r["tiles_exonerated"] == 63


def test_a_consistently_wrong_cu_is_the_only_one_blamed():
    x, ex, events = 0x311, [1] * 64, []
    ex[9] = 0                     # X computed the reference there: nobody reproduces it
    for i in range(1, 21):
        if i % 5:                 # X itself computes tile 9 now and then, and matches
            events.append((i, 9, 0x400 + i, x, 1))
        events.append((i, 20 + i % 8, x, 0x500 + i, 1))
    r = probe.burn_in_blame(events, ex)
    (b,) = r["blamed"]
    assert b["id"] == x and b["as_reference"] == 16 and b["as_worker"] == 20
    assert b["events"] == 36


def test_a_unit_disagreeing_with_itself_is_blamed_as_the_worker():
    for exonerated in (0, 1):
        r = probe.burn_in_blame([(1, 0, 0x077, 0x077, 3)], [exonerated] * 4)
        (b,) = r["blamed"]
        assert b["id"] == 0x077 and b["as_worker"] == 1 and b["as_reference"] == 0


def test_blamed_units_are_sorted_by_events_then_id():
    r = probe.burn_in_blame([(1, 0, 9, 1, 1), (1, 1, 4, 1, 1), (2, 2, 7, 1, 1), (2, 3, 7, 1, 1)],
                            [1] * 4)
    assert ids(r) == [7, 4, 9]


def test_overflow_is_reported_and_blames_only_what_was_logged():
    cap = _native.BURNIN_LOG_CAP
    log = [(1, 2, 0x123, 0x045, 1)] * cap
    r = probe.burn_in_blame(log, [1] * 64, counted=5000)
    assert r["log_overflow"] is True and r["events"] == 5000 and r["logged"] == cap
    assert ids(r) == [0x123] and r["blamed"][0]["events"] == cap
    # what lies past the capacity was counted, not logged: it is never read
    r = probe.burn_in_blame(log + [(9, 2, 0x999, 0x888, 1)], [1] * 64)
    assert r["log_overflow"] is True and r["events"] == cap + 1 and ids(r) == [0x123]
    r = probe.burn_in_blame(log, [1] * 64)
    assert r["log_overflow"] is False and r["events"] == r["logged"] == cap


def test_blame_refusals(monkeypatch):
    monkeypatch.setattr(_native, "probe", lambda: pytest.fail("the native library was reached"))
    for events, ex, kw in (([(1, 0, 1, 2, 1)], [], {}),             # no tiles
                           ([(1, 4, 1, 2, 1)], [1] * 4, {}),        # a tile outside
                           ([(1, 0, 4096, 2, 1)], [1] * 4, {}),     # ids outside
                           ([(1, 0, 1, 4096, 1)], [1] * 4, {}),
                           ([(1, 0, 1, 2)], [1] * 4, {}),           # not five
                           ([(1, 0, -1, 2, 1)], [1] * 4, {}),
                           ([(1, 0, 1, 2, 1)], [1] * 4, {"counted": 0}),
                           ([(1, 0, 1, 2, 1)], [1] * 4, {"counted": 3})):
        with pytest.raises(ProbeError):
            probe.burn_in_blame(events, ex, **kw)


def test_native_blame_refuses_what_it_cannot_index():
    lib, C = _native.probe(), _native.C
    attr, blamed = _native.BurninAttr(), (_native.BurninBlamed * 4)()
    ex = (C.c_uint8 * 4)(1, 1, 1, 1)
    for bad in ((1, 4, 1, 2, 1), (1, 0, 4096, 2, 1), (1, 0, 1, 4096, 1)):
        ev = (_native.BurninEvent * 1)(_native.BurninEvent(*bad))
        assert lib.gm_probe_burn_in_blame(ev, 1, ex, 4, C.byref(attr), blamed, 4) == 1
    ev = (_native.BurninEvent * 1)(_native.BurninEvent(1, 0, 1, 2, 1))
    assert lib.gm_probe_burn_in_blame(ev, 1, ex, 0, C.byref(attr), blamed, 4) == 1
    assert lib.gm_probe_burn_in_blame(ev, -1, ex, 4, C.byref(attr), blamed, 4) == 1
    assert lib.gm_probe_burn_in_blame(None, 1, ex, 4, C.byref(attr), blamed, 4) == 1
    assert lib.gm_probe_burn_in_blame(ev, 1, ex, 4, C.byref(attr), None, 4) == 1
    assert lib.gm_probe_burn_in_blame(ev, 1, ex, 4, None, blamed, 4) == 1
    assert lib.gm_probe_burn_in_blame(ev, 1, ex, 4, C.byref(attr), blamed, 4) == 0
    assert attr.n_blamed == 1 and blamed[0].id == 1


# ---------------------------------------------------------------------------- refusals
def test_parse_burn_in_inject():
    assert probe.parse_burn_in_inject("first:0x1") == ("first", 1)
    assert probe.parse_burn_in_inject(" FIRST : 65535 ") == ("first", 0xFFFF)
    assert probe.parse_burn_in_inject("0x123:0x8000") == (0x123, 0x8000)
    assert probe.parse_burn_in_inject("4095:1") == (4095, 1)
    for bad in ("", "first", "first:0", "first:0x10000", "4096:1", "-1:1", "any:1", "1:2:3",
                "x:1", "1:y"):
        with pytest.raises(ProbeError):
            probe.parse_burn_in_inject(bad)


def test_every_refusal_is_raised_before_the_native_call(monkeypatch):
    monkeypatch.setattr(_native, "probe", lambda: pytest.fail("the native library was reached"))
    bad = ((4096, 1), (-1, 1), (True, 1), ("last", 1), (1.0, 1), (1, 0), (1, 0x10000),
           (1, -1), (1, True), ("first", 0), ("first",), 7, (1, 2, 3))
    for inj in bad:
        with pytest.raises(ProbeError):
            probe.burn_in(0, 1.0, 256, attribute=True, _inject=inj)
        for fmt in mxgemm.FORMATS:
            with pytest.raises(ProbeError):
                mxgemm.burn_in(0, 1.0, fmt, n=256, attribute=True, _inject=inj)
    for inj in ((1, 1), ("first", 1)):      # an injection without the attribution
        with pytest.raises(ProbeError, match="attribute"):
            probe.burn_in(0, 1.0, 256, _inject=inj)
        with pytest.raises(ProbeError, match="attribute"):
            mxgemm.burn_in(0, 1.0, "mxfp8", n=256, _inject=inj)
    with pytest.raises(ProbeError):         # the flips are still checked in this mode
        probe.burn_in(0, 1.0, 256, _flips=[(256 * 256, 1)], attribute=True)
    with pytest.raises(ProbeError):
        mxgemm.burn_in(0, 1.0, "mxfp4", n=128, attribute=True)


def test_native_entries_refuse_before_selecting_a_device():
    lib, C = _native.probe(), _native.C
    out = [C.byref(C.c_double(0)), C.byref(C.c_uint64(0)), C.byref(C.c_int(0))]
    attr, blamed = _native.BurninAttr(), (_native.BurninBlamed * 4)()
    tail = [C.byref(attr), blamed, 4]
    ok = _native.BurninInject(1, 1, 0)
    for inj in (_native.BurninInject(4096, 1, 0), _native.BurninInject(1, 0, 0),
                _native.BurninInject(1, 0x10000, 0), _native.BurninInject(0, 0, 1)):
        assert lib.gm_probe_burn_in_attr(0, 256, 1.0, 0, None, None, C.byref(inj), *out,
                                         *tail) == 1
        assert lib.gm_probe_mx_burn_in_attr(0, 0, 256, 1.0, 0, None, None, C.byref(inj), *out,
                                            *tail) == 1
    assert lib.gm_probe_burn_in_attr(0, 300, 1.0, 0, None, None, C.byref(ok), *out, *tail) == 1
    assert lib.gm_probe_burn_in_attr(0, 256, 0.0, 0, None, None, None, *out, *tail) == 1
    assert lib.gm_probe_burn_in_attr(0, 256, 1.0, 1, None, None, None, *out, *tail) == 1
    assert lib.gm_probe_burn_in_attr(0, 256, 1.0, 0, None, None, None, *out, None, blamed,
                                     4) == 1
    assert lib.gm_probe_burn_in_attr(0, 256, 1.0, 0, None, None, None, *out, C.byref(attr), None,
                                     4) == 1
    assert lib.gm_probe_mx_burn_in_attr(0, 1, 256, 1.0, 0, None, None, None, *out, *tail) == 1
    assert lib.gm_probe_mx_burn_in_attr(0, 4, 128, 1.0, 0, None, None, None, *out, *tail) == 1
    regs = [C.byref(C.c_int(0))] * 2
    assert lib.gm_probe_mxgemm_nt_traced_info(1, *regs) == 1
    assert lib.gm_probe_gemm_nt_traced(None, None, None, 256, 256, 64, 0, None, None, None) == 1
    assert lib.gm_probe_mxgemm_nt_traced(0, None, None, None, None, None, 256, 256, 128, 0, None,
                                         None, None) == 1


# ---------------------------------------------------------------------------- the wiring
def fake_burn_ins(monkeypatch, calls, blamed=()):
    def report(dev, seconds, fmt, kw):
        calls.append((fmt, dev, seconds, kw))
        bad = 16 if kw.get("_flips") or kw.get("_inject") else 0
        out = {"device": dev, "n": 8192, "seconds": seconds, "iterations": 16, "tflops": 1000.0,
               "mismatches": bad, "ok": bad == 0}
        if fmt != "bf16":
            out["format"] = fmt
        if kw.get("attribute"):
            out["attribution"] = {"tiles": 1024, "grid": 1024, "step": 343, "rotations": 16,
                                  "cus_seen": 256, "tiles_moved": 1000, "tiles_exonerated": 999,
                                  "events": bad, "logged": bad, "log_overflow": False,
                                  "first_id": 0x123, "blamed": list(blamed) if bad else []}
        return out

    monkeypatch.setattr(probe, "burn_in",
                        lambda dev, seconds=10.0, **kw: report(dev, seconds, "bf16", kw))
    monkeypatch.setattr(mxgemm, "burn_in",
                        lambda dev, seconds, fmt, **kw: report(dev, seconds, fmt, kw))
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)


UNIT = {"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "events": 16, "words": 16,
        "as_worker": 12, "as_reference": 4}


def test_signatures_default_to_the_plain_burn_in():
    from gpumounter_amd.utils import doctor

    for fn in (probe.burn_in, mxgemm.burn_in, mxgemm.run_burn_in):
        sig = inspect.signature(fn).parameters
        assert sig["attribute"].default is False and sig["_inject"].default is None
    for fn in (doctor.check_gpus, doctor.run):
        sig = inspect.signature(fn).parameters
        assert sig["burn_in_attribute"].default is False
        assert sig["burn_in_attribute"].kind is sig["burn_in_attribute"].KEYWORD_ONLY
        assert sig["burn_in_inject"].default is None
    assert mxgemm.attribute_kwargs(False, None) == {}
    assert mxgemm.attribute_kwargs(True, None) == {"attribute": True}
    assert mxgemm.attribute_kwargs(True, ("first", 1)) == {"attribute": True,
                                                           "_inject": ("first", 1)}


def test_probe_passes_exactly_what_was_asked_for(monkeypatch, capsys):
    from gpumounter_amd import cli

    class Verified:
        def to_dict(self):
            return {"device": 0}
    calls = []
    fake_burn_ins(monkeypatch, calls, [UNIT])
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Verified()])
    ap = cli.build_parser()
    base = ["probe", "--bdf", "0000:05:00.0", "--burn-in", "2"]
    assert cli.cmd_probe(ap.parse_args(base)) == 0
    (r,) = json.loads(capsys.readouterr().out)
    assert calls == [("bf16", 0, 2.0, {})] and "attribution" not in r["burn_in"]
    del calls[:]
    argv = base + ["--burn-in-format", "bf16,mxfp4", "--burn-in-attribute"]
    assert cli.cmd_probe(ap.parse_args(argv)) == 0
    (r,) = json.loads(capsys.readouterr().out)
    assert calls == [(f, 0, 2.0, {"attribute": True}) for f in ("bf16", "mxfp4")]
    assert r["burn_in"]["attribution"]["blamed"] == []
    del calls[:]
    argv += ["--burn-in-inject", "first:0x1", "--burn-in-flip", "9:4"]
    assert cli.cmd_probe(ap.parse_args(argv)) == 1
    (r,) = json.loads(capsys.readouterr().out)
    want = {"_flips": [(9, 4)], "attribute": True, "_inject": ("first", 1)}
    assert calls == [(f, 0, 2.0, want) for f in ("bf16", "mxfp4")]
    assert r["burn_in_mxfp4"]["attribution"]["blamed"] == [UNIT]
    # usage errors: exit 2, nothing run
    del calls[:]
    for argv in (["probe", "--burn-in-attribute"],
                 ["probe", "--burn-in-inject", "first:1", "--burn-in-attribute"],
                 base + ["--burn-in-inject", "first:1"]):
        assert cli.cmd_probe(ap.parse_args(argv)) == 2
    assert "needs --burn-in-attribute" in capsys.readouterr().err and calls == []
    for bad in ("first:0", "4096:1", "first"):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + ["--burn-in-attribute", "--burn-in-inject", bad])
        assert e.value.code == 2
    capsys.readouterr()


def test_doctor_passes_the_options_on_and_names_the_blamed_units(monkeypatch, capsys):
    from gpumounter_amd import cli
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    calls = []
    fake_burn_ins(monkeypatch, calls, [UNIT, dict(UNIT, id=0x045, xcc=0, se=2, sh=0, cu=5,
                                                  as_worker=0, as_reference=3)])
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg, 2.0) if c.name == "gpu0"]
    assert calls == [("bf16", 0, 2.0, {})] and "tiles" not in plain.detail
    del calls[:]
    (ok,) = [c for c in doctor.check_gpus(cfg, 2.0, burn_in_attribute=True) if c.name == "gpu0"]
    assert calls == [("bf16", 0, 2.0, {"attribute": True})]
    assert ok.status == "ok" and "1024 tiles over 256 CUs, 1000 moved" in ok.detail
    assert "blames" not in ok.detail
    del calls[:]
    (bad,) = [c for c in doctor.check_gpus(cfg, 2.0, burn_in_formats=("mxfp4",),
                                           burn_in_attribute=True,
                                           burn_in_inject=("first", 1)) if c.name == "gpu0"]
    assert calls == [("mxfp4", 0, 2.0, {"attribute": True, "_inject": ("first", 1)})]
    assert bad.status == "fail" and "failed: mxfp4 burn-in" in bad.detail
    assert ("mxfp4 burn-in blames: xcc 1 se 1 sh 0 cu 3 (id 0x123) 12 as worker + 4 as "
            "reference; xcc 0 se 2 sh 0 cu 5 (id 0x045) 3 as reference") in bad.detail

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
    argv = ["doctor", "--skip-cluster", "--burn-in", "2"]
    assert cli.cmd_doctor(ap.parse_args(argv)) == 0
    assert seen[-1] == (2.0, {"memtest_bytes": 0})
    assert cli.cmd_doctor(ap.parse_args(argv + ["--burn-in-attribute"])) == 0
    assert seen[-1] == (2.0, {"memtest_bytes": 0, "burn_in_attribute": True})
    assert cli.cmd_doctor(ap.parse_args(argv + ["--burn-in-attribute", "--burn-in-inject",
                                                "0x123:0x1"])) == 1
    assert seen[-1] == (2.0, {"memtest_bytes": 0, "burn_in_attribute": True,
                              "burn_in_inject": (0x123, 1)})
    assert "bf16 burn-in blames: xcc 1 se 1 sh 0 cu 3 (id 0x123)" in capsys.readouterr().out
    n = len(seen)
    assert cli.cmd_doctor(ap.parse_args(argv + ["--burn-in-inject", "first:1"])) == 2
    assert cli.cmd_doctor(ap.parse_args(["doctor", "--skip-cluster",
                                         "--burn-in-attribute"])) == 2
    assert len(seen) == n


def test_validate_passes_the_options_on(monkeypatch, capsys):
    from gpumounter_amd.parallel import validate

    calls = []
    fake_burn_ins(monkeypatch, calls, [UNIT])
    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2 * numel}])
    assert validate.main(["--burn-in", "2"]) == 0
    capsys.readouterr()
    assert calls == [("bf16", 0, 2.0, {})]
    del calls[:]
    assert validate.main(["--burn-in", "2", "--burn-in-format", "mxfp8",
                          "--burn-in-attribute"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert calls == [("mxfp8", 0, 2.0, {"attribute": True})]
    assert rep["burn_in_mxfp8"][0]["attribution"]["tiles"] == 1024
    del calls[:]
    assert validate.main(["--burn-in", "2", "--burn-in-attribute", "--burn-in-inject",
                          "first:0x1"]) == 1
    rep = json.loads(capsys.readouterr().out)
    assert calls == [("bf16", 0, 2.0, {"attribute": True, "_inject": ("first", 1)})]
    assert rep["ok"] is False and rep["burn_in"][0]["attribution"]["blamed"] == [UNIT]
    for argv in (["--burn-in-attribute"], ["--burn-in", "1", "--burn-in-inject", "first:1"],
                 ["--burn-in", "1", "--burn-in-attribute", "--burn-in-inject", "first:0"]):
        with pytest.raises(SystemExit) as e:
            validate.main(argv)
        assert e.value.code == 2
    capsys.readouterr()
