"""The frame the per-CU scans share (gpumounter_amd/ops/cuframe.py): every descriptor against its
module and the C headers, the one result decoder behind every module's ``scan``, and validate's
run of every scan. No GPU."""
import ctypes as C
import importlib
import json

import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe
from gpumounter_amd.ops.probe import ProbeError

SCANS = cuframe.registry()
by_key = pytest.mark.parametrize("scan", SCANS, ids=[s.key for s in SCANS])


def test_the_registry_is_the_four_scans_in_report_order():
    assert [s.key for s in SCANS] == ["cuscan", "mfmascan", "lanescan", "cachescan"]
    assert [s.label for s in SCANS] == ["cu-scan", "mfma-scan", "lane-scan", "cache-scan"]
    assert [s.plain_cli for s in SCANS] == [True, False, False, False]
    assert [tuple(s.controls) for s in SCANS] == [("inject",)] * 3 + [("inject", "poke")]


@by_key
def test_descriptor_agrees_with_its_module_and_the_header(scan):
    from gpumounter_amd.cli import build_parser

    mod = importlib.import_module(f"gpumounter_amd.ops.{scan.key}")
    assert mod.SCAN is scan and scan.module is mod
    assert scan.symbol == f"gm_probe_{scan.key}"
    assert scan.selection in ("tests", "formats")
    assert scan.bits is getattr(mod, scan.selection.upper())
    assert scan.all == getattr(mod, f"ALL_{scan.selection.upper()}") == tuple(scan.bits)
    assert (scan.default_iters, scan.max_iters) == (mod.DEFAULT_ITERS, mod.MAX_ITERS)
    last = scan.all[-1]
    assert mod.bit_of(last) == scan.bits[last] == mod.bit_of(scan.bits[last])
    assert getattr(mod, f"parse_{scan.selection}")(",".join(scan.all)) == scan.all
    # the label is what the module's refusals carry, the stem what argparse calls the options
    with pytest.raises(ProbeError, match=f"^unknown {scan.label} {scan.unit} 'nope'"):
        mod.bit_of("nope")
    with pytest.raises(ProbeError, match=f"^{scan.label} needs at least one {scan.unit}"):
        mod.mask_of(())
    with pytest.raises(ProbeError, match=f"^{scan.label}: cannot read"):
        mod.parse_inject("x")
    args = build_parser().parse_args(["probe", f"--{scan.label}"])
    assert getattr(args, scan.stem) is True and scan.stem == scan.label.replace("-", "_")
    for name in scan.controls:
        assert getattr(args, f"{scan.stem}_{name}") is None
        assert callable(getattr(mod, f"parse_{name}"))
    # the same eight malformed injections are refused by every scan
    t = scan.all[0]
    for bad in (f"any:{t}:0:0", "any:nope:0:0:1", f"any:{t}:256:0:1", f"any:{t}:0:4:1",
                f"any:{t}:0:0:0", f"4096:{t}:0:0:1", f"any:{t}:x:0:1", f"any:{t}:0:0:0x100000000"):
        with pytest.raises(ProbeError, match=f"{scan.label}|CU id"):   # an id is the CU scan's
            mod.parse_inject(bad)
    assert mod.parse_inject(f"any:{t}:255:3:0xffffffff") == ("any", t, 255, 3, 0xFFFFFFFF)
    # the bit table is the header's GM_*_ALL: every bit accepted, the next one refused
    expected = getattr(_native.probe(), scan.symbol + "_expected")
    out = (C.c_uint32 * (cuframe.THREADS * cuframe.WORDS))()
    more = (None,) * len(scan.more_controls)            # no poke
    bits = sorted(scan.bits.values())
    assert bits == [1 << i for i in range(len(bits))]
    for bit in bits:
        assert expected(bit, 0, 1, *more, out) == 0
    assert expected(bits[-1] << 1, 0, 1, *more, out) == 1
    assert expected(bits[-1] | bits[0], 0, 1, *more, out) == 1


@by_key
def test_every_scan_result_is_built_by_the_one_decoder(scan, monkeypatch):
    """The module's ``scan`` over a fake native call that fills the C structures: the exact dict."""
    a, b = scan.all[:2]
    seen = []

    def entry(*args):
        seen.append(args[:6])
        def behind(kind):          # what a byref argument refers to
            return [x._obj for x in args if isinstance(getattr(x, "_obj", None), kind)]
        (res,), (n,) = behind(_native.CuscanResult), behind(C.c_int)
        cus = next(x for x in args if isinstance(x, C.Array))
        res.cus_expected, res.cus_seen, res.complete, res.rounds = 256, 2, 0, 3
        res.blocks_run, res.words_in_error, res.blocks_four_simds, res.failed_cus = 768, 2, 700, 1
        res.xcc_cus[0] = res.xcc_cus[2] = 1
        res.seconds, res.kernel_ms = 0.5, 1.25
        res.records_filled = 1
        res.records[0] = _native.CuscanRecord(0x225, 2, scan.bits[b], 130, 2, 0x10, 0x10010, 0)
        cus[0] = _native.CuscanCu(0x001, 0, 0, 0, 1, 3, 0, 0, 0b1111, 0)
        cus[1] = _native.CuscanCu(0x225, 2, 1, 0, 5, 3, 2, scan.bits[a] | scan.bits[b], 0b0111,
                                  0b0100)
        n.value = 2
        for timing in behind(_native.CachescanTiming):
            timing.blocks = 3
        return 0

    class Lib:
        pass
    lib = Lib()
    setattr(lib, scan.symbol, entry)
    monkeypatch.setattr(_native, "probe", lambda: lib)
    got = scan.module.scan(0)
    sel, unit = scan.selection, scan.unit
    mask = sum(scan.bits.values())
    assert seen == [(0, mask, scan.default_iters, cuframe.DEFAULT_SEED, 1, 16)]
    good = {"id": 1, "xcc": 0, "se": 0, "sh": 0, "cu": 1, "runs": 3, "failed_runs": 0,
            f"{sel}_failed": [], "simds_seen": [0, 1, 2, 3], "simds_failed": []}
    bad = {"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "runs": 3, "failed_runs": 2,
           f"{sel}_failed": [a, b], "simds_seen": [0, 1, 2], "simds_failed": [2]}
    want = {"device": 0, sel: list(scan.all), "iters": scan.default_iters, "cus_expected": 256,
            "cus_seen": 2, "complete": False, "rounds": 3, "blocks_run": 768, "words_in_error": 2,
            "failed_cus": 1, "blocks_four_simds": 700, "xcc_cus": [1, 0, 1] + [0] * 13,
            "seconds": 0.5, "kernel_ms": 1.25,
            "first_errors": [{"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "simd": 2, unit: b,
                              "thread": 130, "word": 2, "expected": "0x00000010",
                              "got": "0x00010010", "xor": "0x00010000"}],
            "failed": [{k: v for k, v in bad.items() if k != "simds_seen"}],
            "per_cu": [good, bad], "ok": False}
    if scan.key == "cachescan":
        zero = {"min": 0, "median": 0, "max": 0}
        want["timing"] = {"blocks": 3, **{t: {"first": zero, "last": zero} for t in scan.all}}
    assert got == want
    assert scan.module.describe_failed(got) == (
        f"xcc 2 se 1 sh 0 cu 5 (id 0x225) simd 2 {a}+{b}")


@by_key
def test_validate_runs_the_scan_on_every_gpu(scan, monkeypatch, capsys):
    """validate.main on the CPU: the report has the scan's key without ``per_cu``, the parsed
    negative controls reach ``scan`` and the exit code follows ``ok``."""
    from gpumounter_amd.ops import probe
    from gpumounter_amd.parallel import validate

    calls = []

    def fake_scan(dev, **kw):
        calls.append((dev, kw))
        return {"ok": not any(v is not None for v in kw.values()), "failed": [],
                "per_cu": [{"id": 1}]}
    monkeypatch.setattr(probe, "device_count", lambda: 2)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": f"0000:0{d}:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2 * numel}] * world)
    monkeypatch.setattr(scan.module, "scan", fake_scan)

    def run(*opts):
        del calls[:]
        code = validate.main(["--no-p2p", f"--{scan.label}", *opts])
        return code, json.loads(capsys.readouterr().out)

    # validate has the negative controls of every scan but the CU scan
    controls = {} if scan.plain_cli else {f"_{name}": None for name in scan.controls}
    code, report = run()
    assert code == 0 and report["ok"] is True
    assert report[scan.key] == [{"ok": True, "failed": []}] * 2          # per_cu is gone
    assert sorted(calls, key=lambda c: c[0]) == [(0, controls), (1, controls)]
    others = [s.key for s in SCANS if s is not scan]
    assert not any(k in report for k in others) and "allreduce" in report
    texts = {"inject": f"any:{scan.all[0]}:0:0:1", "poke": f"{scan.all[0]}:7:8"}
    parsed = {"inject": ("any", scan.all[0], 0, 0, 1), "poke": (scan.all[0], 7, 8)}
    for name in controls:
        name = name[1:]
        code, report = run(f"--{scan.label}-{name}", texts[name])
        assert code == 1 and report["ok"] is False and report[scan.key][0]["ok"] is False
        assert "per_cu" not in report[scan.key][0] and "per_cu" not in report[scan.key][1]
        want = dict(controls, **{f"_{name}": parsed[name]})
        assert sorted(calls, key=lambda c: c[0]) == [(0, want), (1, want)]
