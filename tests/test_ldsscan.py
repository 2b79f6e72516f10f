"""The LDS scan above its kernel (gpumounter_amd/ops/ldsscan.py): the descriptor against the module
and the header, the refusals, the poke, its place behind the registry's four scans, the result
decoder, and the command lines of probe, doctor and validate. No GPU."""
import ctypes as C
import inspect
import json

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe, ldsscan
from gpumounter_amd.ops.probe import ProbeError

SCAN = ldsscan.SCAN


def test_descriptor_agrees_with_the_module_and_the_header():
    assert ldsscan.TESTS == {"width": 1, "atomic": 2, "bank": 4, "tr16": 8, "dma": 16}
    assert (SCAN.label, SCAN.key, SCAN.stem, SCAN.selection) == ("lds-scan", "ldsscan", "lds_scan",
                                                                 "tests")
    assert SCAN.module is ldsscan and SCAN.bits is ldsscan.TESTS and SCAN.all == ldsscan.ALL_TESTS
    assert (SCAN.default_iters, SCAN.max_iters) == (ldsscan.DEFAULT_ITERS, ldsscan.MAX_ITERS)
    assert ldsscan.MAX_ITERS == 63 and ldsscan.DEFAULT_ITERS in (1, 2, 4, 8, 16, 32)
    assert tuple(SCAN.controls) == ("inject", "poke") and not SCAN.plain_cli
    assert ldsscan.parse_tests("width, dma") == ("width", "dma")
    with pytest.raises(ProbeError, match="^unknown lds-scan test 'nope'"):
        ldsscan.bit_of("nope")
    # the bit table is the header's GM_LDSSCAN_ALL: every bit accepted, the next one refused
    expected = _native.probe().gm_probe_ldsscan_expected
    out = (C.c_uint32 * 1024)()
    bits = sorted(ldsscan.TESTS.values())
    assert bits == [1, 2, 4, 8, 16]
    for bit in bits:
        assert expected(bit, 0, 1, None, out) == 0
    assert expected(32, 0, 1, None, out) == 1 and expected(3, 0, 1, None, out) == 1
    assert expected(1, 0, 0, None, out) == 1 and expected(1, 0, 64, None, out) == 1
    assert expected(1, 0, 63, None, out) == 0
    assert ldsscan.geometry() == {"lds_bytes": 163840, "arena_bytes": 163840,
                                  "atomic_table_words": 5792, "tr16_strides": [32, 72, 264]}


def test_the_frames_eight_malformed_injections_are_refused():
    t = "width"
    for bad in (f"any:{t}:0:0", "any:nope:0:0:1", f"any:{t}:256:0:1", f"any:{t}:0:4:1",
                f"any:{t}:0:0:0", f"4096:{t}:0:0:1", f"any:{t}:x:0:1", f"any:{t}:0:0:0x100000000"):
        with pytest.raises(ProbeError, match="lds-scan|CU id"):
            ldsscan.parse_inject(bad)
    assert ldsscan.parse_inject("any:dma:255:3:0xffffffff") == ("any", "dma", 255, 3, 0xFFFFFFFF)
    assert ldsscan.parse_inject("0x123:tr16:130:2:0x10000") == (0x123, "tr16", 130, 2, 0x10000)


def test_poke_parsing_and_refusals():
    assert ldsscan.parse_poke("tr16:4099:0x10") == ("tr16", 4099, 16)
    assert ldsscan.parse_poke(" dma : 40959 : 0x80000000 ") == ("dma", 40959, 1 << 31)
    with pytest.raises(ProbeError, match="atomic has no data to poke"):
        ldsscan.parse_poke("atomic:0:1")
    for bad in ("bank:40960:1", "bank:0:0", "bank:-1:1", "bank:0", "bank:x:1", "nope:0:1",
                "bank:0:0x100000000"):
        with pytest.raises(ProbeError):
            ldsscan.parse_poke(bad)
    # a poke of a test that is not run, before the native library is reached
    with pytest.raises(ProbeError, match="poke of 'bank', which is not run"):
        ldsscan.scan(0, tests=("width",), _poke=("bank", 0, 1))
    with pytest.raises(ProbeError, match="which is not run"):
        ldsscan.signature("width", poke=("bank", 0, 1))
    with pytest.raises(ProbeError, match="atomic has no data to poke"):
        ldsscan.expected("atomic", poke=("atomic", 0, 1))
    # the native entry points refuse the same, before any HIP call
    lib, out, poke = _native.probe(), (C.c_uint32 * 1024)(), _native.LdsscanPoke
    for pk in (poke(2, 0, 1), poke(4, 40960, 1), poke(4, 0, 0), poke(32, 0, 1), poke(6, 0, 1)):
        assert lib.gm_probe_ldsscan_expected(4, 0, 1, C.byref(pk), out) == 1
    res, n, cus = _native.CuscanResult(), C.c_int(7), (_native.CuscanCu * 4)()
    assert lib.gm_probe_ldsscan(0, 1, 1, 0, 1, 1, None, C.byref(poke(4, 0, 1)), C.byref(res), cus,
                                4, C.byref(n)) == 1 and n.value == 0
    assert lib.gm_probe_ldsscan(0, 32, 1, 0, 1, 1, None, None, C.byref(res), cus, 4, C.byref(n)) == 1
    assert lib.gm_probe_ldsscan_kernel_info(None, None) == 1


def test_expected_tables_with_and_without_a_poke():
    clean = {t: ldsscan.expected(t, iters=1) for t in ldsscan.ALL_TESTS}
    for t, table in clean.items():
        assert table.shape == (256, 4) and table.dtype == np.uint32
        assert (ldsscan.expected(t, iters=1) == table).all()
        assert (ldsscan.expected(t, seed=1, iters=1) != table).any()
        assert (ldsscan.expected(t, iters=2) != table).any()
    for t in ("width", "bank", "tr16", "dma"):
        poked = ldsscan.expected(t, iters=1, poke=(t, 100, 0x10))
        assert (poked != clean[t]).any()
        for other in ldsscan.ALL_TESTS:        # a poke changes the table of its own test only
            if other != t:
                assert (ldsscan.expected(other, iters=1, poke=(t, 100, 0x10)) == clean[other]).all()
    # dma counts the poked word as one mismatch seen in flight
    assert clean["dma"][:, 3].sum() == 0
    assert ldsscan.expected("dma", iters=1, poke=("dma", 40959, 1 << 31))[:, 3].sum() == 1


def test_scans_is_the_registry_followed_by_the_lds_scan():
    assert cuframe.MORE_MODULES == ("ldsscan",)
    assert cuframe.scans() == cuframe.registry() + (SCAN,)
    assert [s.key for s in cuframe.scans()] == ["cuscan", "mfmascan", "lanescan", "cachescan",
                                                "ldsscan"]
    from gpumounter_amd import cli
    assert cli._scans() == cuframe.scans()


def test_scan_over_a_fake_native_entry_decodes_to_the_exact_dict(monkeypatch):
    a, b = "width", "atomic"
    seen = []

    def entry(*args):
        seen.append(args[:6])
        def behind(kind):          # what a byref argument refers to
            return [x._obj for x in args if isinstance(getattr(x, "_obj", None), kind)]
        (res,), (n,) = behind(_native.CuscanResult), behind(C.c_int)
        assert args[6] is None and args[7] is None and len(args) == 12      # no inject, no poke
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
        gm_probe_ldsscan = staticmethod(entry)
    monkeypatch.setattr(_native, "probe", lambda: Lib())
    got = ldsscan.scan(0)
    assert seen == [(0, 31, ldsscan.DEFAULT_ITERS, cuframe.DEFAULT_SEED, 1, 16)]
    good = {"id": 1, "xcc": 0, "se": 0, "sh": 0, "cu": 1, "runs": 3, "failed_runs": 0,
            "tests_failed": [], "simds_seen": [0, 1, 2, 3], "simds_failed": []}
    bad = {"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "runs": 3, "failed_runs": 2,
           "tests_failed": [a, b], "simds_seen": [0, 1, 2], "simds_failed": [2]}
    assert got == {
        "device": 0, "tests": list(ldsscan.ALL_TESTS), "iters": ldsscan.DEFAULT_ITERS,
        "cus_expected": 256, "cus_seen": 2, "complete": False, "rounds": 3, "blocks_run": 768,
        "words_in_error": 2, "failed_cus": 1, "blocks_four_simds": 700,
        "xcc_cus": [1, 0, 1] + [0] * 13, "seconds": 0.5, "kernel_ms": 1.25,
        "first_errors": [{"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "simd": 2, "test": b,
                          "thread": 130, "word": 2, "expected": "0x00000010",
                          "got": "0x00010010", "xor": "0x00010000"}],
        "failed": [{k: v for k, v in bad.items() if k != "simds_seen"}],
        "per_cu": [good, bad], "ok": False}
    assert ldsscan.describe_failed(got) == "xcc 2 se 1 sh 0 cu 5 (id 0x225) simd 2 width+atomic"


def test_command_lines_parse_the_lds_scan_options():
    from gpumounter_amd.cli import build_parser, cmd_doctor, cmd_probe
    from gpumounter_amd.parallel import validate

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.lds_scan is False and a.lds_scan_inject is None and a.lds_scan_poke is None
    assert a.lds_scan_tests is None and a.lds_scan_iters is None and a.lds_scan_rounds is None
    a = ap.parse_args(["probe", "--lds-scan", "--lds-scan-tests", "bank,tr16", "--lds-scan-iters",
                       "3", "--lds-scan-rounds", "2", "--lds-scan-inject", "any:bank:0:0:1",
                       "--lds-scan-poke", "tr16:4099:0x10"])
    assert a.lds_scan and tuple(a.lds_scan_tests) == ("bank", "tr16")
    assert a.lds_scan_iters == 3 and a.lds_scan_rounds == 2
    assert a.lds_scan_inject == ("any", "bank", 0, 0, 1) and a.lds_scan_poke == ("tr16", 4099, 16)
    for bad in (["--lds-scan-tests", "bank,nope"], ["--lds-scan-inject", "any:bank:0:0"],
                ["--lds-scan-iters", "x"], ["--lds-scan-poke", "atomic:0:1"],
                ["--lds-scan-poke", "bank:40960:1"], ["--lds-scan-poke", "bank:0:0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--lds-scan", *bad])
    # usage errors (2), not a failed scan (1), before any GPU work
    for opt in (["--lds-scan-inject", "any:bank:0:0:1"], ["--lds-scan-poke", "bank:0:1"],
                ["--lds-scan-iters", "3"], ["--lds-scan-tests", "bank"], ["--lds-scan-rounds", "2"]):
        assert cmd_probe(ap.parse_args(["probe", *opt])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--lds-scan", "--lds-scan-tests", "dma",
                                    "--lds-scan-poke", "bank:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--lds-scan", "--lds-scan-iters", "64"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--lds-scan", "--lds-scan-iters", "0"])) == 2
    d = ap.parse_args(["doctor", "--gpu", "--lds-scan", "--lds-scan-inject", "any:dma:1:2:4",
                       "--lds-scan-poke", "width:7:8"])
    assert d.lds_scan is True and d.lds_scan_inject == ("any", "dma", 1, 2, 4)
    assert d.lds_scan_poke == ("width", 7, 8)
    assert ap.parse_args(["doctor", "--gpu"]).lds_scan is False
    assert cmd_doctor(ap.parse_args(["doctor", "--lds-scan-poke", "width:7:8"])) == 2
    assert cmd_doctor(ap.parse_args(["doctor", "--lds-scan-inject", "any:dma:1:2:4"])) == 2
    for bad in (["--lds-scan-poke", "bank:0:1"], ["--lds-scan-inject", "any:bank:0:0:1"],
                ["--lds-scan", "--lds-scan-poke", "atomic:0:1"],
                ["--lds-scan", "--lds-scan-inject", "any:nope:0:0:1"]):
        with pytest.raises(SystemExit):
            validate.main(bad)


def _fake_gpu(monkeypatch):
    from gpumounter_amd.ops import probe
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)


def test_doctor_passes_the_scan_on_and_names_the_unit_and_test(monkeypatch):
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    for fn in (doctor.check_gpus, doctor.run):
        sig = inspect.signature(fn).parameters
        assert sig["lds_scan"].default is False and sig["lds_scan"].kind is sig["lds_scan"].KEYWORD_ONLY
        assert sig["lds_scan_inject"].default is None and sig["lds_scan_poke"].default is None
    calls = []

    def fake_scan(dev, _inject=None, _poke=None):
        calls.append((dev, _inject, _poke))
        bad = _inject is not None or _poke is not None
        failed = [{"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "runs": 1, "failed_runs": 1,
                   "tests_failed": ["tr16"], "simds_failed": [2]}] if bad else []
        return {"tests": list(ldsscan.ALL_TESTS), "cus_seen": 250, "cus_expected": 256,
                "complete": False, "rounds": 16, "kernel_ms": 1.0, "words_in_error": int(bad),
                "ok": not bad, "failed": failed}
    _fake_gpu(monkeypatch)
    monkeypatch.setattr(ldsscan, "scan", fake_scan)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "lds-scan" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, lds_scan=True) if c.name == "gpu0"]
    assert ok.status == "ok" and "lds-scan 5 tests 250/256 CUs" in ok.detail
    assert "incomplete" in ok.detail and " 0 wrong words" in ok.detail
    inj, pk = (0x123, "tr16", 130, 2, 0x10000), ("tr16", 4099, 0x10)
    (bad,) = [c for c in doctor.check_gpus(cfg, lds_scan=True, lds_scan_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail" and bad.detail.endswith("xcc 1 se 1 sh 0 cu 3 (id 0x123) simd 2 tr16")
    (bad,) = [c for c in doctor.check_gpus(cfg, lds_scan=True, lds_scan_poke=pk) if c.name == "gpu0"]
    assert bad.status == "fail" and bad.detail.endswith("simd 2 tr16")
    assert calls == [(0, None, None), (0, inj, None), (0, None, pk)]


def test_doctor_run_forwards_only_what_is_set(monkeypatch):
    from gpumounter_amd.utils import doctor

    calls = []
    for name in ("check_inventory", "check_cgroup", "check_devnodes", "check_pidns",
                 "check_systemd"):
        monkeypatch.setattr(doctor, name, lambda cfg: [])
    monkeypatch.setattr(doctor, "check_gpus", lambda cfg, burn_in_s=0.0, **kw: calls.append(kw) or [])
    doctor.run(None, skip_cluster=True, gpu=True)
    doctor.run(None, skip_cluster=True, gpu=True, lds_scan=True)
    doctor.run(None, skip_cluster=True, gpu=True, lds_scan=True, lds_scan_poke=("bank", 1, 2))
    doctor.run(None, skip_cluster=True, gpu=True, lds_scan=True,
               lds_scan_inject=("any", "dma", 0, 3, 1))
    doctor.run(None, skip_cluster=True, gpu=True, lds_scan_poke=("bank", 1, 2))    # not switched on
    base = {"memtest_bytes": 0}
    assert calls == [base, dict(base, lds_scan=True),
                     dict(base, lds_scan=True, lds_scan_poke=("bank", 1, 2)),
                     dict(base, lds_scan=True, lds_scan_inject=("any", "dma", 0, 3, 1)), base]


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
    monkeypatch.setattr(ldsscan, "scan", fake_scan)

    def run(*opts):
        del calls[:]
        code = validate.main(["--no-p2p", "--lds-scan", *opts])
        return code, json.loads(capsys.readouterr().out)

    none = {"_inject": None, "_poke": None}
    code, report = run()
    assert code == 0 and report["ok"] is True
    assert report["ldsscan"] == [{"ok": True, "failed": []}] * 2          # per_cu is gone
    assert sorted(calls, key=lambda c: c[0]) == [(0, none), (1, none)]
    assert not any(s.key in report for s in cuframe.registry())
    for opt, text, parsed in (("inject", "any:width:0:0:1", ("any", "width", 0, 0, 1)),
                              ("poke", "width:7:8", ("width", 7, 8))):
        code, report = run(f"--lds-scan-{opt}", text)
        assert code == 1 and report["ok"] is False and report["ldsscan"][0]["ok"] is False
        assert "per_cu" not in report["ldsscan"][0]
        want = dict(none, **{f"_{opt}": parsed})
        assert sorted(calls, key=lambda c: c[0]) == [(0, want), (1, want)]
