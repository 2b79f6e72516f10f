"""Host-link (PCIe) test, everything that needs no GPU: parsers, the ctypes mirrors, the native
argument checks, the sysfs link reader and its under-load sampler, the link arithmetic, and the
plumbing of probe / validate / doctor with the driver stubbed."""
import ctypes as C
import inspect
import json
import os

import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import hostlink, memtest
from gpumounter_amd.ops.probe import ProbeError

BDF = "0000:05:00.0"


# ------------------------------------------------------------------------------------- parsers
def test_constants():
    assert hostlink.LEGS == {"h2d": 1, "d2h": 2, "bidir": 4, "kread": 8, "kwrite": 16,
                             "kduplex": 32}
    assert hostlink.ALL_LEGS == ("h2d", "d2h", "bidir", "kread", "kwrite", "kduplex")
    assert hostlink.DEFAULT_BYTES == 256 << 20
    assert hostlink.DEFAULT_PATTERNS == ("addr", "random")
    # the Python constants are the loaded library's
    g = hostlink.geometry()
    assert g == {"step_bytes": hostlink.STEP_BYTES, "default_blocks": hostlink.DEFAULT_BLOCKS}
    assert hostlink.STEP_BYTES % (256 * 16) == 0
    assert 1 <= hostlink.DEFAULT_BLOCKS <= hostlink.MAX_BLOCKS == 1024


def test_unroll_hook_changes_the_step_and_only_for_4_and_8():
    lib = _native.probe()
    was = lib.gm_probe_hostlink_unroll(-1)
    try:
        assert was * 256 * 16 == hostlink.STEP_BYTES
        for u in (0, 1, 2, 3, 5, 16):
            assert lib.gm_probe_hostlink_unroll(u) == was         # a query, nothing set
        assert lib.gm_probe_hostlink_unroll(4) == was
        assert hostlink.geometry()["step_bytes"] == 4 * 256 * 16
        assert lib.gm_probe_hostlink_unroll(8) == 4
        assert hostlink.geometry()["step_bytes"] == 8 * 256 * 16
    finally:
        lib.gm_probe_hostlink_unroll(was)


def test_parse_legs():
    assert hostlink.parse_legs("h2d") == ("h2d",)
    assert hostlink.parse_legs(" kread , kwrite,") == ("kread", "kwrite")
    assert hostlink.legs_mask(hostlink.ALL_LEGS) == 63
    assert hostlink.legs_mask("bidir") == 4 and hostlink.legs_mask(32) == 32
    assert hostlink.legs_mask(("h2d", 2)) == 3
    for bad in ("", ",", "h2d,p2p", "H2D", "3"):
        with pytest.raises(ProbeError):
            hostlink.parse_legs(bad)
    for bad in ((), 3, 64, True, None, ("h2d", 1.0)):
        with pytest.raises((ProbeError, TypeError)):
            hostlink.legs_mask(bad)


def test_parse_flip():
    assert hostlink.parse_flip("kread:4096:0x10") == ("kread", 4096, 0x10)
    assert hostlink.parse_flip(" h2d : 0 : 1 ") == ("h2d", 0, 1)
    assert hostlink.parse_flip("kduplex:0x100:0xFFFFFFFFFFFFFFFF") == ("kduplex", 256, (1 << 64) - 1)
    for bad in ("kread:4096", "4096:0x10", "kread:4096:0x10:1", "p2p:0:1", "kread:x:1",
                "kread:0:y", "kread:4:1", "kread:-8:1", "kread:0:0", "kread:0:0x10000000000000000",
                ""):
        with pytest.raises(ProbeError):
            hostlink.parse_flip(bad)


def test_parse_blocks_and_patterns():
    assert hostlink.parse_blocks("1") == 1 and hostlink.parse_blocks("1024") == 1024
    for bad in ("0", "1025", "x", "-1", "1.5"):
        with pytest.raises(ProbeError):
            hostlink.parse_blocks(bad)
    assert hostlink.parse_patterns("addr,walk") == ("addr", "walk")
    with pytest.raises(ProbeError):
        hostlink.parse_patterns("addr,noise")
    assert hostlink.parse_size("4M") == 4 << 20


# ------------------------------------------------------------------------------ ctypes and native
def test_structs_mirror_the_header():
    """The numbers are the ones written in the header comment of gm_probe.h."""
    R = _native.HostlinkResult
    assert C.sizeof(_native.HostlinkLeg) == 32
    assert C.sizeof(_native.HostlinkRecord) == 40
    assert C.sizeof(R) == 992
    assert R.legs.offset == 48 and R.bidir_h2d.offset == 240 and R.bidir_d2h.offset == 272
    assert R.records.offset == 304 and R.seconds.offset == 944 and R.stage.offset == 976
    assert R.records_filled.offset == 40 and R.legs_run.offset == 44
    assert _native.HostlinkRecord.leg.offset == 24 and _native.HostlinkRecord.pass_.offset == 32
    assert _native.HOSTLINK_LEGS == len(hostlink.LEGS)
    header = open(os.path.join(os.path.dirname(__file__), "..", "native", "include",
                               "gm_probe.h")).read()
    for text in ("sizeof(gm_hostlink_leg_t) = 32", "sizeof(gm_hostlink_record_t) = 40",
                 "sizeof(gm_hostlink_result_t) = 992", "legs at byte 48", "bidir_h2d at 240",
                 "records at 304", "seconds at 944", "stage at 976"):
        assert text in " ".join(header.replace("//", " ").split())


def test_native_entry_points_validate_before_any_hip_call():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    res = _native.MemtestResult()
    P, Q = C.c_void_p(1 << 20), C.c_void_p(2 << 20)   # never dereferenced: refused first
    good = dict(ptr=P, nbytes=4096, pattern=1, base=0, blocks=4, flip_off=0)

    def kwrite(**kw):
        a = {**good, **kw}
        return lib.gm_probe_hostlink_kwrite(a["ptr"], a["nbytes"], a["pattern"], 0, 0, 0,
                                            a["base"], a["blocks"], a["flip_off"], 1, None)

    def kread(out=res, **kw):
        a = {**good, **kw}
        return lib.gm_probe_hostlink_kread(a["ptr"], a["nbytes"], a["pattern"], 0, 0, 0,
                                           a["base"], a["blocks"], None,
                                           C.byref(out) if out is not None else None)

    def kcopy(dst=Q, out=res, **kw):
        a = {**good, **kw}
        return lib.gm_probe_hostlink_kcopy(a["ptr"], dst, a["nbytes"], a["pattern"], 0, 0, 0,
                                           a["base"], a["blocks"], a["flip_off"], 1, None,
                                           C.byref(out) if out is not None else None)

    bad_buffers = (dict(ptr=None), dict(ptr=C.c_void_p((1 << 20) + 8)), dict(nbytes=0),
                   dict(nbytes=4104), dict(pattern=0), dict(pattern=3), dict(pattern=32),
                   dict(base=4), dict(blocks=0), dict(blocks=-1), dict(blocks=1025),
                   dict(ptr=C.c_void_p((1 << 64) - 4096), nbytes=8192))
    for kw in bad_buffers:
        assert kwrite(**kw) == 1, kw
        assert kread(**kw) == 1, kw
        assert kcopy(**kw) == 1, kw
    assert kwrite(flip_off=4) == 1 and kcopy(flip_off=12) == 1
    assert kread(out=None) == 1 and kcopy(out=None) == 1
    # kcopy: a bad destination, and every way of overlapping
    for dst in (None, C.c_void_p((2 << 20) + 8), P, C.c_void_p((1 << 20) + 4080),
                C.c_void_p((1 << 20) - 4080)):
        assert kcopy(dst=dst) == 1, dst

    out = _native.HostlinkResult()

    def drive(dev=0, nbytes=4096, legs=63, patterns=31, passes=1, iters=1, blocks=0, flip_leg=0,
              flip_off=0, flip_mask=0, res=out):
        return lib.gm_probe_hostlink(dev, nbytes, legs, patterns, passes, iters, blocks, 0,
                                     flip_leg, flip_off, flip_mask,
                                     C.byref(res) if res is not None else None)

    for kw in (dict(dev=-1), dict(nbytes=0), dict(nbytes=4104), dict(legs=0), dict(legs=64),
               dict(patterns=0), dict(patterns=32), dict(passes=0), dict(iters=0),
               dict(iters=1025), dict(blocks=-1), dict(blocks=1025),
               dict(flip_mask=1, flip_leg=0), dict(flip_mask=1, flip_leg=3),
               dict(flip_mask=1, flip_leg=64), dict(flip_mask=1, flip_leg=8, legs=7),
               dict(flip_mask=1, flip_leg=8, flip_off=4),
               dict(flip_mask=1, flip_leg=8, flip_off=4096),
               dict(flip_mask=1, flip_leg=8, flip_off=(1 << 64) - 8)):
        assert drive(**kw) == 1, kw
        assert out.stage == b"args" and out.pinned_bytes == 0 and out.legs_run == 0
    assert drive(res=None) == 1


def test_python_refuses_before_the_native_library(monkeypatch):
    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    for kw in (dict(legs=()), dict(legs=("h2d", "p2p")), dict(legs=64), dict(patterns=()),
               dict(patterns=("noise",)), dict(passes=0), dict(passes=True), dict(iters=0),
               dict(iters=1025), dict(iters=1.5), dict(blocks=0), dict(blocks=1025),
               dict(seed=-1), dict(seed=1 << 64), dict(nbytes=0), dict(nbytes=24),
               dict(nbytes=-16), dict(_flip=("kread", 0)), dict(_flip=("p2p", 0, 1)),
               dict(_flip=("kread", 4, 1)), dict(_flip=("kread", 0, 0)),
               dict(legs=("h2d",), _flip=("kread", 0, 1)),
               dict(nbytes=4096, _flip=("kread", 4096, 1))):
        with pytest.raises(ProbeError):
            hostlink.hostlink(0, **kw)
    with pytest.raises(ProbeError):
        hostlink.hostlink(-1)
    with pytest.raises(AssertionError):                  # a good call does get there
        hostlink.hostlink(0, _bdf=BDF)


def test_caller_owned_calls_want_pinned_tensors(monkeypatch):
    import torch

    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    pageable = torch.zeros(4096, dtype=torch.uint8)
    for call in (lambda: hostlink.kwrite(pageable, "addr"), lambda: hostlink.kread(pageable, "addr"),
                 lambda: hostlink.kcopy(pageable, pageable.clone(), "addr"),
                 lambda: hostlink.kread([1, 2], "addr")):
        with pytest.raises(ProbeError, match="pinned|torch tensor"):
            call()


# ------------------------------------------------------------------------------ the link in sysfs
def fake_device(root, bdf=BDF, **files):
    d = root / "bus" / "pci" / "devices" / bdf
    d.mkdir(parents=True, exist_ok=True)
    for name, text in files.items():
        (d / name).write_text(text)
    return d


FULL = dict(current_link_speed="32.0 GT/s PCIe\n", max_link_speed="32.0 GT/s PCIe\n",
            current_link_width="16\n", max_link_width="16\n", numa_node="1\n")


def test_link_state_full_partial_missing_garbage(tmp_path):
    fake_device(tmp_path, **FULL)
    assert hostlink.link_state(BDF, str(tmp_path)) == {
        "bdf": BDF, "speed_gts": 32.0, "max_speed_gts": 32.0, "width": 16, "max_width": 16,
        "numa_node": 1}
    # the address is looked up in lower case, as sysfs spells it
    assert hostlink.link_state(BDF.upper(), str(tmp_path))["width"] == 16

    partial = tmp_path / "partial"
    fake_device(partial, current_link_speed="2.5 GT/s PCIe", max_link_width="8", numa_node="-1")
    st = hostlink.link_state(BDF, str(partial))
    assert st == {"bdf": BDF, "speed_gts": 2.5, "max_speed_gts": None, "width": None,
                  "max_width": 8, "numa_node": -1}

    nothing = {"bdf": BDF, "speed_gts": None, "max_speed_gts": None, "width": None,
               "max_width": None, "numa_node": None}
    assert hostlink.link_state(BDF, str(tmp_path / "nowhere")) == nothing
    assert hostlink.link_state("0000:ff:00.0", str(tmp_path)) == {**nothing, "bdf": "0000:ff:00.0"}

    garbage = tmp_path / "garbage"
    d = fake_device(garbage, current_link_speed="Unknown", max_link_speed="fast GT/s",
                    current_link_width="sixteen", max_link_width="0", numa_node="")
    assert hostlink.link_state(BDF, str(garbage)) == nothing
    (d / "current_link_speed").write_bytes(b"\xff\xfe\x00 GT/s")
    (d / "max_link_speed").write_text("-8.0 GT/s PCIe")
    (d / "current_link_width").write_text("9" * 40)
    (d / "numa_node").unlink()
    (d / "numa_node").mkdir()                     # a directory where a file should be
    assert hostlink.link_state(BDF, str(garbage)) == nothing


def test_link_files_are_opened_read_only(tmp_path, monkeypatch):
    fake_device(tmp_path, **FULL)
    flags = []
    real = os.open

    def spy(path, fl, *a, **kw):
        flags.append(fl)
        return real(path, fl, *a, **kw)
    monkeypatch.setattr(os, "open", spy)
    hostlink.link_state(BDF, str(tmp_path))
    assert len(flags) == len(hostlink.LINK_FILES)
    assert all(fl & (os.O_WRONLY | os.O_RDWR | os.O_CREAT | os.O_TRUNC) == 0 for fl in flags)


def test_link_arithmetic():
    assert hostlink.link_gbps(32.0, 16) == pytest.approx(32 * 16 * 128 / 130 / 8)   # 63.0
    assert hostlink.link_gbps(32.0, 16) == pytest.approx(63.0, abs=0.05)
    assert hostlink.link_gbps(16.0, 8) == pytest.approx(15.75, abs=0.01)
    assert hostlink.link_gbps(None, 16) is None and hostlink.link_gbps(32.0, None) is None
    top = {"speed_gts": 32.0, "width": 16, "max_speed_gts": 32.0, "max_width": 16}
    assert hostlink.degraded(top) is False
    assert hostlink.degraded({**top, "width": 8}) is True
    assert hostlink.degraded({**top, "speed_gts": 16.0}) is True
    assert hostlink.degraded({**top, "speed_gts": None, "width": None}) is False
    assert hostlink.degraded({**top, "max_width": None, "width": 8}) is False
    assert hostlink.describe_link({**top, "width": 8, "speed_gts": 16.0}) == \
        "x8 of x16, 16.0 of 32.0 GT/s"
    assert hostlink.describe_link({}) == "x? of x?, ? of ? GT/s"
    assert hostlink.rate_above_link(63.1, top) is True
    assert hostlink.rate_above_link(62.9, top) is False
    assert hostlink.rate_above_link(100.0, top, directions=2) is False
    assert hostlink.rate_above_link(127.0, top, directions=2) is True
    assert hostlink.rate_above_link(1e9, {"speed_gts": None, "width": None}) is False


def test_sampler_keeps_the_highest_state_seen_under_load(tmp_path):
    """At rest the link idles at 2.5 GT/s; mid-call it trains up, then falls back before the call
    returns. The report holds what was seen under load, and the state at rest beside it."""
    idle = dict(FULL, current_link_speed="2.5 GT/s PCIe\n")
    d = fake_device(tmp_path, **idle)

    def native_call(sampler):
        assert sampler.wait_for_sample()
        (d / "current_link_speed").write_text("32.0 GT/s PCIe\n")
        assert sampler.wait_for_sample()
        (d / "current_link_speed").write_text("2.5 GT/s PCIe\n")
        assert sampler.wait_for_sample()
        return 0

    rc, link = hostlink.sample_link_during(native_call, BDF, str(tmp_path), interval=0.001)
    assert rc == 0
    assert link["rest"] == {"speed_gts": 2.5, "width": 16}
    assert link["speed_gts"] == 32.0 and link["width"] == 16
    assert link["max_speed_gts"] == 32.0 and link["max_width"] == 16 and link["numa_node"] == 1
    assert link["degraded"] is False and link["readable"] is True and link["samples"] >= 4
    assert link["gbps_per_direction"] == pytest.approx(63.0, abs=0.05)


def test_sampler_reports_a_link_that_stays_narrow_and_one_it_cannot_read(tmp_path):
    d = fake_device(tmp_path, **dict(FULL, current_link_width="8\n"))

    def native_call(sampler):
        (d / "current_link_speed").write_text("16.0 GT/s PCIe\n")
        assert sampler.wait_for_sample()
        return 7
    rc, link = hostlink.sample_link_during(native_call, BDF, str(tmp_path), interval=0.001)
    assert rc == 7 and link["degraded"] is True
    assert (link["speed_gts"], link["width"]) == (16.0, 8)
    assert hostlink.describe_link(link) == "x8 of x16, 16.0 of 32.0 GT/s"

    rc, link = hostlink.sample_link_during(lambda s: 0, BDF, str(tmp_path / "none"),
                                           interval=0.001)
    assert rc == 0 and link["readable"] is False and link["degraded"] is False
    assert link["speed_gts"] is None and link["samples"] >= 1
    # no address, no sampler: the call still runs
    rc, link = hostlink.sample_link_during(lambda s: s, None)
    assert rc is None and link["readable"] is False and link["samples"] == 0

    # an exception in the call stops the thread and comes through
    with pytest.raises(ZeroDivisionError):
        hostlink.sample_link_during(lambda s: 1 / 0, BDF, str(tmp_path), interval=0.001)


# ------------------------------------------------------------------- the driver, native call stubbed
class FakeLib:
    """Stands in for libgm_probe.so: fills the result as the driver would."""

    def __init__(self, rc=0, stage=b"", during=None, flip_leg=None):
        self.rc, self.stage, self.during, self.calls = rc, stage, during, []
        self.flip_leg = flip_leg

    def gm_probe_hostlink(self, dev, nbytes, legs, patterns, passes, iters, blocks, seed,
                          flip_leg, flip_off, flip_mask, out):
        self.calls.append((dev, nbytes, legs, patterns, passes, iters, blocks, seed, flip_leg,
                           flip_off, flip_mask))
        if self.during:
            self.during()
        r = out._obj
        r.stage = self.stage
        if self.rc:
            return self.rc
        r.bytes, r.pinned_bytes, r.legs_run = nbytes, 2 * nbytes, legs
        for i in range(6):
            if legs >> i & 1:
                r.legs[i].bytes = nbytes * iters
                r.legs[i].ms = 1.0
                r.legs[i].gbps = 50.0 if i != 2 else 100.0
        r.legs[3].gbps = 70.0                     # kread: above a x16 Gen5 link's 63 GB/s
        r.bidir_h2d.gbps, r.bidir_d2h.gbps = 52.0, 48.0
        if flip_mask:
            i = flip_leg.bit_length() - 1
            r.legs[i].words_in_error = r.words_in_error = 1
            r.bit_errors, r.stuck_mask, r.records_filled = 1, flip_mask, 1
            rec = r.records[0]
            rec.offset, rec.expected, rec.got = flip_off, 0xF0, 0xF0 ^ flip_mask
            rec.leg, rec.pattern, rec.pass_ = flip_leg, 1, 0
        r.seconds, r.host_seconds, r.transfer_seconds, r.setup_seconds = 1.0, 0.4, 0.5, 0.1
        return 0

    def gm_probe_strerror(self, rc):
        return b"out of memory" if rc == 2 else b"some error"


def test_hostlink_report_with_a_stubbed_native_call(tmp_path, monkeypatch):
    d = fake_device(tmp_path, **dict(FULL, current_link_speed="2.5 GT/s PCIe\n"))
    lib = FakeLib(during=lambda: (d / "current_link_speed").write_text("32.0 GT/s PCIe\n"))
    monkeypatch.setattr(_native, "probe", lambda: lib)
    r = hostlink.hostlink(0, 4 << 20, _sysfs=str(tmp_path), _bdf=BDF)
    assert lib.calls == [(0, 4 << 20, 63, 17, 1, 4, 0, hostlink.DEFAULT_SEED, 0, 0, 0)]
    assert r["ok"] is True and r["errors"] == 0 and r["first_errors"] == []
    assert r["pinned_bytes"] == 8 << 20 and r["blocks"] == hostlink.DEFAULT_BLOCKS
    assert list(r["legs"]) == list(hostlink.ALL_LEGS) and r["patterns"] == ["addr", "random"]
    assert r["seconds"] == 1.0 and r["host_seconds"] == 0.4
    # the speed the call raised is the one reported; the reading at rest is kept beside it
    assert r["link"]["speed_gts"] == 32.0 and r["link"]["rest"]["speed_gts"] == 2.5
    assert r["link"]["degraded"] is False
    # 70 GB/s cannot have crossed a 63 GB/s link; 100 GB/s in two directions can have
    assert r["legs"]["kread"]["rate_above_link"] is True
    assert r["legs"]["h2d"]["rate_above_link"] is False
    assert r["legs"]["bidir"]["rate_above_link"] is False
    assert r["legs"]["bidir"]["h2d"]["gbps"] == 52.0 and r["legs"]["bidir"]["d2h"]["gbps"] == 48.0
    assert r["ok"] is True                        # neither a rate nor the link changes ok
    json.dumps(r)

    # a narrow link: degraded, more rates above it, still ok
    (d / "current_link_width").write_text("8\n")
    r = hostlink.hostlink(0, 4 << 20, legs=("h2d", "kread"), _sysfs=str(tmp_path), _bdf=BDF)
    assert list(r["legs"]) == ["h2d", "kread"] and lib.calls[-1][2] == 9
    assert r["link"]["degraded"] is True and r["legs"]["h2d"]["rate_above_link"] is True
    assert r["ok"] is True

    # the negative control
    r = hostlink.hostlink(0, 4 << 20, patterns=("addr",), blocks=16, iters=2,
                          _flip=("kwrite", 4096, 0x10), _sysfs=str(tmp_path), _bdf=BDF)
    assert lib.calls[-1] == (0, 4 << 20, 63, 1, 1, 2, 16, hostlink.DEFAULT_SEED, 16, 4096, 0x10)
    assert r["ok"] is False and r["errors"] == 1 and r["legs"]["kwrite"]["errors"] == 1
    assert r["first_errors"] == [{"leg": "kwrite", "pattern": "addr", "pass": 0, "offset": 4096,
                                  "expected": "0x00000000000000f0", "got": "0x00000000000000e0",
                                  "xor": "0x0000000000000010"}]
    assert hostlink.describe_errors(r) == \
        "kwrite: 1 wrong word(s) first at offset 4096 xor 0x0000000000000010"


def test_a_refused_pin_is_told_apart(tmp_path, monkeypatch):
    monkeypatch.setattr(_native, "probe", lambda: FakeLib(rc=2, stage=b"pin"))
    with pytest.raises(hostlink.HostlinkError, match="pinning .* refused.*memlock") as e:
        hostlink.hostlink(0, 4 << 20, _sysfs=str(tmp_path), _bdf=BDF)
    assert e.value.stage == "pin" and e.value.code == 2 and isinstance(e.value, ProbeError)
    monkeypatch.setattr(_native, "probe", lambda: FakeLib(rc=700, stage=b"kread"))
    with pytest.raises(hostlink.HostlinkError, match="host-link kread: hip error 700") as e:
        hostlink.hostlink(0, 4 << 20, _sysfs=str(tmp_path), _bdf=BDF)
    assert e.value.stage == "kread"


# --------------------------------------------------------------------------------- command lines
def test_probe_command_line(monkeypatch, capsys):
    from gpumounter_amd.cli import build_parser, cmd_probe

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.host_link is None and a.host_link_flip is None and a.host_link_legs is None
    a = ap.parse_args(["probe", "--host-link"])
    assert a.host_link == -1
    a = ap.parse_args(["probe", "--host-link", "4M", "--host-link-legs", "kread,h2d",
                       "--host-link-patterns", "walk", "--host-link-blocks", "16",
                       "--host-link-flip", "kread:4096:0x10"])
    assert a.host_link == 4 << 20 and a.host_link_legs == ("kread", "h2d")
    assert a.host_link_patterns == ("walk",) and a.host_link_blocks == 16
    assert a.host_link_flip == ("kread", 4096, 0x10)
    for bad in (["--host-link", "4Q"], ["--host-link-legs", "h2d,p2p"],
                ["--host-link-flip", "p2p:0:1"], ["--host-link-flip", "kread:0"],
                ["--host-link-flip", "kread:4:1"], ["--host-link-patterns", "noise"],
                ["--host-link-blocks", "0"], ["--host-link-blocks", "2000"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["probe", "--host-link", *bad] if bad[0] != "--host-link"
                          else ["probe", *bad])
        assert e.value.code == 2
    # usage errors (2) before any GPU work: nothing below may reach the probe
    from gpumounter_amd.ops import probe

    def unreachable(*a, **kw):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(probe, "device_count", unreachable)
    monkeypatch.setattr(probe, "verify", unreachable)
    for argv in (["--host-link-flip", "kread:4096:0x10"], ["--host-link-legs", "h2d"],
                 ["--host-link-patterns", "addr"], ["--host-link-blocks", "4"],
                 ["--host-link", "4M", "--host-link-legs", "h2d,d2h", "--host-link-flip",
                  "kread:4096:0x10"],
                 ["--host-link", "4096", "--host-link-flip", "kread:4096:0x10"],
                 ["--host-link", "24"], ["--host-link", "0"]):
        assert cmd_probe(ap.parse_args(["probe", *argv])) == 2, argv
    assert "needs --host-link" in capsys.readouterr().err
    assert ap.parse_args(["doctor", "--gpu", "--host-link"]).host_link == -1
    assert ap.parse_args(["doctor", "--gpu", "--host-link", "64M"]).host_link == 64 << 20
    assert ap.parse_args(["doctor", "--gpu"]).host_link is None


def _report(dev, flip=None, degraded=False):
    legs = {n: {"bytes": 1, "ms": 1.0, "gbps": 50.0, "errors": 0, "rate_above_link": False}
            for n in hostlink.ALL_LEGS}
    first = []
    if flip:
        legs[flip[0]]["errors"] = 2
        first = [{"leg": flip[0], "pattern": "addr", "pass": 0, "offset": flip[1],
                  "expected": "0x0", "got": "0x1", "xor": f"{flip[2]:#018x}"}]
    link = {"speed_gts": 16.0 if degraded else 32.0, "width": 8 if degraded else 16,
            "max_speed_gts": 32.0, "max_width": 16, "degraded": degraded}
    return {"device": dev, "bytes": 4 << 20, "legs": legs, "errors": 2 if flip else 0,
            "first_errors": first, "ok": not flip, "link": link}


def test_probe_runs_the_driver_and_exits_1_on_a_wrong_word(monkeypatch, capsys):
    from gpumounter_amd.cli import build_parser, cmd_probe
    from gpumounter_amd.ops import probe

    class R:
        def __init__(self, d):
            self.d = d

        def to_dict(self):
            return {"device": self.d, "bdf": BDF}
    calls = []

    def fake(dev, nbytes=None, **kw):
        calls.append((dev, nbytes, kw))
        return _report(dev, kw.get("_flip"))
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [R(0), R(1)])
    monkeypatch.setattr(hostlink, "hostlink", fake)
    ap = build_parser()
    assert cmd_probe(ap.parse_args(["probe", "--bdf", BDF, "--host-link"])) == 0
    out = json.loads(capsys.readouterr().out)
    assert [r["hostlink"]["ok"] for r in out] == [True, True]
    assert calls[0] == (0, None, dict(legs=hostlink.ALL_LEGS, patterns=hostlink.DEFAULT_PATTERNS,
                                      blocks=None, _flip=None))
    calls.clear()
    assert cmd_probe(ap.parse_args(["probe", "--bdf", BDF, "--host-link", "4M",
                                    "--host-link-legs", "kread", "--host-link-blocks", "8",
                                    "--host-link-flip", "kread:4096:0x10"])) == 1
    assert calls[1] == (1, 4 << 20, dict(legs=("kread",), patterns=hostlink.DEFAULT_PATTERNS,
                                         blocks=8, _flip=("kread", 4096, 0x10)))
    assert "kread" in capsys.readouterr().out
    calls.clear()
    assert cmd_probe(ap.parse_args(["probe", "--bdf", BDF])) == 0 and calls == []


def test_validate_runs_every_gpu_and_reports(monkeypatch, capsys):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.parallel import collectives, validate

    calls = []

    def fake(dev, nbytes=None, **kw):
        calls.append((dev, nbytes))
        return _report(dev, ("d2h", 8, 1) if dev == 1 and nbytes == 32 else None)
    monkeypatch.setattr(probe, "device_count", lambda: 2)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": BDF, "gcn_arch": "gfx950"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(collectives, "xgmi_matrix", lambda devs: {"peer": [[True]]})
    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2}] * world)
    monkeypatch.setattr(hostlink, "hostlink", fake)
    assert validate.main(["--no-p2p"]) == 0 and calls == []
    assert "hostlink" not in json.loads(capsys.readouterr().out)
    assert validate.main(["--no-p2p", "--host-link"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert sorted(calls) == [(0, None), (1, None)] and len(rep["hostlink"]) == 2 and rep["ok"]
    calls.clear()
    assert validate.main(["--no-p2p", "--host-link", "32"]) == 1
    rep = json.loads(capsys.readouterr().out)
    assert sorted(calls) == [(0, 32), (1, 32)] and rep["ok"] is False
    assert [h["ok"] for h in rep["hostlink"]] == [True, False]
    for bad in ("4Q", "24", "0"):
        with pytest.raises(SystemExit) as e:
            validate.main(["--no-p2p", "--host-link", bad])
        assert e.value.code == 2
    capsys.readouterr()
    # CPU ranks: no GPU check of any kind
    calls.clear()
    assert validate.main(["--cpu-ranks", "2", "--host-link"]) == 0 and calls == []


def test_doctor_fails_on_a_wrong_word_or_refused_pin_and_warns_on_the_link(monkeypatch):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["host_link_bytes"].default == 0
    assert sig["host_link_bytes"].kind is sig["host_link_bytes"].KEYWORD_ONLY
    assert sig["host_link_flip"].default is None
    assert inspect.signature(doctor.run).parameters["host_link_bytes"].default == 0

    calls, mode = [], {"degraded": False, "refuse": False}

    def fake(dev, nbytes=None, _flip=None):
        calls.append((dev, nbytes, _flip))
        if mode["refuse"]:
            raise hostlink.HostlinkError("host-link: pinning 64 bytes of host memory was "
                                         "refused: hip error 2 (out of memory); check the "
                                         "container's memlock limit", "pin", 2)
        return _report(dev, _flip, mode["degraded"])
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": BDF,
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(hostlink, "hostlink", fake)
    monkeypatch.setattr(hostlink, "describe_errors", hostlink.describe_errors)
    cfg = Config.load(env={}, amdsmi_lib="mock")

    def gpu0(**kw):
        (c,) = [c for c in doctor.check_gpus(cfg, **kw) if c.name == "gpu0"]
        return c
    plain = gpu0()
    assert "host-link" not in plain.detail and calls == []
    ok = gpu0(host_link_bytes=-1)
    assert ok.status == "ok" and "host-link 4 MiB" in ok.detail and "kread 50.0" in ok.detail
    assert calls == [(0, None, None)]
    bad = gpu0(host_link_bytes=4 << 20, host_link_flip=("kduplex", 4096, 0x10))
    assert calls[-1] == (0, 4 << 20, ("kduplex", 4096, 0x10))
    assert bad.status == "fail" and "kduplex: 2 wrong word(s) first at offset 4096" in bad.detail
    mode["degraded"] = True
    warn = gpu0(host_link_bytes=-1)
    assert warn.status == "warn" and "x8 of x16, 16.0 of 32.0 GT/s" in warn.detail
    # a wrong word is not softened by the link warning
    assert gpu0(host_link_bytes=-1, host_link_flip=("h2d", 0, 1)).status == "fail"
    mode.update(degraded=False, refuse=True)
    refused = gpu0(host_link_bytes=-1)
    assert refused.status == "fail" and "refused" in refused.detail and "memlock" in refused.detail
    assert "hip error 2" in refused.detail


def test_doctor_command_passes_the_size_on(monkeypatch, capsys):
    from gpumounter_amd import cli
    from gpumounter_amd.utils import doctor

    seen = []

    def fake_run(cfg, **kw):
        seen.append(kw)
        return [doctor.Check("stub", "ok", "")]
    monkeypatch.setattr(doctor, "run", fake_run)
    ap = cli.build_parser()
    assert cli.cmd_doctor(ap.parse_args(["doctor", "--skip-cluster"])) == 0
    assert "host_link_bytes" not in seen[-1] and seen[-1]["gpu"] is False
    assert cli.cmd_doctor(ap.parse_args(["doctor", "--skip-cluster", "--host-link"])) == 0
    assert seen[-1]["host_link_bytes"] == -1 and seen[-1]["gpu"] is True
    assert cli.cmd_doctor(ap.parse_args(["doctor", "--skip-cluster", "--gpu", "--host-link",
                                         "64M"])) == 0
    assert seen[-1]["host_link_bytes"] == 64 << 20


def test_memtest_reference_is_the_one_the_kernels_share():
    """The host-link kernels take every expected value from the memtest pattern function; its
    host evaluation is what the GPU tests compare with."""
    e = memtest.expected("addr", 5, 0, (1 << 35) - 8, 2)
    assert [int(x) for x in e] == [((1 << 35) - 8) ^ 5, (1 << 35) ^ 5]
