"""The host-GPU atomics and hand-off test without a GPU: the parsers and every refusal, the
struct layout, the host reference (gm_probe_hostsync_expected) against independent numpy folds
over blocks + host_threads, the decoding of a native result, and the doctor / probe / validate
wiring against a stubbed call."""
import ctypes as C
import inspect
import json

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import hostsync
from gpumounter_amd.ops.probe import ProbeError

SEED = 0x0123456789ABCDEF
SHAPES = ((1, 0, 1, 1), (2, 1, 3, 64), (9, 3, 3, 1))      # blocks, host_threads, iters, spread
M32 = np.uint64(0xFFFFFFFF)


def H(seed, test, idx):
    """gm_probe.h's mixer on a uint32 index array, in uint64 arithmetic masked to 32 bits."""
    idx = np.asarray(idx, dtype=np.uint64)
    h = (np.uint64(seed & 0xFFFFFFFF) ^ (idx * np.uint64(0x9E3779B1) & M32))
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x85EBCA6B) & M32
    h ^= h >> np.uint64(13)
    h = (h + (np.uint64(seed >> 32) ^ np.uint64(test * 0xC2B2AE35 & 0xFFFFFFFF))) & M32
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0xC2B2AE35) & M32
    h ^= h >> np.uint64(13)
    h = h * np.uint64(0x27D4EB2F) & M32
    h ^= h >> np.uint64(16)
    return h


def numpy_fold(kind, total_blocks, iters, width, seed):
    """The final table by np.ufunc.at over every thread of the GPU blocks and the host-played
    ones: nothing shared with the C fold but the formulas of gm_probe.h."""
    k = hostsync.KINDS[kind]
    T = total_blocks * 256
    g, s = np.meshgrid(np.arange(T, dtype=np.uint64), np.arange(iters, dtype=np.uint64),
                       indexing="ij")
    g, s = g.ravel(), s.ravel()
    idx = g * np.uint64(1024) + s
    w = ((g + np.uint64(97) * s) % np.uint64(width)).astype(np.int64)
    if kind == "swap":
        return (w.astype(np.uint64) << np.uint64(32)) | (np.uint64(1) + idx)
    if kind == "count":
        return np.bincount(w, minlength=width).astype(np.uint32)
    h, hi = H(seed, 0x100 + k, idx), H(seed, 0x120 + k, idx)
    t = np.zeros(width, np.uint64)
    if kind == "add_u32":
        np.add.at(t, w, h)
        return (t & M32).astype(np.uint32)
    if kind == "ticket":
        np.add.at(t, w, np.uint64(1) + (h & np.uint64(3)))
        return t.astype(np.uint32)
    np.add.at(t, w, (hi << np.uint64(32)) | h)         # add_u64, cas: wraps modulo 2^64
    return t


@pytest.mark.parametrize("blocks,threads,iters,spread", SHAPES)
@pytest.mark.parametrize("kind", tuple(hostsync.KINDS))
def test_expected_equals_the_numpy_fold(kind, blocks, threads, iters, spread):
    got = hostsync.expected(kind, blocks, threads, iters, spread, SEED)
    width = hostsync.cas_width(blocks, threads, iters, spread) if kind == "cas" else spread
    want = numpy_fold(kind, blocks + threads, iters, width, SEED)
    assert got.dtype == (np.uint64 if kind in hostsync.WIDE else np.uint32)
    assert got.shape == ((blocks + threads) * 256 * iters,) if kind == "swap" else (width,)
    np.testing.assert_array_equal(got, want)


def test_expected_is_the_atomics_reference_over_the_sum_and_the_cas_width_rule():
    from gpumounter_amd.ops import atomics

    for kind in ("add_u32", "add_u64", "ticket"):
        np.testing.assert_array_equal(hostsync.expected(kind, 9, 3, 3, 64, SEED),
                                      atomics.expected(kind, 12, 3, 64, SEED))
    assert hostsync.cas_width(9, 3, 3, 1) == atomics.widths(12, 3, 1)["cas"]["width"] == 16
    assert hostsync.cas_width(1, 0, 1, 1) == 1 and hostsync.cas_width(16, 2) == 4096
    # a host-played block changes the table: 2 + 1 is not 2 + 0
    assert (hostsync.expected("add_u32", 2, 1, 3, 64) != hostsync.expected("add_u32", 2, 0, 3, 64)
            ).any()
    index = 3 << 20 | 2 << 14 | 1500
    assert hostsync.payload("d2h", 3, 2, 1500, SEED) == int(H(SEED, 0x601, index))
    assert hostsync.payload(0, 3, 2, 1500, SEED) == int(H(SEED, 0x600, index))


def test_parsers():
    assert hostsync.parse_tests("add,ticket, swap,cas,handoff") == hostsync.ALL_TESTS
    assert hostsync.parse_tests("handoff") == ("handoff",)
    assert hostsync.mask_of(("add", 16)) == 17 and hostsync.mask_of("swap") == 4
    assert hostsync.mask_of(hostsync.ALL_TESTS) == 31
    assert hostsync.parse_inject("add:add_u64:300:2:0x1") == ("add", "add_u64", 300, 2, 1)
    assert hostsync.parse_inject("add:0:4100:0:7") == ("add", "add_u32", 4100, 0, 7)
    assert hostsync.parse_inject("cas:300:2:0x10") == ("cas", 300, 2, 16)
    assert hostsync.parse_inject("ticket:300:2") == ("ticket", 300, 2)
    assert hostsync.parse_inject("swap:300:2:0x10") == ("swap", 300, 2, 16)
    assert hostsync.parse_inject("handoff:d2h:3:2:1500:0x100") == ("handoff", "d2h", 3, 2, 1500,
                                                                   256)
    assert hostsync.parse_inject("handoff:0:3:2:1500:1") == ("handoff", "h2d", 3, 2, 1500, 1)
    for bad in ("", "add", "sub:1:2", "add:add_u32:0:0", "add:add_f32:0:0:1", "add:2:0:0:1",
                "add:add_u32:0:0:0", "cas:0:0:x", "ticket:0", "ticket:0:0:1", "swap:0:0",
                "swap:0:0:0", "handoff:0:0:0:1", "handoff:up:0:0:0:1", "handoff:2:0:0:0:1",
                "handoff:h2d:0:64:0:1", "handoff:h2d:4096:0:0:1", "handoff:h2d:0:0:16384:1",
                "handoff:h2d:0:0:0:0", "cas:0:1024:1", f"swap:{(4096 + 8) * 256}:0:1"):
        with pytest.raises(ProbeError):
            hostsync.parse_inject(bad)
    for bad in ("", "add,sub", ",", "xor"):
        with pytest.raises(ProbeError):
            hostsync.parse_tests(bad)
    inj = hostsync._inject_arg(("handoff", "d2h", 3, 2, 1500, 0x100))
    assert (inj.test, inj.kind, inj.a, inj.b, inj.word, inj.mask) == (16, 1, 3, 2, 1500, 256)
    inj = hostsync._inject_arg(("add", "add_u64", 5, 1, 3))
    assert (inj.test, inj.kind, inj.a, inj.b, inj.word, inj.mask) == (1, 1, 5, 1, 0, 3)
    inj = hostsync._inject_arg(("swap", 5, 1, 3))
    assert (inj.test, inj.kind, inj.a, inj.b, inj.word, inj.mask) == (4, 0, 5, 1, 0, 3)


def test_python_validates_before_the_native_call(monkeypatch):
    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    for kw in (dict(tests=()), dict(tests=("add", "sub")), dict(tests=32), dict(blocks=-1),
               dict(blocks=4097), dict(blocks=True), dict(host_threads=-1),
               dict(host_threads=9), dict(iters=0), dict(iters=1025),
               dict(blocks=4, host_threads=1, iters=1024),          # 5 * 256 * 1024 > 2^20
               dict(spread=0), dict(spread=48), dict(spread=131072), dict(rounds=0),
               dict(rounds=65), dict(lines=2), dict(budget_us=0), dict(budget_us=20001),
               dict(host_budget_us=0), dict(host_budget_us=100001), dict(seed=-1),
               dict(seed=1 << 64), dict(blocks=4096, rounds=64),      # 32 GiB of mailboxes
               dict(host_threads=0),                                  # the hand-off needs one
               dict(tests=("handoff",), host_threads=0),
               dict(_inject=("add", "cas", 0, 0, 1)), dict(_inject=("add", "add_u32", 0, 0, 0)),
               dict(_inject=("cas", 0, 0)), dict(_inject=("ticket", -1, 0)),
               dict(_inject=("swap", 0, 0, 0)), dict(_inject=("handoff", "h2d", 0, 64, 0, 1)),
               dict(_inject=("handoff", "h2d", 0, 0, 16384, 1)), dict(_inject=("sub", 0, 0)),
               dict(_inject=("handoff", 2, 0, 0, 0, 1)),
               # an injection into a test that is not run
               dict(tests=("add",), _inject=("ticket", 0, 0)),
               dict(tests=("add", "cas"), _inject=("handoff", "h2d", 0, 0, 0, 1)),
               # a place beyond the geometry
               dict(blocks=2, host_threads=1, _inject=("swap", 3 * 256, 0, 1)),
               dict(blocks=2, iters=3, _inject=("cas", 0, 3, 1)),
               dict(blocks=2, _inject=("handoff", "d2h", 2, 0, 0, 1)),
               dict(blocks=2, rounds=3, _inject=("handoff", "d2h", 0, 3, 0, 1)),
               dict(blocks=2, lines=1, _inject=("handoff", "d2h", 0, 0, 1024, 1))):
        with pytest.raises(ProbeError):
            hostsync.run(0, **kw)
    with pytest.raises(ProbeError):
        hostsync.run(-1)
    for call in (lambda: hostsync.handoff(1, 0), lambda: hostsync.add("cas", 1),
                 lambda: hostsync.add("add_u32", 1, 0, 1, 48),
                 lambda: hostsync.swap(1, 0, 1, 1, _inject=("swap", 256, 0, 1)),
                 lambda: hostsync.ticket(1, 9), lambda: hostsync.cas(0),
                 lambda: hostsync.expected("xor_u64", 1), lambda: hostsync.cas_width(1, 0, 1, 3)):
        with pytest.raises(ProbeError):
            call()
    for kw in ({}, dict(tests=("add", "swap"), host_threads=0),       # good calls do get there
               dict(blocks=2, host_threads=1, _inject=("swap", 3 * 256 - 1, 0, 1))):
        with pytest.raises(AssertionError):
            hostsync.run(0, **kw)


def test_native_entry_points_validate_before_any_hip_call():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    out = (C.c_uint64 * 1024)()
    res = _native.HostsyncResult()
    inject = _native.HostsyncInject
    exp = lib.gm_probe_hostsync_expected
    assert exp(0, 2, 1, 3, 64, 0, out, 256) == 0 and exp(1, 2, 1, 3, 64, 0, out, 512) == 0
    assert exp(14, 1, 1, 2, 64, 0, out, 2 * 256 * 2 * 8) == 0
    for args in ((0, 2, 1, 3, 64, 0, out, 512), (2, 1, 0, 1, 1, 0, out, 8),
                 (12, 1, 0, 1, 1, 0, out, 4),
                 (0, 0, 1, 1, 1, 0, out, 4), (0, 1, 9, 1, 1, 0, out, 4), (0, 1, 0, 0, 1, 0, out, 4),
                 (0, 1, 0, 1, 3, 0, out, 12), (11, 9, 3, 3, 8, 0, out, 64),
                 (14, 1, 1, 2, 64, 0, out, 8), (0, 1, 0, 1, 1, 0, None, 4)):
        assert exp(*args) == 1, args
    w = C.c_uint32()
    assert lib.gm_probe_hostsync_cas_width(9, 3, 3, 1, C.byref(w)) == 0 and w.value == 16
    assert lib.gm_probe_hostsync_cas_width(9, 3, 3, 3, C.byref(w)) == 1
    assert lib.gm_probe_hostsync_supported(-1, None) == 1
    add, r = lib.gm_probe_hostsync_add, C.byref(res)
    for args in ((2, 1, 0, 1, 64), (0, 0, 0, 1, 64), (0, 1, 9, 1, 64), (0, 1, 0, 0, 64),
                 (0, 1, 0, 1, 48), (0, 4, 1, 1024, 64), (0, 1, 0, 1, 131072)):
        assert add(*args, 0, None, None, None, r) == 1, args
    assert add(0, 1, 0, 1, 64, 0, None, None, None, None) == 1
    for inj in (inject(1, 0, 256, 0, 0, 1), inject(1, 0, 0, 1, 0, 1), inject(1, 0, 0, 0, 0, 0),
                inject(1, 1, 0, 0, 0, 1), inject(4, 0, 0, 0, 0, 1)):
        assert add(0, 1, 0, 1, 64, 0, C.byref(inj), None, None, r) == 1
    assert lib.gm_probe_hostsync_ticket(1, 0, 1, 3, 0, None, None, r) == 1
    assert lib.gm_probe_hostsync_swap(1, 0, 1, 0, 0, None, None, r) == 1
    assert lib.gm_probe_hostsync_swap(1, 1, 1, 1, 0, C.byref(inject(4, 0, 512, 0, 0, 1)), None,
                                      r) == 1
    assert lib.gm_probe_hostsync_cas(9, 3, 3, 8, 0, None, None, None, r) == 1     # 1152 into a word
    assert lib.gm_probe_hostsync_cas(9, 3, 3, 4, 0, None, None, None, r) == 1     # 2304 into a word
    ho = lib.gm_probe_hostsync_handoff
    for args in ((0, 1, 1, 1, 1000, 5000), (1, 0, 1, 1, 1000, 5000), (1, 9, 1, 1, 1000, 5000),
                 (1, 1, 0, 1, 1000, 5000), (1, 1, 65, 1, 1000, 5000), (1, 1, 1, 2, 1000, 5000),
                 (1, 1, 1, 1, 0, 5000), (1, 1, 1, 1, 20001, 5000), (1, 1, 1, 1, 1000, 0),
                 (1, 1, 1, 1, 1000, 100001), (4096, 1, 64, 16, 1000, 5000)):
        assert ho(*args, 0, None, None, r) == 1, args
    bad = inject(16, 2, 0, 0, 0, 1)                                        # no such direction
    assert ho(1, 1, 1, 1, 1000, 5000, 0, C.byref(bad), None, r) == 1

    def run(mask=31, blocks=1, threads=1, iters=1, spread=1, rounds=1, lines=1, budget=1000,
            host_budget=5000, inj=None, out=res):
        return lib.gm_probe_hostsync(0, mask, blocks, threads, iters, spread, rounds, lines,
                                     budget, host_budget, 0,
                                     C.byref(inj) if inj is not None else None,
                                     C.byref(out) if out is not None else None)
    assert run(mask=0) == 1 and run(mask=32) == 1 and run(blocks=4097) == 1
    assert run(threads=9) == 1 and run(threads=0) == 1 and run(mask=16, threads=0) == 1
    assert run(iters=0) == 1 and run(iters=1025) == 1 and run(blocks=4, iters=1024) == 1
    assert run(spread=0) == 1 and run(spread=3) == 1 and run(spread=131072) == 1
    assert run(rounds=0) == 1 and run(rounds=65) == 1 and run(lines=4) == 1
    assert run(budget=0) == 1 and run(budget=20001) == 1 and run(host_budget=100001) == 1
    assert run(out=None) == 1 and run(blocks=4096, rounds=64, lines=16) == 1
    assert run(mask=1, inj=inject(2, 0, 0, 0, 0, 0)) == 1                  # a test that is not run
    assert run(inj=inject(3, 0, 0, 0, 0, 1)) == 1                          # not one test
    assert run(inj=inject(1, 2, 0, 0, 0, 1)) == 1 and run(inj=inject(4, 0, 512, 0, 0, 1)) == 1
    assert run(inj=inject(16, 0, 1, 0, 0, 1)) == 1 and run(inj=inject(16, 0, 0, 1, 0, 1)) == 1
    assert lib.gm_probe_hostsync(-1, 31, 1, 1, 1, 1, 1, 1, 1000, 5000, 0, None, C.byref(res)) == 1


def test_structs_mirror_the_header():
    """The sizes and offsets native/include/gm_probe.h pins with static_asserts."""
    assert C.sizeof(_native.HostsyncRecord) == 40 and C.sizeof(_native.HostsyncInject) == 24
    assert C.sizeof(_native.HostsyncDir) == 40
    R = _native.HostsyncResult
    assert C.sizeof(R) == 968
    assert [getattr(R, f).offset for f in (
        "words_in_error", "tickets", "swaps", "cas_giveups", "host_ops_in_flight", "lost_words",
        "dir", "rtt_median_us", "ms", "records_filled", "records", "seconds")] == [
        48, 80, 120, 152, 160, 168, 176, 256, 272, 312, 320, 960]
    assert _native.HostsyncRecord.test.offset == 24 and _native.HostsyncRecord.where.offset == 32
    assert _native.HostsyncDir.poll_max_us.offset == 32
    assert R.tests_skipped.offset == 4 and R.atomics_supported.offset == 8


def test_constants_mirror_the_header():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "native", "include", "gm_hostsync_ref.h")) as fh:
        text = fh.read()

    def macro(name):
        v = re.search(rf"#define GM_HOSTSYNC_{name} \(?([0-9a-fx]+)u?(?:ll)?(?: << (\d+))?", text)
        return int(v.group(1), 0) << int(v.group(2) or 0)
    for name in ("MAX_BLOCKS", "DEFAULT_BLOCKS", "MAX_HOST_THREADS", "DEFAULT_HOST_THREADS",
                 "MAX_ITERS", "DEFAULT_ITERS", "MAX_OPS", "DEFAULT_SPREAD", "MAX_ROUNDS",
                 "DEFAULT_ROUNDS", "DEFAULT_LINES", "MAX_BUDGET_US", "DEFAULT_BUDGET_US",
                 "MAX_HOST_BUDGET_US", "DEFAULT_HOST_BUDGET_US", "MAX_MAILBOX_BYTES"):
        assert getattr(hostsync, name) == macro(name), name
    assert hostsync.TESTS == {"add": 1, "ticket": 2, "swap": 4, "cas": 8, "handoff": 16}
    assert hostsync.DEFAULT_BUDGET_US >= 1000 and hostsync.DEFAULT_HOST_BUDGET_US >= 5000


class FakeLib:
    """gm_probe_hostsync answering from `script`; records what it was called with."""

    def __init__(self, **script):
        self.script, self.seen = script, {}

    def gm_probe_hostsync(self, dev, mask, blocks, threads, iters, spread, rounds, lines, budget,
                          host_budget, seed, inj, out):
        res, s = out._obj, self.script
        self.seen.update(mask=mask, blocks=blocks, threads=threads, budget=budget,
                         host_budget=host_budget, inj=inj)
        supported = s.get("supported", 1)
        res.atomics_supported = supported
        res.tests_skipped = 0 if supported else mask & 15
        res.tests_run = mask if supported else mask & 16
        res.blocks, res.host_threads, res.iters, res.spread = 16, threads, iters, spread
        res.rounds, res.lines = rounds, lines
        res.budget_us, res.host_budget_us = budget, host_budget
        res.cas_width, res.seconds = 4096, 0.03
        if res.tests_run & 15:
            res.tickets = res.swaps = 18 * 256 * iters
            res.host_ops_in_flight = 1234
            res.ms[0], res.ms[2] = 4.0, 2.0
        if res.tests_run & 16:
            for d, seen_ in enumerate(s.get("observed", (128, 128))):
                res.dir[d].handoffs, res.dir[d].observed = 128, seen_
                res.dir[d].unseen, res.dir[d].poll_max_us = 128 - seen_, 30.0 + d
            res.rtt_median_us, res.rtt_max_us, res.ms[4] = 130.0, 160.0, 2.5
        if s.get("stale"):
            res.dir[1].stale_words, res.lost_words, res.records_filled = 1, 1, 2
            for i, where in enumerate((1, 2)):
                rec = res.records[i]
                rec.test, rec.kind, rec.where = 16, 1, where
                rec.index, rec.expected, rec.got = 1 << 20 | 2 << 14 | 1500, 5, 4
        return 0


def test_run_decodes_the_native_result(monkeypatch):
    """ok is about data only; unseen and skipped tests never change it."""
    lib = FakeLib()
    monkeypatch.setattr(_native, "probe", lambda: lib)
    r = hostsync.run(0)
    assert lib.seen["mask"] == 31 and lib.seen["blocks"] == 0 and lib.seen["threads"] == 2
    assert (lib.seen["budget"], lib.seen["host_budget"]) == (
        hostsync.DEFAULT_BUDGET_US, hostsync.DEFAULT_HOST_BUDGET_US) and lib.seen["inj"] is None
    h2d = {"handoffs": 128, "observed": 128, "unseen": 0, "stale_words": 0, "poll_max_us": 30.0}
    assert r == {
        "device": 0, "tests": list(hostsync.ALL_TESTS), "tests_skipped": {},
        "atomics_supported": True, "blocks": 16, "host_threads": 2, "iters": 4, "spread": 4096,
        "rounds": 8, "lines": 16, "budget_us": hostsync.DEFAULT_BUDGET_US,
        "host_budget_us": hostsync.DEFAULT_HOST_BUDGET_US, "cas_width": 4096,
        "words_in_error": 0, "add_u32_errors": 0, "add_u64_errors": 0, "cas_errors": 0,
        "tickets": 18432, "holes": 0, "duplicates": 0, "counter_errors": 0, "out_of_range": 0,
        "swaps": 18432, "swap_missing": 0, "swap_duplicates": 0, "swap_foreign": 0,
        "cas_giveups": 0, "host_ops_in_flight": 1234,
        "ms": {"add": 4.0, "ticket": 0.0, "swap": 2.0, "cas": 0.0, "handoff": 2.5},
        "seconds": 0.03, "h2d": h2d, "d2h": dict(h2d, poll_max_us=31.0), "stale_words_h2d": 0,
        "stale_words_d2h": 0, "lost_words": 0, "rtt_median_us": 130.0, "rtt_max_us": 160.0,
        "first_errors": [], "handoff_vacuous": False, "ok": True}
    assert hostsync.describe_failed(r) == ""

    lib.script.update(observed=(100, 0))                # the host saw no reply in time
    r = hostsync.run(0)
    assert r["ok"] and r["handoff_vacuous"] and r["d2h"]["unseen"] == 128
    assert r["h2d"]["unseen"] == 28
    r = hostsync.run(0, tests=("add", "swap"), host_threads=0)
    assert r["ok"] and not r["handoff_vacuous"] and lib.seen["mask"] == 5     # it did not run
    assert r["tests"] == ["add", "swap"] and list(r["ms"]) == ["add", "swap"]

    lib.script.update(observed=(128, 128), supported=0)  # no native atomics over this link
    r = hostsync.run(0)
    assert r["ok"] and not r["atomics_supported"] and r["tests"] == ["handoff"]
    assert r["tests_skipped"] == {t: hostsync.NO_ATOMICS for t in hostsync.ATOMIC_TESTS}
    assert r["tickets"] == 0 and not r["handoff_vacuous"] and list(r["ms"]) == ["handoff"]

    lib.script.update(supported=1, stale=True)
    r = hostsync.run(0, _inject=("handoff", "d2h", 1, 2, 1500, 1))
    assert not r["ok"] and lib.seen["inj"] is not None
    assert (r["stale_words_d2h"], r["stale_words_h2d"], r["lost_words"]) == (1, 0, 1)
    rec = {"test": "handoff", "index": 1 << 20 | 2 << 14 | 1500, "expected": "0x5", "got": "0x4",
           "xor": "0x1", "direction": "d2h", "block": 1, "round": 2, "word": 1500}
    assert r["first_errors"] == [dict(rec, found="consumer"), dict(rec, found="audit")]
    assert hostsync.describe_failed(r) == (
        "stale_words_d2h 1; lost_words 1; first: handoff d2h block 1 round 2 word 1500 "
        "(by the consumer) expected 0x5 got 0x4")


def _result(**over):
    """A clean :func:`hostsync.run` result, as the stubs return it."""
    d = {"handoffs": 128, "observed": 128, "unseen": 0, "stale_words": 0, "poll_max_us": 30.0}
    r = {"device": 0, "tests": list(hostsync.ALL_TESTS), "tests_skipped": {},
         "atomics_supported": True, "blocks": 16, "host_threads": 2, "iters": 4, "spread": 4096,
         "rounds": 8, "lines": 16, "budget_us": 1000, "host_budget_us": 5000, "cas_width": 4096,
         "add_u32_errors": 0, "add_u64_errors": 0, "cas_errors": 0, "tickets": 18432,
         "swaps": 18432, "host_ops_in_flight": 1234, "ms": {}, "seconds": 0.033, "h2d": dict(d),
         "d2h": dict(d), "rtt_median_us": 130.0, "rtt_max_us": 160.0, "first_errors": [],
         "handoff_vacuous": False, "ok": True}
    r.update({c: 0 for c in hostsync.ERROR_COUNTERS})
    r.update(over)
    return r


SWAP_BAD = dict(ok=False, swap_missing=1, swap_foreign=1, first_errors=[
    {"test": "swap", "index": 494, "expected": "0x0", "got": "0x4b013", "xor": "0x4b013"}])


def test_doctor_wiring_ok_warn_and_fail(monkeypatch):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    for fn in (doctor.check_gpus, doctor.run):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-2:] == ["host_sync", "host_sync_inject"]        # at the end
        assert sig["host_sync"].default is False and sig["host_sync_inject"].default is None
        for name in ("host_sync", "host_sync_inject"):
            assert sig[name].kind is sig[name].KEYWORD_ONLY
    calls, answer = [], {}

    def fake_run(dev, _inject=None):
        calls.append((dev, _inject))
        return _result(**(SWAP_BAD if _inject else answer))
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(hostsync, "run", fake_run)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "host-sync" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, host_sync=True) if c.name == "gpu0"]
    assert ok.status == "ok"
    assert "host-sync add+ticket+swap+cas+handoff 16 blocks and 2 host threads" in ok.detail
    assert "hand-offs 128/128 seen by the GPU 128/128 by the host" in ok.detail
    answer.update(handoff_vacuous=True, d2h={"handoffs": 128, "observed": 0, "unseen": 128,
                                             "stale_words": 0, "poll_max_us": 0.0})
    (vac,) = [c for c in doctor.check_gpus(cfg, host_sync=True) if c.name == "gpu0"]
    assert vac.status == "warn" and "proved nothing there" in vac.detail
    assert "128/128 seen by the GPU 0/128 by the host" in vac.detail
    answer.clear()
    answer.update(atomics_supported=False, tests=["handoff"],
                  tests_skipped={t: hostsync.NO_ATOMICS for t in hostsync.ATOMIC_TESTS})
    (skipped,) = [c for c in doctor.check_gpus(cfg, host_sync=True) if c.name == "gpu0"]
    assert skipped.status == "warn"
    assert f"skipped add+ticket+swap+cas: {hostsync.NO_ATOMICS}" in skipped.detail
    inj = ("swap", 300, 2, 0x10)
    (bad,) = [c for c in doctor.check_gpus(cfg, host_sync=True, host_sync_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail" and ("failed: swap_missing 1; swap_foreign 1; first: swap index "
                                     "494 expected 0x0 got 0x4b013") in bad.detail
    assert calls == [(0, None), (0, None), (0, None), (0, inj)]

    # run() forwards the two keywords only when set
    got = []
    monkeypatch.setattr(doctor, "check_gpus", lambda cfg, burn, **kw: got.append(kw) or [])
    for name in ("check_inventory", "check_cgroup", "check_devnodes", "check_pidns",
                 "check_systemd"):
        monkeypatch.setattr(doctor, name, lambda cfg: [])
    doctor.run(cfg, skip_cluster=True, gpu=True)
    doctor.run(cfg, skip_cluster=True, gpu=True, host_sync=True)
    doctor.run(cfg, skip_cluster=True, gpu=True, host_sync=True, host_sync_inject=inj)
    doctor.run(cfg, skip_cluster=True, gpu=True, host_sync_inject=inj)     # not asked for
    assert got == [{"memtest_bytes": 0}, {"memtest_bytes": 0, "host_sync": True},
                   {"memtest_bytes": 0, "host_sync": True, "host_sync_inject": inj},
                   {"memtest_bytes": 0}]


def test_command_lines_parse_the_host_sync_options():
    from gpumounter_amd.cli import build_parser, cmd_doctor, cmd_probe

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.host_sync is False and a.host_sync_inject is None and a.host_sync_tests is None
    assert a.host_sync_threads is None
    a = ap.parse_args(["probe", "--host-sync", "--host-sync-tests", "swap,handoff",
                       "--host-sync-blocks", "9", "--host-sync-threads", "3",
                       "--host-sync-rounds", "3", "--host-sync-inject",
                       "handoff:d2h:3:2:1500:0x100"])
    assert a.host_sync and a.host_sync_tests == ("swap", "handoff") and a.host_sync_blocks == 9
    assert a.host_sync_threads == 3 and a.host_sync_rounds == 3
    assert a.host_sync_inject == ("handoff", "d2h", 3, 2, 1500, 256)
    for bad in (["--host-sync-tests", "add,sub"], ["--host-sync-inject", "ticket:0"],
                ["--host-sync-blocks", "x"], ["--host-sync-inject", "swap:0:0:0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--host-sync", *bad])
    # usage errors (2), not a failed test (1), before any GPU work
    for argv in (["--host-sync-inject", "ticket:0:0"], ["--host-sync-tests", "add"],
                 ["--host-sync-blocks", "4"], ["--host-sync-threads", "2"],
                 ["--host-sync-rounds", "2"], ["--host-sync", "--host-sync-blocks", "0"],
                 ["--host-sync", "--host-sync-blocks", "4097"],
                 ["--host-sync", "--host-sync-threads", "9"],
                 ["--host-sync", "--host-sync-threads", "0"],           # the hand-off needs one
                 ["--host-sync", "--host-sync-rounds", "65"],
                 ["--host-sync", "--host-sync-tests", "add", "--host-sync-inject",
                  "ticket:0:0"]):
        assert cmd_probe(ap.parse_args(["probe", *argv])) == 2, argv
    assert ap.parse_args(["doctor", "--gpu", "--host-sync"]).host_sync is True
    assert ap.parse_args(["doctor", "--gpu"]).host_sync is False
    assert cmd_doctor(ap.parse_args(["doctor", "--host-sync-inject", "ticket:0:0"])) == 2
    import gpumounter_amd.cli as cli
    for line in ("[--host-sync]", "--host-sync-threads N", "swap:G:S:MASK",
                 "handoff:DIR:BLOCK:ROUND:WORD:MASK", "[--gpu --host-sync]"):
        assert line in cli.__doc__, line


def test_probe_and_validate_wiring(monkeypatch, capsys):
    from gpumounter_amd import cli
    from gpumounter_amd.ops import probe
    from gpumounter_amd.parallel import validate

    calls = []

    def fake_run(dev, tests=hostsync.ALL_TESTS, blocks=0,
                 host_threads=hostsync.DEFAULT_HOST_THREADS, rounds=hostsync.DEFAULT_ROUNDS,
                 _inject=None):
        calls.append((dev, tuple(tests), blocks, host_threads, rounds, _inject))
        return _result(**(SWAP_BAD if _inject else {}))

    class Verified:
        def to_dict(self):
            return {"device": 0, "ok": True}
    monkeypatch.setattr(hostsync, "run", fake_run)
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Verified()])
    ap = cli.build_parser()
    assert cli.cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--host-sync"])) == 0
    assert json.loads(capsys.readouterr().out)[0]["hostsync"]["ok"] is True
    assert cli.cmd_probe(ap.parse_args(
        ["probe", "--bdf", "0000:05:00.0", "--host-sync", "--host-sync-tests", "add,swap",
         "--host-sync-blocks", "9", "--host-sync-threads", "0", "--host-sync-rounds", "3",
         "--host-sync-inject", "swap:300:2:0x10"])) == 1
    assert json.loads(capsys.readouterr().out)[0]["hostsync"]["swap_foreign"] == 1
    assert cli.cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0"])) == 0
    assert "hostsync" not in json.loads(capsys.readouterr().out)[0]
    assert calls == [(0, hostsync.ALL_TESTS, 0, 2, 8, None),
                     (0, ("add", "swap"), 9, 0, 3, ("swap", 300, 2, 16))]

    # doctor's command line forwards exactly what was given
    from gpumounter_amd.utils import doctor
    seen = []
    monkeypatch.setattr(doctor, "run", lambda cfg, **kw: seen.append(kw) or [
        doctor.Check("gpu0", "ok", "fine")])
    assert cli.cmd_doctor(ap.parse_args(["doctor", "--skip-cluster", "--host-sync",
                                         "--host-sync-inject", "swap:300:2:0x10"])) == 0
    capsys.readouterr()
    assert seen[0]["gpu"] is True and seen[0]["host_sync"] is True
    assert seen[0]["host_sync_inject"] == ("swap", 300, 2, 16)

    del calls[:]
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2 * numel}])
    assert validate.main(["--host-sync"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert rep["ok"] and rep["hostsync"][0]["ok"]
    assert validate.main(["--host-sync", "--host-sync-inject", "ticket:300:2"]) == 1
    assert json.loads(capsys.readouterr().out)["ok"] is False
    assert validate.main([]) == 0 and "hostsync" not in json.loads(capsys.readouterr().out)
    assert [c[5] for c in calls] == [None, ("ticket", 300, 2)]
    with pytest.raises(SystemExit):
        validate.main(["--host-sync-inject", "ticket:300:2"])
    with pytest.raises(SystemExit):
        validate.main(["--host-sync", "--host-sync-inject", "ticket:300"])
    assert "--host-sync" in validate.__doc__
