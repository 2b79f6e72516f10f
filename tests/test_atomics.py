"""The cross-XCC atomics test without a GPU: the host reference (gm_probe_atomics_expected)
against an independent numpy fold for every kind, the width rule and every cap refusal, the
parsers, the structs, the command lines, and the doctor / validate / probe wiring against a
stubbed native call."""
import ctypes as C
import inspect
import json

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import atomics
from gpumounter_amd.ops.probe import ProbeError

SEED = 0x0123456789ABCDEF
SHAPES = ((1, 1, 1), (2, 3, 64), (9, 3, 1), (9, 2, 4096))
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


def bf16_of_int(n):
    """bf16 bit pattern of a small non-negative integer (<= 256: exact)."""
    return (np.asarray(n, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint32)


def numpy_fold(kind, blocks, iters, width, seed):
    """The final table by np.ufunc.at in (g, s) order: nothing shared with the C fold but the
    formulas of gm_probe.h."""
    k = atomics.KINDS.index(kind) if kind != "count" else 13
    T = blocks * 256
    g, s = np.meshgrid(np.arange(T, dtype=np.uint64), np.arange(iters, dtype=np.uint64),
                       indexing="ij")
    g, s = g.ravel(), s.ravel()
    idx = g * np.uint64(1024) + s
    h = H(seed, 0x100 + k, idx)
    hi = H(seed, 0x120 + k, idx)
    w = ((g + np.uint64(97) * s) % np.uint64(width)).astype(np.int64)
    op64 = (hi << np.uint64(32)) | h
    bit = np.where((h >> np.uint64(5)) & np.uint64(7) == 0, np.uint64(1) << (h & np.uint64(31)),
                   np.uint64(0))
    small = (h % np.uint64(9)).astype(np.int64) - 4
    if kind == "count":
        return np.bincount(w, minlength=width).astype(np.uint32)
    if kind == "add_u32":
        t = np.zeros(width, np.uint64)
        np.add.at(t, w, h)
        return (t & M32).astype(np.uint32)
    if kind in ("add_u64", "cas"):
        t = np.zeros(width, np.uint64)
        np.add.at(t, w, op64)                      # wraps modulo 2^64
        return t
    if kind == "xor_u64":
        t = np.zeros(width, np.uint64)
        np.bitwise_xor.at(t, w, op64)
        return t
    if kind == "umax_u32":
        t = np.zeros(width, np.uint64)
        np.maximum.at(t, w, h)
        return t.astype(np.uint32)
    if kind == "umin_u32":
        t = np.full(width, 0xFFFFFFFF, np.uint64)
        np.minimum.at(t, w, h)
        return t.astype(np.uint32)
    if kind == "and_u32":
        t = np.full(width, 0xFFFFFFFF, np.uint64)
        np.bitwise_and.at(t, w, ~bit & M32)
        return t.astype(np.uint32)
    if kind == "or_u32":
        t = np.zeros(width, np.uint64)
        np.bitwise_or.at(t, w, bit)
        return t.astype(np.uint32)
    if kind in ("add_f32", "add_f64"):
        t = np.zeros(width, np.int64)
        np.add.at(t, w, small)
        return (t.astype(np.float32).view(np.uint32) if kind == "add_f32"
                else t.astype(np.float64).view(np.uint64))
    if kind == "pk_add_bf16":
        lo, up = np.zeros(width, np.int64), np.zeros(width, np.int64)
        np.add.at(lo, w, (h & np.uint64(1)).astype(np.int64))
        np.add.at(up, w, ((h >> np.uint64(1)) & np.uint64(1)).astype(np.int64))
        assert lo.max() <= 128 and up.max() <= 128
        return bf16_of_int(lo) | (bf16_of_int(up) << 16)
    if kind == "ticket":
        t = np.zeros(width, np.uint64)
        np.add.at(t, w, np.uint64(1) + (h & np.uint64(3)))
        return t.astype(np.uint32)
    raise AssertionError(kind)


@pytest.mark.parametrize("blocks,iters,spread", SHAPES)
@pytest.mark.parametrize("kind", atomics.KINDS[:12] + ("count",))
def test_expected_equals_the_numpy_fold(kind, blocks, iters, spread):
    got = atomics.expected(kind, blocks, iters, spread, SEED)
    width = spread if kind == "count" else atomics.widths(blocks, iters, spread)[kind]["width"]
    assert got.shape == (width,)
    assert got.dtype == (np.uint64 if kind in atomics.WIDE else np.uint32)
    np.testing.assert_array_equal(got, numpy_fold(kind, blocks, iters, width, SEED))


def test_expected_depends_on_seed_and_kind_and_takes_the_index():
    a = atomics.expected("add_u32", 2, 3, 64, SEED)
    assert (a != atomics.expected("add_u32", 2, 3, 64, SEED + 1)).any()
    assert (a != atomics.expected("umax_u32", 2, 3, 64, SEED)).any()
    np.testing.assert_array_equal(a, atomics.expected(0, 2, 3, 64, SEED))
    # and / or do not saturate after a handful of operations: 108 per word at (9, 3, 64)
    assert (atomics.expected("or_u32", 9, 3, 64) != 0xFFFFFFFF).all()
    assert (atomics.expected("and_u32", 9, 3, 64) != 0).all()


def test_width_rule():
    w = atomics.widths(9, 3, 1)
    # 9 * 256 * 3 = 6912 adds, 128 at most into a bf16 word: at least 54 words, so 64
    assert w["pk_add_bf16"] == {"width": 64, "cap": 128, "max_adds": 108}
    assert w["add_f32"] == {"width": 1, "cap": (1 << 22) - 1, "max_adds": 6912}
    assert w["add_f64"]["width"] == 1 and w["add_u32"] == {"width": 1, "cap": 0, "max_adds": 6912}
    assert w["ticket"]["width"] == 1 and w["handoff"]["width"] == 0
    # a CAS loop's retries grow with the square of the operations into a word: 1024 at most
    assert w["cas"] == {"width": 8, "cap": 1024, "max_adds": 864}
    assert atomics.widths(1, 1, 1)["pk_add_bf16"]["width"] == 2
    assert atomics.widths(9, 2, 4096)["pk_add_bf16"] == {"width": 4096, "cap": 128, "max_adds": 2}
    # 2^26 adds into one word would break 4 * adds < 2^24: 32 words of 2^21 adds each
    big = atomics.widths(4096, 64, 1)
    assert big["add_f32"]["width"] == 32 and big["add_f64"]["max_adds"] == 1 << 21
    assert big["pk_add_bf16"]["width"] == (1 << 26) // 128
    # the busiest word is counted: 3 blocks do not divide over 512 words evenly
    assert atomics.widths(3, 5, 512)["add_u32"]["max_adds"] == int(
        numpy_fold("count", 3, 5, 512, 0).max())


def test_every_cap_refusal():
    for call in (
            lambda: atomics.expected("pk_add_bf16", 9, 3, width=32),     # 216 adds into a word
            lambda: atomics.expected("add_f32", 4096, 64, width=16),     # 2^22 adds
            lambda: atomics.expected("add_f64", 4096, 64, width=16),
            lambda: atomics.expected("cas", 9, 3, width=4),              # 1728 into a word
            lambda: atomics.expected("add_u32", 1, 1, width=96),         # no power of two
            lambda: atomics.expected("add_u32", 1, 1, width=atomics.MAX_WIDTH * 2),
            lambda: atomics.expected("add_u32", 4096, 65, 1),            # T * iters > 2^26
            lambda: atomics.expected("add_u32", 0, 1, 1),
            lambda: atomics.expected("add_u32", 4097, 1, 1),
            lambda: atomics.expected("add_u32", 1, 0, 1),
            lambda: atomics.expected("add_u32", 1, 1025, 1),
            lambda: atomics.expected("add_u32", 1, 1, 3),
            lambda: atomics.expected("add_u32", 1, 1, 131072),
            lambda: atomics.expected("handoff", 1, 1, 1),
            lambda: atomics.expected("add_f16", 1, 1, 1),
            lambda: atomics.expected("add_u32", 1, 1, 1, seed=-1),
            lambda: atomics.widths(1, 1, 48), lambda: atomics.widths(4096, 65, 1)):
        with pytest.raises(ProbeError):
            call()
    assert "more than 128 operations" in str(pytest.raises(
        ProbeError, atomics.expected, "pk_add_bf16", 9, 3, width=32).value)
    atomics.expected("pk_add_bf16", 9, 3, width=64)                      # the cap itself is kept
    atomics.expected("add_f32", 4096, 64, width=32)


def test_native_entry_points_validate_before_any_hip_call():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    out = (C.c_uint64 * 64)()
    P = C.c_void_p(1 << 20)               # never dereferenced: every call is refused first
    res = _native.AtomicsResult()
    inject = _native.AtomicsInject
    exp = lib.gm_probe_atomics_expected
    assert exp(0, 2, 3, 64, 0, out, 256) == 0 and exp(1, 2, 3, 64, 0, out, 512) == 0
    for args in ((0, 2, 3, 64, 0, out, 512), (1, 2, 3, 64, 0, out, 256), (12, 1, 1, 1, 0, out, 4),
                 (14, 1, 1, 1, 0, out, 4), (0, 0, 1, 1, 0, out, 4), (0, 1, 0, 1, 0, out, 4),
                 (0, 1, 1, 3, 0, out, 12), (9, 9, 3, 32, 0, out, 128), (0, 1, 1, 1, 0, None, 4)):
        assert exp(*args) == 1, args
    assert lib.gm_probe_atomics_widths(1, 1, 3, None, None, None) == 1
    assert lib.gm_probe_atomics_widths(1, 1, 4, None, None, None) == 0
    add = lib.gm_probe_atomics_add
    for args in ((10, P, 64, 1, 1, 0, None, None), (0, None, 64, 1, 1, 0, None, None),
                 (1, C.c_void_p((1 << 20) + 4), 64, 1, 1, 0, None, None),
                 (0, P, 48, 1, 1, 0, None, None), (9, P, 32, 9, 3, 0, None, None),
                 (0, P, 64, 0, 1, 0, None, None), (0, P, 64, 1, 0, 0, None, None)):
        assert add(*args) == 1, args
    for inj in (inject(1, 0, 256, 0, 0, 1), inject(1, 0, 0, 1, 0, 1), inject(1, 0, 0, 0, 0, 0),
                inject(1, 3, 0, 0, 0, 1), inject(4, 0, 0, 0, 0, 1)):
        assert add(0, P, 64, 1, 1, 0, C.byref(inj), None) == 1
    assert lib.gm_probe_atomics_cas(P, P, 48, 1, 1, 0, None, None, C.byref(res)) == 1
    assert lib.gm_probe_atomics_cas(P, P, 4, 9, 3, 0, None, None, C.byref(res)) == 1
    assert lib.gm_probe_atomics_cas(P, None, 64, 1, 1, 0, None, None, C.byref(res)) == 1
    assert lib.gm_probe_atomics_cas(P, P, 64, 1, 1, 0, None, None, None) == 1
    tk = lib.gm_probe_atomics_ticket
    assert tk(P, P, P, 255, 1, 1, 1, 0, None, None, C.byref(res)) == 1     # fewer marks than draws
    assert tk(P, P, P, 1025, 1, 1, 1, 0, None, None, C.byref(res)) == 1    # more than 4 per draw
    assert tk(P, P, P, 600, 3, 1, 1, 0, None, None, C.byref(res)) == 1
    assert tk(P, None, P, 600, 1, 1, 1, 0, None, None, C.byref(res)) == 1
    ho = lib.gm_probe_atomics_handoff
    for args in ((P, P, 0, 1, 1, 200), (P, P, 1, 0, 1, 200), (P, P, 1, 65, 1, 200),
                 (P, P, 1, 1, 2, 200), (P, P, 1, 1, 1, 0), (P, P, 1, 1, 1, 1001),
                 (P, P, 4096, 64, 16, 200),                                # 16 GiB of mailboxes
                 (None, P, 1, 1, 1, 200), (C.c_void_p((1 << 20) + 8), P, 1, 1, 1, 200),
                 (P, C.c_void_p((1 << 20) + 64), 1, 1, 1, 200)):
        assert ho(*args, 0, None, None, C.byref(res)) == 1, args
    bad = inject(8, 0, 0, 0, 1024, 1)                                      # word outside 1 line
    assert ho(P, P, 1, 1, 1, 200, 0, C.byref(bad), None, C.byref(res)) == 1

    def run(mask=15, blocks=1, iters=1, spread=1, rounds=1, lines=1, budget=200, inj=None,
            out=res):
        return lib.gm_probe_atomics(0, mask, blocks, iters, spread, rounds, lines, budget, 0,
                                    C.byref(inj) if inj is not None else None,
                                    C.byref(out) if out is not None else None)
    assert run(mask=0) == 1 and run(mask=16) == 1 and run(blocks=4097) == 1
    assert run(iters=0) == 1 and run(iters=1025) == 1 and run(blocks=4096, iters=65) == 1
    assert run(spread=0) == 1 and run(spread=3) == 1 and run(spread=131072) == 1
    assert run(rounds=0) == 1 and run(rounds=65) == 1 and run(lines=4) == 1
    assert run(budget=0) == 1 and run(budget=1001) == 1 and run(out=None) == 1
    assert run(blocks=4096, rounds=64, lines=16) == 1
    assert run(mask=1, inj=inject(2, 0, 0, 0, 0, 0)) == 1                  # a test that is not run
    assert run(inj=inject(3, 0, 0, 0, 0, 1)) == 1                          # not one test
    assert run(inj=inject(1, 10, 0, 0, 0, 1)) == 1 and run(inj=inject(2, 0, 256, 0, 0, 0)) == 1
    assert run(inj=inject(8, 0, 1, 0, 0, 1)) == 1 and run(inj=inject(8, 0, 0, 1, 0, 1)) == 1
    assert lib.gm_probe_atomics(-1, 15, 1, 1, 1, 1, 1, 200, 0, None, C.byref(res)) == 1


def test_python_validates_before_the_native_call(monkeypatch):
    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    for kw in (dict(tests=()), dict(tests=("add", "sub")), dict(tests=16), dict(blocks=-1),
               dict(blocks=4097), dict(blocks=True), dict(iters=0), dict(iters=1025),
               dict(blocks=4096, iters=65), dict(spread=0), dict(spread=48),
               dict(spread=131072), dict(rounds=0), dict(rounds=65), dict(lines=2),
               dict(budget_us=0), dict(budget_us=1001), dict(seed=-1), dict(seed=1 << 64),
               dict(blocks=4096, rounds=64), dict(_inject=("add", "cas", 0, 0, 1)),
               dict(_inject=("add", "add_u32", 0, 0, 0)), dict(_inject=("cas", 0, 0)),
               dict(_inject=("ticket", -1, 0)), dict(_inject=("handoff", 0, 64, 0, 1)),
               dict(_inject=("handoff", 0, 0, 16384, 1)), dict(_inject=("sub", 0, 0)),
               dict(tests=("add",), _inject=("ticket", 0, 0))):
        with pytest.raises(ProbeError):
            atomics.run(0, **kw)
    with pytest.raises(ProbeError):
        atomics.run(-1)
    with pytest.raises(AssertionError):                  # a good call does get there
        atomics.run(0)


def test_parsers():
    assert atomics.parse_tests("add,ticket, cas,handoff") == atomics.ALL_TESTS
    assert atomics.parse_tests("handoff") == ("handoff",)
    assert atomics.mask_of(("add", 8)) == 9 and atomics.mask_of("cas") == 4
    assert atomics.parse_spread("64") == 64 and atomics.parse_spread("0x1000") == 4096
    assert atomics.parse_inject("add:add_f32:300:2:0x1") == ("add", "add_f32", 300, 2, 1)
    assert atomics.parse_inject("add:pk_add_bf16:0:0:7") == ("add", "pk_add_bf16", 0, 0, 7)
    assert atomics.parse_inject("cas:300:2:0x10") == ("cas", 300, 2, 16)
    assert atomics.parse_inject("ticket:300:2") == ("ticket", 300, 2)
    assert atomics.parse_inject("handoff:3:2:1500:0x100") == ("handoff", 3, 2, 1500, 256)
    for bad in ("", "add", "sub:1:2", "add:add_u32:0:0", "add:cas:0:0:1", "add:9:0:0:1", "add:add_u32:0:0:0",
                "cas:0:0:x", "ticket:0", "ticket:0:0:1", "handoff:0:0:0", "handoff:0:64:0:1",
                "handoff:4096:0:0:1", "cas:0:1024:1"):
        with pytest.raises(ProbeError):
            atomics.parse_inject(bad)
    for bad in ("", "add,sub", ","):
        with pytest.raises(ProbeError):
            atomics.parse_tests(bad)
    for bad in ("0", "3", "131072", "x"):
        with pytest.raises(ProbeError):
            atomics.parse_spread(bad)
    inj = atomics._inject_arg(("handoff", 3, 2, 1500, 0x100))
    assert (inj.test, inj.kind, inj.a, inj.b, inj.word, inj.mask) == (8, 12, 3, 2, 1500, 256)
    inj = atomics._inject_arg(("add", "add_f64", 5, 1, 3))
    assert (inj.test, inj.kind, inj.a, inj.b, inj.word, inj.mask) == (1, 8, 5, 1, 0, 3)


def test_payload_and_partner_formulas():
    for b, r, word in ((0, 0, 0), (3, 2, 1500), (4095, 63, 16383)):
        assert atomics.payload(b, r, word, SEED) == int(H(SEED, 0x10C, b << 20 | r << 14 | word))


def test_structs_mirror_the_header():
    """The sizes and offsets native/include/gm_probe.h pins with static_asserts."""
    assert C.sizeof(_native.AtomicsKind) == 40 and C.sizeof(_native.AtomicsRecord) == 40
    assert C.sizeof(_native.AtomicsInject) == 24
    R = _native.AtomicsResult
    assert C.sizeof(R) == 3448
    assert [getattr(R, f).offset for f in (
        "kinds", "words_in_error", "tickets", "cas_giveups", "handoffs", "poll_max_us",
        "pairs_observed", "pairs_stale", "xcc_blocks", "records_filled", "records", "seconds")] == [
        32, 552, 560, 608, 616, 664, 680, 1704, 2728, 2792, 2800, 3440]
    assert _native.AtomicsRecord.test.offset == 24 and _native.AtomicsKind.width.offset == 32
    assert len(atomics.KINDS) == _native.ATOMICS_KINDS


def test_command_lines_parse_the_atomics_options():
    from gpumounter_amd.cli import build_parser, cmd_doctor, cmd_probe

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.atomics is False and a.atomics_inject is None and a.atomics_tests is None
    a = ap.parse_args(["probe", "--atomics", "--atomics-tests", "add,handoff", "--atomics-spread",
                       "64", "--atomics-blocks", "9", "--atomics-rounds", "3",
                       "--atomics-inject", "handoff:3:2:1500:0x100"])
    assert a.atomics and a.atomics_tests == ("add", "handoff") and a.atomics_spread == 64
    assert a.atomics_blocks == 9 and a.atomics_rounds == 3
    assert a.atomics_inject == ("handoff", 3, 2, 1500, 256)
    for bad in (["--atomics-tests", "add,sub"], ["--atomics-spread", "48"],
                ["--atomics-inject", "ticket:0"], ["--atomics-blocks", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--atomics", *bad])
    # usage errors (2), not a failed test (1), before any GPU work
    for argv in (["--atomics-inject", "ticket:0:0"], ["--atomics-spread", "64"],
                 ["--atomics-tests", "add"], ["--atomics-blocks", "4"], ["--atomics-rounds", "2"],
                 ["--atomics", "--atomics-blocks", "0"], ["--atomics", "--atomics-blocks", "4097"],
                 ["--atomics", "--atomics-rounds", "65"],
                 ["--atomics", "--atomics-tests", "add", "--atomics-inject", "ticket:0:0"]):
        assert cmd_probe(ap.parse_args(["probe", *argv])) == 2, argv
    assert ap.parse_args(["doctor", "--gpu", "--atomics"]).atomics is True
    assert ap.parse_args(["doctor", "--gpu"]).atomics is False
    assert cmd_doctor(ap.parse_args(["doctor", "--atomics-inject", "ticket:0:0"])) == 2


def _result(**over):
    """A clean :func:`atomics.run` result, as the stubs return it."""
    r = {"device": 0, "tests": list(atomics.ALL_TESTS), "blocks": 256, "iters": 8,
         "spread": 4096, "rounds": 8, "lines": 16, "budget_us": 200, "xccs_seen": 8,
         "xcc_blocks": [32] * 8 + [0] * 8,
         "kinds": {"add_f32": {"ops": 1, "ms": 1.0, "gops": 1.0, "width": 4096,
                               "words_in_error": 0}},
         "tickets": 524288, "seconds": 0.013, "handoffs": 2048, "observed": 2048,
         "observed_cross_xcc": 1792, "unseen": 0, "poll_max_us": 10.0, "poll_mean_us": 0.5,
         "pairs_observed": [[0] * 16] * 16, "pairs_stale": [[0] * 16] * 16, "first_errors": [],
         "handoff_vacuous": False, "ok": True}
    r.update({c: 0 for c in atomics.ERROR_COUNTERS})
    r.update(over)
    return r


STALE = dict(ok=False, stale_words=1, lost_words=1, first_errors=[
    {"test": "handoff", "kind": "handoff", "index": 427484, "expected": "0x3ebfef9f",
     "got": "0x3ebfee9f", "xor": "0x100", "mailbox": 26, "word": 1500, "xcc_producer": 3,
     "xcc_consumer": 0}])


def test_describe_failed():
    assert atomics.describe_failed(_result()) == ""
    assert atomics.describe_failed(_result(**STALE)) == (
        "stale_words 1; lost_words 1; first: handoff mailbox 26 word 1500 expected 0x3ebfef9f "
        "got 0x3ebfee9f producer xcc 3 consumer xcc 0")
    bad = _result(ok=False, words_in_error=2, first_errors=[
        {"test": "add", "kind": "add_f32", "index": 494, "expected": "0x41100000",
         "got": "0x41000000", "xor": "0x100000"}])
    bad["kinds"]["add_f32"]["words_in_error"] = 2
    assert atomics.describe_failed(bad) == (
        "words_in_error 2; kinds add_f32; first: add_f32 index 494 expected 0x41100000 "
        "got 0x41000000")


def test_run_decodes_the_native_result(monkeypatch):
    """ok is about data only; unseen never changes it; observed == 0 is vacuous."""
    seen = {}

    class Lib:
        @staticmethod
        def gm_probe_atomics(dev, mask, blocks, iters, spread, rounds, lines, budget, seed, inj,
                             out):
            res = out._obj
            seen.update(mask=mask, blocks=blocks, inj=inj)
            res.tests_run, res.blocks, res.xccs_seen = mask, 256, 8
            res.kinds[7].ops, res.kinds[7].width = 100, 4096
            res.handoffs, res.observed, res.unseen = 10, seen["observed"], 10 - seen["observed"]
            res.stale_words = seen.get("stale", 0)
            if res.stale_words:
                res.records_filled = 1
                rec = res.records[0]
                rec.test, rec.kind, rec.index = 8, 12, 26 << 14 | 1500
                rec.expected, rec.got, rec.xcc_producer, rec.xcc_consumer = 5, 4, 3, 0
            return 0
    monkeypatch.setattr(_native, "probe", lambda: Lib)
    seen["observed"] = 7
    r = atomics.run(0)
    assert r["ok"] and not r["handoff_vacuous"] and r["unseen"] == 3 and seen["mask"] == 15
    assert list(r["kinds"]) == ["add_f32"] and r["tests"] == list(atomics.ALL_TESTS)
    seen["observed"] = 0
    r = atomics.run(0)
    assert r["ok"] and r["handoff_vacuous"] and r["unseen"] == 10
    r = atomics.run(0, tests=("add",))
    assert r["ok"] and not r["handoff_vacuous"]            # the hand-off did not run
    seen.update(observed=10, stale=1)
    r = atomics.run(0, _inject=("handoff", 3, 2, 1500, 0x100))
    assert not r["ok"] and r["stale_words"] == 1 and seen["inj"] is not None
    assert r["first_errors"] == [{"test": "handoff", "kind": "handoff", "index": 26 << 14 | 1500,
                                  "expected": "0x5", "got": "0x4", "xor": "0x1", "mailbox": 26,
                                  "word": 1500, "xcc_producer": 3, "xcc_consumer": 0}]


def test_doctor_wiring_ok_failed_and_vacuous(monkeypatch):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["atomics"].default is False and sig["atomics"].kind is sig["atomics"].KEYWORD_ONLY
    assert sig["atomics_inject"].default is None
    assert inspect.signature(doctor.run).parameters["atomics"].default is False
    calls, answer = [], {}

    def fake_run(dev, _inject=None):
        calls.append((dev, _inject))
        return _result(**(STALE if _inject else answer))
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(atomics, "run", fake_run)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "atomics" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, atomics=True) if c.name == "gpu0"]
    assert ok.status == "ok" and "hand-offs 2048/2048 seen (1792 across XCCs)" in ok.detail
    assert "atomics add+ticket+cas+handoff 256 blocks on 8 XCCs" in ok.detail
    answer.update(observed=0, unseen=2048, handoff_vacuous=True)
    (vac,) = [c for c in doctor.check_gpus(cfg, atomics=True) if c.name == "gpu0"]
    assert vac.status == "warn" and "proved nothing" in vac.detail
    inj = ("handoff", 3, 2, 1500, 0x100)
    (bad,) = [c for c in doctor.check_gpus(cfg, atomics=True, atomics_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail" and "failed: stale_words 1; lost_words 1; first: handoff " \
        "mailbox 26 word 1500" in bad.detail
    assert calls == [(0, None), (0, None), (0, inj)]


def test_probe_and_validate_wiring(monkeypatch, capsys):
    from gpumounter_amd import cli
    from gpumounter_amd.ops import probe
    from gpumounter_amd.parallel import validate

    calls = []

    def fake_run(dev, tests=atomics.ALL_TESTS, blocks=0, spread=atomics.DEFAULT_SPREAD,
                 rounds=atomics.DEFAULT_ROUNDS, _inject=None):
        calls.append((dev, tuple(tests), blocks, spread, rounds, _inject))
        return _result(**(STALE if _inject else {}))

    class Verified:
        def to_dict(self):
            return {"device": 0, "ok": True}
    monkeypatch.setattr(atomics, "run", fake_run)
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Verified()])
    ap = cli.build_parser()
    assert cli.cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--atomics"])) == 0
    assert json.loads(capsys.readouterr().out)[0]["atomics"]["ok"] is True
    assert cli.cmd_probe(ap.parse_args(
        ["probe", "--bdf", "0000:05:00.0", "--atomics", "--atomics-tests", "handoff",
         "--atomics-spread", "64", "--atomics-blocks", "9", "--atomics-rounds", "3",
         "--atomics-inject", "handoff:3:2:1500:0x100"])) == 1
    assert json.loads(capsys.readouterr().out)[0]["atomics"]["stale_words"] == 1
    assert cli.cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0"])) == 0
    assert "atomics" not in json.loads(capsys.readouterr().out)[0]
    assert calls == [(0, atomics.ALL_TESTS, 0, 4096, 8, None),
                     (0, ("handoff",), 9, 64, 3, ("handoff", 3, 2, 1500, 256))]

    del calls[:]
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2 * numel}])
    assert validate.main(["--atomics"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert rep["ok"] and rep["atomics"][0]["ok"] and "pairs_stale" not in rep["atomics"][0]
    assert validate.main(["--atomics", "--atomics-inject", "ticket:300:2"]) == 1
    assert json.loads(capsys.readouterr().out)["ok"] is False
    assert validate.main([]) == 0 and "atomics" not in json.loads(capsys.readouterr().out)
    assert [c[5] for c in calls] == [None, ("ticket", 300, 2)]
    with pytest.raises(SystemExit):
        validate.main(["--atomics-inject", "ticket:300:2"])
    with pytest.raises(SystemExit):
        validate.main(["--atomics", "--atomics-inject", "ticket:300"])
