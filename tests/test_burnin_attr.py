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


def plain_map_mn(block, ntm, ntn):
    """plain_map for a grid of ntm × ntn tiles: the tile as (row, column)."""
    grid = ntm * ntn
    q, rem, xcd = grid // 8, grid % 8, block % 8
    wgid = block // 8 + sum(q + 1 if x < rem else q for x in range(xcd))
    group, within = divmod(wgid, 8 * ntn)
    rows = min(ntm - group * 8, 8)
    return group * 8 + within % rows, within // rows


@pytest.mark.parametrize("m,n", ((512, 768), (2304, 256), (768, 512), (256, 2304), (2560, 768)))
def test_the_rotated_map_of_a_grid_that_is_not_square_is_a_bijection(m, n):
    """On a square grid tm · (N / 256) + tn and tm · (M / 256) + tn are the same number. 2304 ×
    256 and 2560 × 768 end in a group of fewer than 8 tile rows."""
    lib, C = _native.probe(), _native.C
    ntm, ntn = m // 256, n // 256
    grid = ntm * ntn
    tm, tn, step = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    for r in range(grid):
        got = []
        for b in range(grid):
            assert lib.gm_probe_burn_in_tile_map(m, n, b, r, C.byref(tm), C.byref(tn),
                                                 C.byref(step)) == 0
            got.append((tm.value, tn.value))
        assert sorted(got) == [(i, j) for i in range(ntm) for j in range(ntn)], (m, n, r)
        assert got == [plain_map_mn((b + r) % grid, ntm, ntn) for b in range(grid)], (m, n, r)
    assert gcd(step.value, grid) == 1 and (grid <= 8 or step.value % 8 != 0)
    assert lib.gm_probe_burn_in_tile_map(m, n, 0, grid, C.byref(tm), C.byref(tn),
                                         C.byref(step)) == 1


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


def test_a_reference_that_its_own_cu_contradicts_too_is_still_blamed_as_the_reference():
    """At r = 0 a block may land on the CU that computed the reference's tile. Where other units
    contradict that reference as well and none reproduced it, the event is one more against the
    reference, not a unit disagreeing with itself."""
    others = [(i, 7, 0x200 + i, 0x045, 1) for i in range(1, 9)]
    own = [(9, 7, 0x045, 0x045, 1)]
    ex = [1] * 64
    ex[7] = 0
    for events in (others + own, own + others):                 # the order does not matter
        (b,) = probe.burn_in_blame(events, ex)["blamed"]
        assert b["id"] == 0x045 and b["as_reference"] == 9 and b["as_worker"] == 0
    # the witnesses must be at that tile, and logged
    (b,) = probe.burn_in_blame(own, ex)["blamed"]
    assert b["id"] == 0x045 and b["as_worker"] == 1 and b["as_reference"] == 0
    r = probe.burn_in_blame(own + [(1, 8, 0x201, 0x045, 1)], ex)
    unit = {b["id"]: b for b in r["blamed"]}
    assert unit[0x045]["as_worker"] == 1 and unit[0x201]["as_worker"] == 1
    # an exonerated tile stands: whoever differs from it there is blamed as the worker
    r = probe.burn_in_blame(others + own, [1] * 64)
    unit = {b["id"]: b for b in r["blamed"]}
    assert unit[0x045]["as_worker"] == 1 and unit[0x045]["as_reference"] == 0 and len(unit) == 9


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


# ---------------------------------------------------------------------------- the compare's seam
def test_the_published_state_is_the_one_the_library_uses():
    C = _native.C
    assert _native.probe().gm_probe_burn_in_state_bytes() == probe.BURN_IN_STATE_BYTES
    assert probe.BURN_IN_STATE_BYTES == 16 + 20 * _native.BURNIN_LOG_CAP
    s = _native.BurninState
    assert (s.total.offset, s.cursor.offset, s.log.offset) == (0, 8, 16)
    assert C.sizeof(_native.BurninEvent) == 20


def test_count_diff_tiles_refuses_before_the_native_call(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(_native, "probe", lambda: pytest.fail("the native library was reached"))
    bf, i32 = torch.bfloat16, torch.int32
    a, b = torch.zeros(512, 512, dtype=bf), torch.zeros(512, 512, dtype=bf)
    cu, ref = torch.zeros(4, dtype=i32), torch.zeros(4, dtype=i32)

    def state(nbytes=probe.BURN_IN_STATE_BYTES, exonerated=4, moved=4, seen=_native.CUSCAN_IDS):
        return probe.CompareState(torch.zeros(nbytes, dtype=torch.uint8),
                                  *(torch.zeros(k, dtype=i32) for k in (exonerated, moved, seen)))

    wide = torch.zeros(512, 1024, dtype=bf)
    for args, kw, why in (
            ((a.float(), b, cu, ref, 1), {}, "2-D bf16"),                       # dtype
            ((a, b.view(torch.int16), cu, ref, 1), {}, "2-D bf16"),
            ((a.view(-1), b.view(-1), cu, ref, 1), {}, "2-D bf16"),
            ((a, wide[:, ::2], cu, ref, 1), {}, "contiguous"),                  # strided
            ((a.t(), b, cu, ref, 1), {}, "contiguous"),
            ((torch.zeros(300, 300, dtype=bf),) * 2 + (cu, ref, 1), {}, "multiple of 256"),
            ((torch.zeros(0, 0, dtype=bf),) * 2 + (cu, ref, 1), {}, "multiple of 256"),
            ((a, torch.zeros(256, 256, dtype=bf), cu, ref, 1), {}, "multiple of 256"),
            ((wide, wide, cu, ref, 1), {}, "multiple of 256"),                  # not square
            ((a, b, cu, ref, -1), {}, "iteration"),
            ((a, b, cu, ref, 1 << 32), {}, "iteration"),
            ((a, b, cu, ref, True), {}, "iteration"),
            ((a, b, torch.zeros(9, dtype=i32), ref, 1), {}, "cu has 9 entries, not 4"),
            ((a, b, cu, torch.zeros(3, dtype=i32), 1), {}, "ref_cu has 3 entries, not 4"),
            ((a, b, cu.to(torch.int64), ref, 1), {}, "cu must be a contiguous int32"),
            ((a, b, cu, ref.float(), 1), {}, "ref_cu must be a contiguous int32"),
            ((a, b, cu, torch.zeros(8, dtype=i32)[::2], 1), {}, "ref_cu must be a contiguous"),
            ((a, b, [0] * 4, ref, 1), {}, "cu must be a contiguous int32"),
            ((a, b, cu, ref, 1), {"state": state(nbytes=probe.BURN_IN_STATE_BYTES - 20)},
             "exactly"),                                                        # the state
            ((a, b, cu, ref, 1), {"state": state(nbytes=probe.BURN_IN_STATE_BYTES + 64)},
             "exactly"),
            ((a, b, cu, ref, 1), {"state": state(exonerated=9)}, "exonerated has 9"),
            ((a, b, cu, ref, 1), {"state": state(moved=3)}, "moved has 3"),
            ((a, b, cu, ref, 1), {"state": state(seen=256)}, "seen has 256"),
            ((a, b, cu, ref, 1), {"state": tuple(state())}, "CompareState"),
            ((a, b, cu, ref, 1), {"state": state()}, "HIP device"),             # all else is right
            ((a, b, cu, ref, 1), {}, "HIP device")):
        with pytest.raises(ProbeError, match=why):
            probe.count_diff_tiles(*args, **kw)


def test_native_count_diff_tiles_refuses_before_any_hip_call():
    """Null, misaligned, bad n: 1 (hipErrorInvalidValue). Every pointer here is a host address,
    so a launch that got past the checks would not return quietly."""
    lib, C = _native.probe(), _native.C
    buf = (C.c_uint8 * 4096)()
    p = (C.addressof(buf) + 63) & ~63                   # 64-byte aligned, 4000 bytes behind it
    good = [p, p + 64, 256, p + 128, p + 192, 1, p + 256, p + 320, p + 384, p + 448, None]
    assert lib.gm_probe_count_diff_tiles.argtypes[2] is C.c_int
    for at, bad in ([(i, None) for i in (0, 1, 3, 4, 6, 7, 8, 9)] +
                    [(0, p + 8), (1, p + 64 + 2), (3, p + 128 + 1), (4, p + 192 + 2),
                     (6, p + 256 + 4), (7, p + 320 + 1), (8, p + 384 + 2), (9, p + 448 + 3)] +
                    [(2, n) for n in (0, -256, 100, 255, 257, 768 + 128, (1 << 31) - 256)]):
        args = list(good)
        args[at] = bad
        assert lib.gm_probe_count_diff_tiles(*args) == 1, (at, bad)


# ---------------------------------------------------------------------------- the tests' model
def test_the_numpy_model_of_the_compare_on_a_case_written_out_by_hand():
    """tests/test_burnin_compare_gpu.py checks the kernel against its ``tile_words``; this pins
    that model: 512 × 512, tiles 0 1 / 2 3, every count below worked out by hand."""
    np = pytest.importorskip("numpy")
    pytest.importorskip("torch")
    from test_burnin_compare_gpu import tile_words

    a = np.random.default_rng(1).integers(0, 1 << 16, size=(512, 512), dtype=np.uint16)
    assert tile_words(a, a).tolist() == [0, 0, 0, 0]
    b = a.copy()
    b[0, 0] ^= 1            # tile 0, row 0, word 0
    b[0, 7] ^= 0x8000       # the same word: its last element
    b[0, 8] ^= 1            # tile 0, row 0, word 1
    b[255, 255] ^= 2        # tile 0's last word
    b[255, 256] ^= 2        # tile 1, row 255, word 0: the next 16 bytes in memory
    b[256, 255] ^= 4        # tile 2, row 0, its last word
    b[511, 504] ^= 4        # tile 3's last word, first element
    b[511, 511] ^= 4        # ... and last
    b[300, 16:32] ^= 0x10   # tile 2, row 44: words 2 and 3 in full
    assert tile_words(a, b).tolist() == [3, 1, 3, 1]
    assert tile_words(b, a).tolist() == [3, 1, 3, 1]
    b = a ^ np.uint16(0x0100)                           # every element
    assert tile_words(a, b).tolist() == [8192] * 4
    b[256:, :256] = a[256:, :256]                       # but tile 2
    assert tile_words(a, b).tolist() == [8192, 8192, 0, 8192]
    c = np.zeros((768, 768), dtype=np.uint16)
    d = c.copy()
    d[256 + 5, 512 + 9] = 1                             # 3 × 3: tile 1 · 3 + 2
    assert tile_words(c, d).tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]


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
