"""The attributed burn-in's per-tile compare (k_count_diff_tiles) and what hangs on it, on
constructed data on the MI355X (``pytest -m gpu``): the counts, the three mark arrays, the log's
end, the kernel's log through the host blame rule, the plain and the attributed burn-in side by
side, and the traced GEMMs at M != N. Nothing here depends on where the runtime places a block:
the CU maps the compare reads are data the test writes.

The reference is :func:`tile_words`, a numpy model of the compare written out here; every
expected value is an exact count or bit pattern, so nothing has a tolerance.

n = 768 throughout: a 3 × 3 grid of tiles, so tile / 3 and tile % 3 are no shifts, and tile 4 has
a neighbour on every side."""
import functools

import numpy as np
import pytest

import test_burnin_attr_gpu as sibling
from gpumounter_amd import _native
from gpumounter_amd.ops import mxgemm, probe
from gpumounter_amd.ops.probe import ProbeError

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
N, T = 768, 256
NT = N // T
TILES = NT * NT
TILE_WORDS = T * T // 8                  # 16-byte words of one tile: 8192
CAP = _native.BURNIN_LOG_CAP
FORMATS = mxgemm.BURN_IN_FORMATS


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a host without a GPU")


# ---------------------------------------------------------------------------- the model
def tile_words(a, b):
    """The compare, in numpy: a and b are uint16 [n, n] (bf16 bit patterns), n a multiple of 256.
    Returns the differing 16-byte words of every 256 × 256 tile, row-major over the tiles."""
    n = a.shape[0]
    x = np.ascontiguousarray(a).view(np.uint32).reshape(n, n // 2)
    y = np.ascontiguousarray(b).view(np.uint32).reshape(n, n // 2)
    words = (x != y).reshape(n, n // 8, 4).any(axis=2)                   # [n, n / 8]
    return words.reshape(n // T, T, n // T, T // 8).sum(axis=(1, 3)).reshape(-1)


def dev(x):
    """A uint16 numpy array as a bf16 device tensor of the same bits."""
    return torch.from_numpy(np.array(x, dtype=np.uint16).view(np.int16)).to(DEV).view(
        torch.bfloat16)


def ids(values):
    """CU ids (0xFFFFFFFF included) as the int32 device tensor the traced GEMMs write."""
    return torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in values],
                        dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def base():
    """Random bits, made once and never written: every case's ``a``."""
    x = np.random.default_rng(768).integers(0, 1 << 16, size=(N, N), dtype=np.uint16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def base_dev():
    return dev(base())


def flipped(flips):
    """A copy of the base with element (row, col) XORed with mask for every (row, col, mask)."""
    b = base().copy()
    assert len({(r, c) for r, c, _ in flips}) == len(flips)
    for r, c, m in flips:
        assert 0 < m < 1 << 16
        b[r, c] ^= np.uint16(m)
    return b


def at(tile, row, col):
    """Element (row, col) of a tile as (row, col) of the n × n result."""
    return (tile // NT) * T + row, (tile % NT) * T + col


def by_tile(events):
    return sorted((e[0], e[1], e[4]) for e in events)


# ---------------------------------------------------------------------------- a. counts
def _corners():
    out = []
    for t in range(TILES):
        for k, (r, c) in enumerate(((0, 0), (0, T - 1), (T - 1, 0), (T - 1, T - 1))):
            out.append(at(t, r, c) + (1 + 4 * t + k,))
    return flipped(out)


def _full(tiles):
    """Every word of the given tiles differs: a nonzero mask on every element of them."""
    b = base().copy()
    rng = np.random.default_rng(4)
    for t in tiles:
        r, c = at(t, 0, 0)
        b[r:r + T, c:c + T] ^= rng.integers(1, 1 << 16, size=(T, T), dtype=np.uint16)
    return b


def _lanes():
    """Lane k (32 bits) of a 16-byte word is elements 2k and 2k + 1 of its 8; each of the 8
    (lane, half) pairs in a word of its own, spread over tiles 1, 3, 4, 5 and 7."""
    out = []
    for k in range(4):
        for h in range(2):
            word = 3 + 4 * (2 * k + h)                    # of the tile's 32 words per row
            t = (1, 3, 4, 5, 7)[(2 * k + h) % 5]
            out.append(at(t, 17 * k + 100 * h, 8 * word + 2 * k + h) + (1 << (2 * k + 7 * h),))
    return flipped(out)


def _sweep():
    """Word w of a tile's sweep is row w / 32, word w % 32 of the row. Thread w % 256 reads it
    in pass w / 256; waves are 64 threads: the words where the wave (63 | 64), the pass
    (255 | 256) and the sweep (8191) end, in tiles 4 and 2."""
    out = []
    for t, e in ((4, 0), (2, 7)):
        for w in (63, 64, 255, 256, TILE_WORDS - 1):
            out.append(at(t, w // 32, 8 * (w % 32) + e) + (0x8000 >> e,))
    return flipped(out)


def _random():
    rng = np.random.default_rng(500)
    elems = rng.choice(N * N, size=500, replace=False)
    masks = rng.integers(1, 1 << 16, size=500)
    return flipped([(int(e) // N, int(e) % N, int(m)) for e, m in zip(elems, masks)])


# name → (b, the per-tile counts written out by hand, or None where only the model knows them)
CASES = {
    "none": (lambda: base().copy(), [0] * TILES),
    "corners_of_every_tile": (_corners, [4] * TILES),
    "tile_4_in_full": (lambda: _full([4]), [0, 0, 0, 0, TILE_WORDS, 0, 0, 0, 0]),
    "all_but_tile_4_in_full": (lambda: _full([0, 1, 2, 3, 5, 6, 7, 8]),
                               [TILE_WORDS] * 4 + [0] + [TILE_WORDS] * 4),
    "each_lane_and_half": (_lanes, [0, 2, 0, 2, 2, 1, 0, 1, 0]),
    "two_elements_of_one_word": (lambda: flipped([at(4, 100, 8 * 9 + 1) + (0x10,),
                                                  at(4, 100, 8 * 9 + 6) + (0x2000,)]),
                                 [0, 0, 0, 0, 1, 0, 0, 0, 0]),
    "thread_and_wave_changes": (_sweep, [0, 0, 5, 0, 5, 0, 0, 0, 0]),
    "random_500": (_random, None),
}
CU_A = [0x001, 0x102, 0x203, 0x304, 0x405, 0x506, 0x607, 0x708, 0x010]
REF_A = [0x001, 0x112, 0x203, 0x314, 0x405, 0x516, 0x607, 0x718, 0x010]


@pytest.mark.parametrize("name", list(CASES))
def test_the_compare_counts_exactly_the_words_that_differ_tile_by_tile(name):
    make, by_hand = CASES[name]
    b_host = make()
    want = tile_words(base(), b_host)
    if by_hand is not None:
        assert want.tolist() == by_hand, "the model and the case's own arithmetic disagree"
    a, b = base_dev(), dev(b_host)
    cu, ref = ids(CU_A), ids(REF_A)
    for x, y in ((a, b), (b, a)):                         # and with the operands swapped
        r = probe.count_diff_tiles(x, y, cu, ref, 7)
        got = by_tile(r["events"])
        print(f"{name}: total={r['total']} cursor={r['cursor']} events={got}")
        assert got == [(7, t, int(w)) for t, w in enumerate(want) if w], name
        assert r["cursor"] == len(got) and r["total"] == int(want.sum()), name
        assert r["total"] == probe.count_diff(x, y), name
        assert all(e[2] == CU_A[e[1]] and e[3] == REF_A[e[1]] for e in r["events"]), name


# ---------------------------------------------------------------------------- b. marks
def one_word_in(tiles, salt=0):
    """One flipped element, so one word, in each of the given tiles."""
    return flipped([at(t, (37 * t + salt) % T, (91 * t + 3 * salt) % T) + (0x4000,)
                    for t in tiles])


def marks_model(cu, ref, words):
    """What one compare marks: (exonerated, moved, the ids seen)."""
    moved = [int(c != r) for c, r in zip(cu, ref)]
    exon = [int(c != r and w == 0) for c, r, w in zip(cu, ref, words)]
    seen = {c for c, r in zip(cu, ref) if c < 4096 and r < 4096}
    return exon, moved, seen


def seen_ids(r):
    assert len(r["seen"]) == _native.CUSCAN_IDS and set(r["seen"]) <= {0, 1}
    return {i for i, s in enumerate(r["seen"]) if s}


def test_the_marks_follow_the_maps_and_stay_set():
    a = base_dev()
    # ids 0 and 0xFFF, and 0x0FF / 0x7FF, which differ only above bit 7; tiles 0 1 3 5 7 stay
    # where the reference computed them, tiles 2 4 6 8 moved
    ref = [0x000, 0xFFF, 0x7FF, 0x7FF, 0x045, 0x045, 0x200, 0x0FF, 0x123]
    cu1 = [0x000, 0xFFF, 0x0FF, 0x7FF, 0x123, 0x045, 0x311, 0x0FF, 0x000]
    b1 = one_word_in([1, 2, 4, 7])                 # two that moved, two that did not
    w1 = tile_words(base(), b1)
    r1 = probe.count_diff_tiles(a, dev(b1), ids(cu1), ids(ref), 1)
    exon1, moved1, seen1 = marks_model(cu1, ref, w1)
    assert moved1 == [0, 0, 1, 0, 1, 0, 1, 0, 1] and exon1 == [0, 0, 0, 0, 0, 0, 1, 0, 1]
    assert r1["moved"] == moved1 and r1["exonerated"] == exon1
    assert seen_ids(r1) == seen1 == {0x000, 0xFFF, 0x0FF, 0x7FF, 0x123, 0x045, 0x311}
    want1 = [(1, t, cu1[t], ref[t], 1) for t in (1, 2, 4, 7)]
    assert sorted(r1["events"]) == want1 and r1["total"] == r1["cursor"] == 4

    # a second compare into the same state: other CUs, other differences. Tile 4 mismatched
    # above and now matches on another CU; tiles 6 and 8 are back on the reference's CU
    cu2 = [0x400, 0xFFF, 0x0FF, 0x001, 0x222, 0x045, 0x200, 0x333, 0x123]
    b2 = one_word_in([0, 5], salt=11)
    w2 = tile_words(base(), b2)
    r2 = probe.count_diff_tiles(a, dev(b2), ids(cu2), ids(ref), 2, state=r1["state"])
    exon2, moved2, seen2 = marks_model(cu2, ref, w2)
    assert exon2[4] == 1 and exon2[6] == exon2[8] == 0 and moved2[6] == moved2[8] == 0
    assert r2["moved"] == [x | y for x, y in zip(moved1, moved2)]
    assert r2["exonerated"] == [x | y for x, y in zip(exon1, exon2)] == [0, 0, 1, 1, 1, 0, 1, 1, 1]
    assert all(x >= y for x, y in zip(r2["moved"] + r2["exonerated"],
                                      r1["moved"] + r1["exonerated"]))       # nothing cleared
    assert seen_ids(r2) == seen1 | seen2 and seen_ids(r2) >= seen_ids(r1)
    want2 = want1 + [(2, 0, 0x400, 0x000, 1), (2, 5, 0x045, 0x045, 1)]
    assert sorted(r2["events"]) == want2                  # tile 4's event is still in the log
    assert r2["events"][:4] == r1["events"]               # and the log only grew
    assert r2["total"] == r2["cursor"] == 6
    assert r2["state"] is r1["state"]
    # the exoneration that came after the event decides the blame: tile 4's worker, not its
    # reference
    blame = probe.burn_in_blame(r2["events"], r2["exonerated"])
    unit = {b["id"]: b for b in blame["blamed"]}
    assert unit[0x123]["as_worker"] == 1 and 0x311 not in unit


@pytest.mark.parametrize("which", ("cu", "ref_cu"))
def test_an_unset_map_entry_is_no_cu(which):
    """0xFFFFFFFF is what a map holds where a block stored nothing: it is not CU 0xFFF."""
    cu = [0x001, 0x102, 0x203, 0x155, 0x405, 0x506, 0x607, 0x708, 0x010]
    ref = list(REF_A)
    (cu if which == "cu" else ref)[3] = 0xFFFFFFFF
    b = one_word_in([3, 6])
    r = probe.count_diff_tiles(base_dev(), dev(b), ids(cu), ids(ref), 5)
    assert r["seen"][0xFFF] == 0 and r["seen"][0x155] == 0
    assert seen_ids(r) == set(cu) - {0x155, 0xFFFFFFFF}
    assert sorted(r["events"]) == [(5, 3, cu[3], ref[3], 1), (5, 6, cu[6], ref[6], 1)]
    assert r["moved"][3] == 1 and r["total"] == 2
    with pytest.raises(ProbeError):
        probe.burn_in_blame(r["events"], r["exonerated"])


# ---------------------------------------------------------------------------- c. the log's end
def test_the_log_ends_at_its_capacity_and_the_count_goes_on():
    nbytes, guard = probe.BURN_IN_STATE_BYTES, 256
    buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    buf[:nbytes].zero_()
    state = probe.CompareState(buf[:nbytes], *(torch.zeros(k, dtype=torch.int32, device=DEV)
                                               for k in (TILES, TILES, _native.CUSCAN_IDS)))
    a, b = base_dev(), dev(one_word_in(range(TILES)))
    cu, ref = ids(CU_A), ids(REF_A)
    for i in range(1, 115):                               # 114 × 9 = 1026 events
        probe.count_diff_tiles(a, b, cu, ref, i, state=state, read=False)
    torch.cuda.synchronize()
    r = probe.read_compare_state(state)
    assert r["cursor"] == 1026 and r["total"] == 1026
    log = r["events"]
    assert len(log) == CAP and len(set(log)) == CAP
    assert all(e[2] == CU_A[e[1]] and e[3] == REF_A[e[1]] and e[4] == 1 for e in log)
    where = sorted((e[0], e[1]) for e in log)
    assert where[:1017] == [(i, t) for i in range(1, 114) for t in range(TILES)]
    last = where[1017:]
    assert len(last) == 7 and all(i == 114 and 0 <= t < TILES for i, t in last)
    assert len({t for _, t in last}) == 7
    assert buf[nbytes:].cpu().tolist() == [0xA5] * guard, "the compare wrote behind the log"
    blame = probe.burn_in_blame(log, r["exonerated"], counted=r["cursor"])
    assert blame["log_overflow"] is True and blame["events"] == 1026 and blame["logged"] == CAP


# ---------------------------------------------------------------------------- d. log → blame
UNITS = [0x005, 0x106, 0x207, 0x300, 0x401, 0x502, 0x603, 0x704, 0x00F]   # block b runs on UNITS[b]


def cu_map(r):
    """The CU of every tile when block b runs on UNITS[b] at rotation r."""
    tiles, _ = probe.burn_in_tile_map(N, r)
    out = [None] * TILES
    for block, t in enumerate(tiles):
        out[t] = UNITS[block]
    return out


def run_on_the_host(result_of, reference, iterations):
    """A burn-in in data: iteration i at rotation i · step mod 9, its result result_of(i, map)
    compared with `reference` on the device, one state for the run. Returns the host's view."""
    step = probe.burn_in_tile_map(N)[1]
    ref_map, state, r = cu_map(0), None, None
    ref_dev = dev(reference)
    for i in iterations:
        cu = cu_map(i * step % TILES)
        r = probe.count_diff_tiles(dev(result_of(i, cu)), ref_dev, ids(cu), ids(ref_map), i,
                                   state=state)
        state = r["state"]
    return r, ref_map


def test_a_cu_that_is_wrong_in_the_reference_too_is_the_only_unit_blamed():
    x = UNITS[4]

    def result(cu):        # every tile X computes has its element (0, 0) flipped
        return flipped([at(t, 0, 0) + (1,) for t in range(TILES) if cu[t] == x])

    r, ref_map = run_on_the_host(lambda i, cu: result(cu), result(cu_map(0)), range(1, 10))
    home = ref_map.index(x)
    # 8 rotated iterations, two events each (X's tile of the day, and the reference's tile of
    # X that another unit got right); at r = 0 (iteration 9) X computes its own tile again
    assert r["cursor"] == 16 and r["total"] == 16
    assert all(e[0] != 9 and (e[2] == x) != (e[3] == x) for e in r["events"])
    assert r["exonerated"] == [int(t != home) for t in range(TILES)]
    blame = probe.burn_in_blame(r["events"], r["exonerated"])
    assert [b["id"] for b in blame["blamed"]] == [x], blame
    assert blame["blamed"][0]["as_worker"] == 8 and blame["blamed"][0]["as_reference"] == 8


def test_a_transient_fault_blames_the_worker_it_happened_on():
    def result(i, cu):
        return flipped([at(5, 200, 100) + (0x80,)] if i == 3 else [])

    r, ref_map = run_on_the_host(result, base(), range(1, 10))
    worker = cu_map(3 * probe.burn_in_tile_map(N)[1] % TILES)[5]
    assert r["events"] == [(3, 5, worker, ref_map[5], 1)] and worker != ref_map[5]
    assert r["exonerated"] == [1] * TILES
    blame = probe.burn_in_blame(r["events"], r["exonerated"])
    (b,) = blame["blamed"]
    assert b["id"] == worker and b["as_worker"] == 1 and b["as_reference"] == 0


def test_a_reference_tile_nobody_reproduces_blames_the_references_cu():
    reference = flipped([at(7, 31, 255) + (0x8000,)])
    r, ref_map = run_on_the_host(lambda i, cu: base(), reference, range(1, 10))
    assert by_tile(r["events"]) == [(i, 7, 1) for i in range(1, 10)]
    assert r["exonerated"] == [int(t != 7) for t in range(TILES)]
    blame = probe.burn_in_blame(r["events"], r["exonerated"])
    (b,) = blame["blamed"]
    # 8 other units contradict it, and at r = 0 (iteration 9) its own block does: one more
    # against a reference nobody reproduced, not a unit disagreeing with itself
    assert b["id"] == ref_map[7] and b["as_reference"] == 9 and b["as_worker"] == 0
    assert (9, 7, ref_map[7], ref_map[7], 1) in r["events"]


# ---------------------------------------------------------------------------- e. both burn-ins
FLIPS_E = [(e, 0x8000) for e in (0, 9, 15, 255 * N + 255, 256 * N + 256, N * N - 1)]


@functools.lru_cache(maxsize=None)
def both_burn_ins(fmt):
    """One plain and one attributed burn-in with the same flips, run once per format."""
    plain = sibling.burn_in(fmt, N, _flips=FLIPS_E)
    attr = sibling.burn_in(fmt, N, _flips=FLIPS_E, attribute=True)
    a = attr["attribution"]
    print(f"{fmt}: plain iterations={plain['iterations']} mismatches={plain['mismatches']}; "
          f"attributed iterations={attr['iterations']} mismatches={attr['mismatches']} "
          f"events={a['events']} logged={a['logged']} blamed={a['blamed']} "
          f"first_events={a['first_events']}")
    return plain, attr


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_plain_and_the_attributed_burn_in_count_the_same_flips(fmt):
    """Six elements in 5 distinct words: 3 in tile 0 (elements 9 and 15 share one), 1 in tile 4,
    1 in tile 8."""
    want = tile_words(base(), flipped([(e // N, e % N, m) for e, m in FLIPS_E]))
    assert want.tolist() == [3, 0, 0, 0, 1, 0, 0, 0, 1]
    assert sibling.BURN_S == 0.3
    plain, attr = both_burn_ins(fmt)
    a = attr["attribution"]
    assert plain["iterations"] >= 1 and attr["iterations"] >= 1
    assert plain["mismatches"] == 5 * plain["iterations"]
    assert attr["mismatches"] == 5 * attr["iterations"]
    assert a["events"] == 3 * attr["iterations"]
    first = sorted((e["iteration"], e["tile"], e["words"]) for e in a["first_events"][:3])
    assert first == [(1, 0, 3), (1, 4, 1), (1, 8, 1)]
    assert ({b["id"] for b in a["blamed"]} ==
            {e["reference"] for e in a["first_events"]}), a        # 16 events: every tile's
    assert sum(b["events"] for b in a["blamed"]) == a["logged"] == min(a["events"], CAP)
    # the log's words: whole iterations of 5, and of the iteration the log's end cuts, one or
    # two of its three events (3, 1 and 1 words) in the order they were booked
    whole, rest = divmod(a["logged"], 3)
    cut = {0: {0}, 1: {1, 3}, 2: {2, 4}}[rest]
    assert sum(b["words"] for b in a["blamed"]) - 5 * whole in cut


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_flipped_reference_is_blamed_as_the_reference_only(fmt):
    """With 9 tiles every 9th iteration runs at r = 0, and about every fourth of those the runtime
    puts the block on the CU that computed the reference's tile (observed, not promised). Such
    an event used to be booked as a unit disagreeing with itself: 332 as reference + 10 as
    worker for tile 0's unit, 332 + 9 for the other two, in all three formats. Every other CU
    contradicts that reference too, so the rule now counts it against the reference."""
    a = both_burn_ins(fmt)[1]["attribution"]
    print(f"{fmt}: " + "; ".join(f"id {b['id']:#05x} {b['as_reference']} as reference + "
                                 f"{b['as_worker']} as worker" for b in a["blamed"]))
    assert a["blamed"]
    assert all(b["as_worker"] == 0 and b["as_reference"] > 0 for b in a["blamed"]), a["blamed"]


# ---------------------------------------------------------------------------- f. M != N
SHAPES_F = ((512, 768), (2304, 256))     # grids of 6 and 9; the second's last group: one tile row


@functools.lru_cache(maxsize=None)
def operands(fmt, m, n):
    """Operands of 3 K-tiles, filled once per case and never written to."""
    if fmt == "bf16":
        k = 192
        a = probe.fill_bf16(torch.empty((m, k), dtype=torch.bfloat16, device=DEV), sibling.SEED_A)
        bt = probe.fill_bf16(torch.empty((n, k), dtype=torch.bfloat16, device=DEV),
                             sibling.SEED_B)
        return a, bt
    k = 3 * mxgemm.TILE_K[fmt]
    return (mxgemm.fill(fmt, "random", sibling.SEED_A, m, k) +
            mxgemm.fill(fmt, "random", sibling.SEED_B, n, k))


def traced(fmt, m, n, r, _inject=None):
    ops = operands(fmt, m, n)
    if fmt == "bf16":
        return probe.gemm_nt_traced(*ops, r=r, _inject=_inject)
    return mxgemm.gemm_nt_traced(fmt, *ops, r=r, _inject=_inject)


@pytest.mark.parametrize("m,n", SHAPES_F)
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_traced_gemm_that_is_not_square_changes_no_bit_and_maps_every_tile(fmt, m, n):
    ops = operands(fmt, m, n)
    want = probe.gemm_nt(*ops) if fmt == "bf16" else mxgemm.gemm_nt(fmt, *ops)
    assert tuple(want.shape) == (m, n)
    grid, ntn = (m // T) * (n // T), n // T
    maps = {}
    for r in range(grid):
        c, cus = traced(fmt, m, n, r)
        assert probe.count_diff(c, want) == 0, (fmt, m, n, r)
        maps[r] = cus.cpu().tolist()
        assert len(maps[r]) == grid and all(0 <= i < 4096 for i in maps[r]), (r, maps[r])
    bits = want.view(torch.int16).cpu().numpy().view(np.uint16)
    for r in (0, grid - 2):
        target = maps[r][0]
        c, cus = traced(fmt, m, n, r, _inject=(target, 0x1))
        hit = [t for t, i in enumerate(cus.cpu().tolist()) if i == target]
        got = c.view(torch.int16).cpu().numpy().view(np.uint16)
        diff = sorted(map(tuple, np.argwhere(got != bits).tolist()))
        print(f"{fmt} {m}x{n} r={r}: id {target:#05x} computed tiles {hit}")
        assert diff == sorted((T * (t // ntn), T * (t % ntn)) for t in hit), (diff, hit)
        assert all(int(got[p]) ^ int(bits[p]) == 1 for p in diff)
