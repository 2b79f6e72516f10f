"""The independent GEMM reference and the caller-built cases of tests/gemm_operands.py, checked
without a GPU: the decoders against torch's own conversions and the formats' definitions; the
reference against ``mxgemm.expected`` on the fill classes, read back through the numpy model of
tests/test_mxgemm.py (the only place the two meet); for every case the exactness proof and the
coverage it claims; and the sensitivity matrix: every case is moved by each modelled slip it
claims, and every slip moves some case. tests/test_gemm_operands_gpu.py runs the kernels on these
cases."""
import functools

import numpy as np
import pytest
import torch

import gemm_operands as go

FORMATS = ("mxfp8", "mxfp4")


@functools.lru_cache(maxsize=None)
def cases(fmt):
    return go.bf16_cases() if fmt == "bf16" else go.mx_cases(fmt)


def all_cases():
    return [c for fmt in FORMATS + ("bf16",) for c in cases(fmt)]


def bound_of(case):
    if case.fmt == "bf16":
        return lambda e: go.bf16_bound(e, case.k)
    return go.mx_bound


# ------------------------------------------------------------------ the decoders
def test_e4m3_table_is_torchs_float8_e4m3fn():
    want = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn)
    want = want.float().double().numpy()
    got = go.e4m3_table()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert set(np.nonzero(np.isnan(got))[0]) == {0x7F, 0xFF} and np.isfinite(got).sum() == 254
    fin = ~np.isnan(got)
    assert np.array_equal(got.view(np.uint64)[fin], want.view(np.uint64)[fin])
    assert got[0x7E] == 448 and got[0x01] == 2.0 ** -9 and got[0x38] == 1 and np.signbit(got[0x80])


def test_bf16_table_is_torchs_view_for_all_65536_patterns():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    want = bits.view(torch.bfloat16).double().numpy()
    got = go.bf16_table()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.sum() == 2 * 127
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])
    assert len(go.BF16_NORMALS) == 65024 and len(go.BF16_SUBNORMALS) == 254


def test_e8m0_e2m1_and_the_fp4_packing():
    s = go.e8m0_table()
    assert np.array_equal(s[:255], np.ldexp(1.0, np.arange(255) - 127)) and np.isnan(s[255])
    assert s[127] == 1.0 and s[0] == 2.0 ** -127 and s[254] == 2.0 ** 127
    t = go.e2m1_table()
    assert list(t[:8]) == [0, .5, 1, 1.5, 2, 3, 4, 6] and np.array_equal(t[8:], -t[:8])
    assert np.signbit(t[8]) and not np.signbit(t[0])
    packed = go.pack_fp4(np.array([[1, 2, 15, 0], [7, 8, 3, 12]]))
    assert packed.dtype == np.uint8 and packed.tolist() == [[0x21, 0x0F], [0x87, 0xC3]]
    assert go.code_of("mxfp8", 1.5) == 0x3C and go.code_of("mxfp8", -0.5) == 0xB0
    assert go.code_of("mxfp4", -6.0) == 15 and go.code_of("bf16", 1.0) == go.ONE


def test_bf16_rounding_helper_and_the_exactness_test_itself():
    x = np.array([B[1] for B in go.B4_EDGES], np.uint32).view(np.float32).astype(np.float64)
    assert go.bf16_bits(x).tolist() == [B[2] for B in go.B4_EDGES]
    assert go.bf16_bits(-x).tolist() == [B[2] | 0x8000 for B in go.B4_EDGES]
    assert go.bf16_bits(x, truncate=True).tolist() == [B[1] >> 16 for B in go.B4_EDGES]
    with pytest.raises(AssertionError):
        go.bf16_bits(np.array([1.0 + 2.0 ** -30]))
    # 2^24 and 1 in one sum: not every order is exact; 2^23 and 1 is
    one = np.array([[1.0, 1.0]])
    assert not go.exact_in_fp32(np.array([[2.0 ** 24, 1.0]]), one)
    assert go.exact_in_fp32(np.array([[2.0 ** 23, 1.0]]), one)
    assert not go.exact_in_fp32(np.array([[2.0 ** -130, 0.0]]), one)       # an fp32 denormal
    assert go.exact_in_fp32(np.array([[np.inf, 3.0]]), one)                # IEEE fixes the rest
    ref, s = go.product(np.array([[np.inf, -0.0]]), np.array([[0.0, 1.0], [2.0, 0.0], [0.0, 0.0]]))
    assert np.isnan(ref[0, 0]) and ref[0, 1] == np.inf and np.isnan(ref[0, 2])
    ref, _ = go.product(np.array([[-0.0, 0.0]]), np.array([[1.0, 0.0]]))
    assert ref[0, 0] == 0 and not np.signbit(ref[0, 0])


# ------------------------------------------------------------------ the two references meet once
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cls", ("exact", "blocks", "random"))
def test_reference_reproduces_mxgemm_expected_on_the_fill_classes(fmt, cls):
    import test_mxgemm as model
    from gpumounter_amd.ops import mxgemm

    m, n, k = 256, 256, go.TILE_K[fmt]
    sa, sb = 0x5151, 0xA3A3
    case = go.Case("fill", fmt, model.codes(fmt, cls, sa, m, k).astype(np.uint8),
                   model.codes(fmt, cls, sb, n, k).astype(np.uint8),
                   model.scales(cls, sa, m, k // 32).astype(np.uint8),
                   model.scales(cls, sb, n, k // 32).astype(np.uint8), exact=cls != "random")
    want = mxgemm.expected(fmt, cls, sa, sb, m, n, k)
    if cls == "random":
        e = case.expected(ordered=True)
        assert np.array_equal(e.ref.view(np.uint64), want[0].view(np.uint64))
        assert np.array_equal(e.s.view(np.uint64), want[1].view(np.uint64))
    else:
        assert case.proves_exact()
        e = case.expected()
        assert not e.nan.any() and e.compared.all() and np.array_equal(e.bits, want)


# ------------------------------------------------------------------ proofs and coverage
def test_every_bit_exact_case_sums_exactly_in_fp32():
    exact = [c for c in all_cases() if c.exact]
    assert len(exact) > 40
    for c in exact:
        assert c.proves_exact(), c.name
        e = c.expected()
        assert e.bits is not None and e.compared.any(), c.name
    for c in all_cases():
        assert c.m % 64 == 0 and c.n % 64 == 0 and (c.fmt == "bf16" or c.m % 256 == c.n % 256 == 0)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("hot", "ab")
def test_m1_m2_cover_every_code_pair_and_every_k(fmt, hot):
    c = go.m1(fmt, hot)
    hot_op, const_op = (c.a, c.bt) if hot == "a" else (c.bt, c.a)
    assert c.tiles == 2 and len(hot_op) == c.k and len(const_op) == 256
    assert np.all((const_op == const_op[:, :1]))
    e = c.expected()
    if fmt == "mxfp8":
        where = np.argmax(hot_op != 0, axis=1)[1:]          # row 0 holds code 0
        assert len(set(where)) == 255 and np.all((hot_op != 0).sum(axis=1)[1:] == 1)
        assert np.array_equal(hot_op.max(axis=1), np.arange(256))
        assert np.array_equal(const_op[:, 0], np.arange(256))
        nan = np.zeros((256, 256), bool)
        nan[[127, 255], :] = True
        nan[:, [127, 255]] = True
        assert np.array_equal(e.nan, nan) and e.compared.all()
        assert (~e.nan).sum() == 254 * 254                   # every finite pair, once
    else:
        assert not e.nan.any() and e.compared.all()
        pairs = (c.a.max(axis=1).astype(int)[:, None] * 16 + c.bt.max(axis=1)[None, :]).ravel()
        assert np.bincount(pairs, minlength=256).min() >= 16
        # every k of both K-tiles is hot in exactly one row (rows of code 0 hold a zero there)
        assert (hot_op != 0).sum(axis=0).max() == 1 and (hot_op != 0).sum() == c.k * 15 // 16
    for s in (c.sa, c.sb):
        assert s.min() >= 124 and s.max() <= 132 and np.all(s[:, 1:] != s[:, :-1])
    # no rounding at all: the expected bf16 is the exact value
    v = go.bf16_table()[e.bits]
    assert np.array_equal(v[~e.nan], e.ref[~e.nan])


@pytest.mark.parametrize("fmt", FORMATS)
def test_m3_pairs_each_element_with_its_own_blocks_scales(fmt):
    c = go.m3(fmt)
    blocks = c.k // go.BLOCK
    assert c.tiles == 3 and blocks == {"mxfp8": 12, "mxfp4": 24}[fmt]
    for s in (c.sa, c.sb):
        assert s.min() >= 120 and s.max() <= 134
        assert np.all(s[:, 1:] != s[:, :-1]) and np.all(s[1:] != s[:-1])
    assert np.all((c.a != 0).sum(axis=1) == 1) and np.all((c.bt != 0).sum(axis=1) == 1)
    p, q = np.argmax(c.a != 0, axis=1), np.argmax(c.bt != 0, axis=1)
    assert set(p // go.BLOCK) == set(range(blocks))          # every block of every K-tile is hot
    e = c.expected()
    assert np.array_equal(e.ref != 0, p[:, None] == q[None, :]) and (e.ref != 0).sum() == 256
    i, j = np.nonzero(e.ref)
    t = go.TABLES[fmt]()
    want = (t[c.a[i, p[i]]] * t[c.bt[j, q[j]]] *
            2.0 ** (c.sa[i, p[i] // 32].astype(int) + c.sb[j, q[j] // 32].astype(int) - 254))
    assert np.array_equal(e.ref[i, j], want) and np.array_equal(go.bf16_table()[e.bits], e.ref)
    assert np.any(e.ref < 0) and np.any(e.ref > 0)


@pytest.mark.parametrize("fmt", FORMATS)
def test_m4_meets_every_scale_byte_in_every_block_position_of_both_stages(fmt):
    positions = go.m4_positions(fmt)
    assert len(positions) == {"mxfp8": 8, "mxfp4": 16}[fmt]
    every = set(range(255))
    for tile, block in positions:
        c = go.m4(fmt, tile, block)
        hot = tile * (go.TILE_K[fmt] // go.BLOCK) + block
        assert np.all((c.a != 0).sum(axis=1) == 1) and np.array_equal(c.a != 0, c.bt != 0)
        assert set(np.argmax(c.a != 0, axis=1) // go.BLOCK) == {hot}
        assert c.sa.max() < 255 and c.sb.max() < 255
        e = c.expected()
        assert not e.nan.any() and e.compared.mean() >= 0.5, (c.name, e.compared.mean())
        assert np.all(e.ref != 0)
        rows, cols = e.compared.any(axis=1), e.compared.any(axis=0)
        assert set(c.sa[rows, hot]) == every and set(c.sb[cols, hot]) == every
        mag = np.abs(e.ref)
        assert np.array_equal(e.compared, (mag >= 2.0 ** -100) & (mag <= 2.0 ** 100))
        assert mag.min() < 2.0 ** -150 and mag.max() > 2.0 ** 150       # the band excludes some
    c = go.m4(fmt, 1, 2, nan=True)
    nan = np.zeros((256, 256), bool)
    nan[77, :] = True
    nan[:, 200] = True
    assert np.array_equal(c.expected().nan, nan)
    assert (c.sa == 255).sum() == 1 and (c.sb == 255).sum() == 1


@pytest.mark.parametrize("fmt", FORMATS)
def test_m5_m6_hold_what_they_claim(fmt):
    t = go.TABLES[fmt]()
    for m, n in ((256, 256), (512, 768)):
        c = go.m5(fmt, m, n)
        assert (c.m, c.n, c.tiles) == (m, n, 3)
        assert set(np.unique(t[c.a])) == set(go.M5_VALUES) == set(np.unique(t[c.bt]))
        assert set(np.unique(c.sa)) == {126, 127, 128, 129} == set(np.unique(c.sb))
        e = c.expected()
        assert np.any(go.bf16_table()[e.bits] != e.ref)      # some results do round
    c = go.m6(fmt)
    assert (c.m, c.n, c.tiles) == (512, 512, 3) and not c.exact
    codes = set(range(256)) - {0x7F, 0xFF} if fmt == "mxfp8" else set(range(16))
    assert set(np.unique(c.a)) == codes == set(np.unique(c.bt))
    assert set(np.unique(c.sa)) == set(range(120, 135)) == set(np.unique(c.sb))
    e = c.expected()
    assert np.isfinite(e.ref).all() and np.all(e.s > 0)


@pytest.mark.parametrize("small", (False, True))
@pytest.mark.parametrize("hot", "ab")
def test_b1_routes_every_finite_normal_pattern(hot, small):
    c = go.b1(hot, small)
    one, full = (c.a, c.bt) if hot == "a" else (c.bt, c.a)
    assert c.k == (96 if small else 192) and c.tiles * 64 >= c.k - 32
    assert np.all((one != 0).sum(axis=1) == 1) and np.all((one != 0).sum(axis=0) >= 1)
    assert set(full.ravel()) == set(go.BF16_NORMALS) | {0x0000, 0x8000}
    e = c.expected()
    assert not e.nan.any() and np.isfinite(e.ref).all()
    got = e.bits if hot == "a" else e.bits.T
    assert set(got.ravel()) == set(go.BF16_NORMALS) | {0x0000}     # 1 · (-0) + 0 = +0
    sub = go.b1(hot, small, patterns=go.BF16_SUBNORMALS)
    full = sub.bt if hot == "a" else sub.a
    assert set(full.ravel()) == set(go.BF16_SUBNORMALS)


def test_b2_plants_specials_on_every_path():
    for plant, wave in ((go.B2_A, lambda r: r % 256 // 128), (go.B2_B, lambda r: r % 256 // 64)):
        assert len(plant) >= 8 and {pat for _, _, pat in plant} == {go.NAN, go.PINF, go.NINF}
        assert {r // 256 for r, _, _ in plant} == {0, 1}
        assert {wave(r) for r, _, _ in plant} == set(range(2 if plant is go.B2_A else 4))
        assert {k // 64 for _, k, _ in plant} == {0, 1, 2}
        assert {k % 64 // 32 for _, k, _ in plant} == {0, 1}
    c = go.b2()
    assert (c.m, c.n, c.k) == go.B2_SHAPE
    e = c.expected()
    t = go.bf16_table()
    rows = {r for r, _, _ in go.B2_A}
    cols = {r for r, _, _ in go.B2_B}
    special = ~np.isfinite(e.ref)
    outside = np.ones_like(special)
    outside[sorted(rows), :] = False
    outside[:, sorted(cols)] = False
    assert not special[outside].any() and special[~outside].all()
    assert e.nan.any() and (e.ref == np.inf).any() and (e.ref == -np.inf).any()
    # the meetings: equal signs of infinity in one product give -inf · … as IEEE has it
    assert e.ref[130, 140] == -np.inf or np.isnan(e.ref[130, 140])
    assert np.isnan(e.ref[200, 460]) or np.isinf(e.ref[200, 460])
    clean = np.where(np.isfinite(t[c.a]), t[c.a], 0) @ np.where(np.isfinite(t[c.bt]), t[c.bt], 0).T
    assert np.array_equal(e.ref[outside], clean[outside]) and np.abs(clean).max() > 100


def test_b4_lands_every_edge_on_every_register_of_both_wave_rows():
    c = go.b4()
    assert (c.m, c.n, c.k) == (256, 256, 128)
    edge = go.b4_edge_of_row()
    for v in range(len(go.B4_EDGES)):
        rows = np.nonzero(edge == v)[0]
        assert {(r % 4, r // 128) for r in rows} == {(reg, wm) for reg in range(4) for wm in (0, 1)}
    e = c.expected()
    want = np.array([B[2] for B in go.B4_EDGES], np.uint16)[edge]
    assert np.array_equal(e.bits[:, 0::2], np.repeat(want[:, None], 128, axis=1))
    assert np.array_equal(e.bits[:, 1::2], np.repeat(want[:, None] | 0x8000, 128, axis=1))
    assert np.array_equal(c.expected(out="fp32").bits[:, 0],
                          np.array([B[1] for B in go.B4_EDGES], np.uint32)[edge])
    # the pieces of a row lie in different 32-wide k steps: no MFMA sums two of them
    k = [np.nonzero(row)[0] // 32 for row in c.a]
    assert all(len(set(s)) == len(s) and 2 <= len(s) <= 3 for s in k)


# ------------------------------------------------------------------ the sensitivity matrix
def test_every_case_is_moved_by_its_slips_and_every_slip_moves_a_case():
    moved = {kind: [] for kind in go.SLIP_KINDS}
    for c in all_cases():
        assert c.slips, f"{c.name} claims no slip"
        for slip in c.slips:
            assert c.moved_by(slip, bound_of(c)), f"{c.name} is not moved by {slip}"
            moved[slip.kind].append(c.name)
    for kind, names in moved.items():
        assert names, f"no case is sensitive to slip {kind!r}"
    # each slip kind is caught in both operands, and in both MX formats where it applies
    for kind in ("scale", "reverse", "parity", "entry"):
        for fmt in FORMATS:
            ops = {s.operand for c in cases(fmt) for s in c.slips if s.kind == kind}
            assert ops == {"a", "b"}, (kind, fmt)
    assert {s.operand for c in cases("mxfp8") for s in c.slips if s.kind == "chunks"} == {"a", "b"}
    assert {s.operand for c in cases("mxfp4") for s in c.slips if s.kind == "nibbles"} == {"a", "b"}
