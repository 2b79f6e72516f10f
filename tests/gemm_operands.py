"""Caller-built operands for the five GEMM kernels and a reference that shares nothing with the
project: plain numpy/torch on the CPU, no import from ``gpumounter_amd``, no table taken from a
header. The decoders are written from the formats' definitions (OCP 8-bit floating point, OCP
microscaling formats, bfloat16) so that each can be read against its definition in a minute.

Layouts are the kernels' public ones: A ``[M, K]`` and Bt ``[N, K]``, both K-major; for the MX
formats one code per element here (an e4m3 byte, or an e2m1 nibble that :func:`pack_fp4` packs two
per byte, low nibble first) and one E8M0 scale byte per 32 elements of K, ``[rows, K / 32]``.

A :class:`Case` holds operands; :meth:`Case.expected` evaluates them in float64 and returns the
expected bits, the NaN mask and the mask of compared elements. A :class:`Slip` is a modelled
mistake applied to that evaluation only (never to the operands): tests/test_gemm_operands.py
proves on the CPU that every case is moved by the slips it claims, so a kernel with that mistake
cannot pass tests/test_gemm_operands_gpu.py.
"""
from collections import namedtuple

import numpy as np
import torch

TILE_K = {"bf16": 64, "mxfp8": 128, "mxfp4": 256}     # elements of K in one K-tile (128 bytes)
BLOCK = 32                                            # elements of K under one scale


# ------------------------------------------------------------------ decoders, from the definitions
def e4m3_table():
    """OCP e4m3 (the "fn" form): 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 0 is
    subnormal (m/8 · 2^-6); S.1111.111 is NaN; there are no infinities."""
    t = np.empty(256, np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            t[b] = np.nan
            continue
        mag = m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -mag if b & 0x80 else mag
    return t


def e2m1_table():
    """OCP e2m1: nibble S.EE.M; the eight magnitudes, then their negatives (bit 3 is the sign)."""
    mags = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    return np.array(mags + [-v for v in mags], np.float64)


def e8m0_table():
    """E8M0 scale: 2^(b - 127); 255 is NaN."""
    t = 2.0 ** (np.arange(256, dtype=np.float64) - 127.0)
    t[255] = np.nan
    return t


def bf16_table():
    """bfloat16: 1 sign, 8 exponent (bias 127), 7 mantissa bits; all 65536 patterns as float64."""
    b = np.arange(65536, dtype=np.int64)
    e, m = (b >> 7) & 0xFF, (b & 0x7F).astype(np.float64)
    mag = np.where(e == 0, np.ldexp(m / 128.0, -126), np.ldexp(1.0 + m / 128.0, e - 127))
    mag = np.where(e == 255, np.where(m == 0, np.inf, np.nan), mag)
    return np.where(b & 0x8000, -mag, mag)


TABLES = {"mxfp8": e4m3_table, "mxfp4": e2m1_table, "bf16": bf16_table}


def code_of(fmt, value):
    """The code of ``value`` in the format's table, looked up by value (and sign)."""
    t = TABLES[fmt]()
    (hit,) = np.nonzero((t == value) & (np.signbit(t) == np.signbit(value)))
    assert len(hit) == 1, (fmt, value)
    return int(hit[0])


def pack_fp4(nibbles):
    """[rows, K] nibbles → [rows, K / 2] bytes, low nibble first."""
    n = np.asarray(nibbles, np.uint8)
    assert n.max() < 16 and n.shape[1] % 2 == 0
    return n[:, 0::2] | (n[:, 1::2] << 4)


# ------------------------------------------------------------------ the product and its rounding
def product(av, bv, ordered=False):
    """(ref, S): the float64 product av · bvᵀ of [M, K] and [N, K] values and the float64 sum of
    |products|. With any NaN or infinity among the values, or ``ordered``, the sum runs in k order
    in elementwise IEEE arithmetic (0 · inf = NaN, inf - inf = NaN); otherwise in the order numpy's
    matrix product takes, which gives the same for sums that are exact. ``+ 0.0``: the
    accumulators start at +0, so a sum of -0 products is +0."""
    if ordered or not (np.isfinite(av).all() and np.isfinite(bv).all()):
        ref, s = np.zeros((len(av), len(bv))), np.zeros((len(av), len(bv)))
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(av.shape[1]):
                p = av[:, k, None] * bv[None, :, k]
                ref += p
                s += np.abs(p)
        return ref, s
    return av @ bv.T + 0.0, np.abs(av) @ np.abs(bv).T


def to_f32(x):
    """float64 → float32, asserting that every finite value is exact in float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
    fin = np.isfinite(x)
    assert np.array_equal(f.astype(np.float64)[fin], x[fin]), "not exact in float32"
    return f


def bf16_bits(x, truncate=False):
    """float64 that is exact in float32 → bf16 bits, rounded to nearest even by torch's
    float32 → bfloat16 conversion (``truncate``: the fp32 bits cut instead, slip g)."""
    f = to_f32(x)
    if truncate:
        return (f.view(np.uint32) >> 16).astype(np.uint16)
    t = torch.from_numpy(f).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def f32_bits(x):
    return to_f32(x).view(np.uint32).copy()


def _lsb_exponent(x):
    """The exponent of the lowest set bit of every float64 in x (a large number for 0)."""
    m, e = np.frexp(x)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    _, le = np.frexp(low)
    return np.where(x == 0, 1 << 20, e.astype(np.int64) - 53 + le - 1)


def exact_in_fp32(av, bv, where=None):
    """True when every output element (of ``where``) has the same fp32 sum in any order. An
    element with one non-zero product only needs that product to be a normal fp32. Otherwise:
    with u the smallest product's lowest bit, every product is an integer multiple of u, so is
    every partial sum, and none exceeds S; S / u < 2^24 then makes each of them an exact fp32
    (also required: u ≥ 2^-126 and S < 2^128, so no fp32 denormal or overflow). u is taken per
    element as (lowest bit in A's row) · (lowest bit in Bt's row), which is never above the lowest
    bit of any product of the two rows, so the test is sufficient. Non-finite values are left
    out: what they give is fixed by IEEE, not by the order."""
    av, bv = np.where(np.isfinite(av), av, 0.0), np.where(np.isfinite(bv), bv, 0.0)
    s = np.abs(av) @ np.abs(bv).T
    terms = (av != 0).astype(np.float64) @ (bv != 0).astype(np.float64).T
    u = _lsb_exponent(av).min(axis=1)[:, None] + _lsb_exponent(bv).min(axis=1)[None, :]
    live = s != 0
    if where is not None:
        live = live & where
    single = live & (terms == 1)
    if np.any(s[single] < 2.0 ** -126) or np.any(s[single] >= 2.0 ** 128):
        return False
    if np.any(np.ldexp(s[single], -_lsb_exponent(s[single])) >= 2.0 ** 24):
        return False
    live &= ~single
    if not live.any():
        return True
    u, s = u[live], s[live]
    return bool(np.all(u >= -126) and np.all(s < 2.0 ** 128) and
                np.all(np.ldexp(s, -u) < 2.0 ** 24))


# ------------------------------------------------------------------ modelled slips
# kind: scale (a) | chunks (b) | nibbles (c) | reverse (d) | entry (e) | parity (f) | trunc (g);
# operand: "a" or "b" (None for trunc); code: the decoder entry of kind "entry".
Slip = namedtuple("Slip", "kind operand code", defaults=(None, None))
SLIP_KINDS = ("scale", "chunks", "nibbles", "reverse", "entry", "parity", "trunc")


def _k_index(kind, tk, k):
    """Where the slipped evaluation takes element k of a row from (tk: elements in a K-tile)."""
    i = np.arange(k)
    if kind == "chunks":          # fp8: 16-byte chunks g and 4 + g of a K-tile's 128 bytes
        return i ^ 64
    if kind == "nibbles":         # fp4: the two nibbles of a byte
        return i ^ 1
    if kind == "reverse":
        return i // tk * tk + (tk - 1 - i % tk)
    if kind == "parity":          # K-tile t from t ^ 1 where that tile exists (the other stage)
        t = i // tk ^ 1
        return np.where(t < k // tk, t * tk + i % tk, i)
    return i


Expected = namedtuple("Expected", "ref s bits nan compared")


class Case:
    """Operands of one launch. ``a`` / ``bt``: codes [rows, K] (uint8) or bf16 bits (uint16);
    ``sa`` / ``sb``: scale bytes [rows, K / 32], None for bf16. ``exact``: compared bit for bit
    (the builder proved :func:`exact_in_fp32`), else under a bound. ``band``: only elements whose
    exact value is 0 or within 2^±100 are compared. ``slips``: the modelled slips the case claims
    to catch."""

    def __init__(self, name, fmt, a, bt, sa=None, sb=None, exact=True, band=False, slips=(),
                 tile_k=None):
        self.name, self.fmt, self.exact, self.band, self.slips = name, fmt, exact, band, list(slips)
        self.a, self.bt, self.sa, self.sb = a, bt, sa, sb
        self.m, self.n, self.k = a.shape[0], bt.shape[0], a.shape[1]
        self.tile_k = tile_k or TILE_K[fmt]            # the 64² bf16 kernel's K-tile is 32
        assert bt.shape[1] == self.k and self.k % self.tile_k == 0
        assert self.m % 64 == 0 and self.n % 64 == 0
        if fmt != "bf16":
            assert sa.shape == (self.m, self.k // BLOCK) and sb.shape == (self.n, self.k // BLOCK)
            assert a.dtype == bt.dtype == sa.dtype == sb.dtype == np.uint8
            assert fmt == "mxfp8" or max(a.max(), bt.max()) < 16
        else:
            assert a.dtype == bt.dtype == np.uint16
        self._cache = {}

    @property
    def tiles(self):
        return self.k // self.tile_k

    def packed(self):
        """(A, sA, Bt, sB) as the MX kernel takes them."""
        pack = pack_fp4 if self.fmt == "mxfp4" else np.ascontiguousarray
        return pack(self.a), self.sa, pack(self.bt), self.sb

    def _operand(self, which, slip):
        codes, scales = (self.a, self.sa) if which == "a" else (self.bt, self.sb)
        table = TABLES[self.fmt]()
        if slip is not None and slip.operand == which:
            if slip.kind == "entry":
                table[slip.code] = table[slip.code ^ 1]
            elif slip.kind == "scale":
                scales = scales[:, np.arange(scales.shape[1]) ^ 1]
            else:
                codes = codes[:, _k_index(slip.kind, self.tile_k, self.k)]
                if slip.kind == "parity" and scales is not None:
                    scales = scales[:, _k_index("parity", self.tile_k, self.k)[::BLOCK] // BLOCK]
        v = table[codes]
        if scales is not None:
            v = v * np.repeat(e8m0_table()[scales], BLOCK, axis=1)
        return v

    def values(self, slip=None):
        """The decoded, scaled operands in float64: (A [M, K], Bt [N, K])."""
        return self._operand("a", slip), self._operand("b", slip)

    def expected(self, slip=None, out="bf16", ordered=False):
        """:class:`Expected` for a kernel that writes ``out`` ("bf16" or "fp32"): ``ref`` and
        ``s`` in float64; ``bits`` the expected pattern (only for exact cases; where ``nan`` the
        pattern is not compared); ``compared`` the elements a test asserts."""
        key = (slip, out, ordered)
        if key not in self._cache:
            ref, s = product(*self.values(slip), ordered=ordered)
            nan = np.isnan(ref)
            compared = np.ones(ref.shape, bool)
            if self.band:
                with np.errstate(invalid="ignore"):
                    mag = np.abs(ref)
                    compared = nan | (ref == 0) | ((mag >= 2.0 ** -100) & (mag <= 2.0 ** 100))
            bits = None
            if self.exact:
                shown = np.where(compared & ~nan, ref, 0.0)
                bits = (f32_bits(shown) if out == "fp32" else
                        bf16_bits(shown, truncate=slip is not None and slip.kind == "trunc"))
            for arr in (ref, s, nan, compared, bits):
                if arr is not None:
                    arr.setflags(write=False)
            self._cache[key] = Expected(ref, s, bits, nan, compared)
        return self._cache[key]

    def proves_exact(self):
        e = self.expected()
        return exact_in_fp32(*self.values(), where=e.compared & ~e.nan)

    def moved_by(self, slip, bound=None):
        """Whether the slip changes a compared element of the expected output: a bit for exact
        cases; for bounded ones |Δref| beyond twice the bound, so that no result can satisfy
        both."""
        e, x = self.expected(), self.expected(slip)
        both = e.compared & x.compared
        if self.exact:
            return bool(np.any((e.nan != x.nan) & (e.compared | x.compared)) or
                        np.any((e.bits != x.bits) & both & ~e.nan & ~x.nan))
        return bool(np.any(np.abs(e.ref - x.ref) > bound(e) + bound(x)))


def _both(*kinds):
    return [Slip(k, o) for k in kinds for o in "ab"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _perm(n, seed):
    return torch.randperm(n, generator=_gen(seed)).numpy()


def _randint(lo, hi, shape, seed):
    return torch.randint(lo, hi, shape, generator=_gen(seed)).numpy()


def _block_scales(rows, blocks, lo, span, seed):
    """Scale bytes lo … lo + span - 1 in which neighbouring blocks of a row, and the same block of
    neighbouring rows, always differ: (5 r + 7 s + offset) mod span with span coprime to 5, 7."""
    assert span % 5 and span % 7 and span > 7
    r, s = np.arange(rows)[:, None], np.arange(blocks)[None, :]
    return (lo + (5 * r + 7 * s + seed) % span).astype(np.uint8)


# ------------------------------------------------------------------ MX cases
def m1(fmt, hot="a"):
    """M1 (hot = "a") / M2 (hot = "b"): the hot operand has one code per row at k = p(row), p a
    bijection onto the k positions of two K-tiles; every row of the other holds one code at every
    k. fp8: 256 × 256, code = row, so rows and columns 127 and 255 are the NaN codes. fp4: 512 hot
    rows, 256 constant ones, code = row mod 16. Scales 124 … 132, different in neighbouring
    blocks and in the same block of the two K-tiles, so a hot element that lands in another block
    shows. One product per output of two ≤ 4-bit significands: exact in fp32 and in bf16."""
    k = 2 * TILE_K[fmt]
    rows = {"a": k if hot == "a" else 256, "b": k if hot == "b" else 256}     # hot: one row per k
    mask = 255 if fmt == "mxfp8" else 15
    ops = {}
    for which in "ab":
        code = (np.arange(rows[which]) & mask).astype(np.uint8)
        if which == hot:
            c = np.zeros((rows[which], k), np.uint8)
            c[np.arange(rows[which]), _perm(k, 11 if hot == "a" else 13)] = code
        else:
            c = np.repeat(code[:, None], k, axis=1)
        ops[which] = c, _block_scales(rows[which], k // BLOCK, 124, 9, 3 if which == "a" else 5)
    slips = [Slip("scale", "a"), Slip("scale", "b"), Slip("reverse", hot), Slip("parity", hot)]
    if fmt == "mxfp8":
        slips += [Slip("chunks", hot)]
        slips += [Slip("entry", o, c) for o in "ab" for c in (0x01, 0x39, 0x7E, 0xB2, 0xFE)]
    else:
        slips += [Slip("entry", o, c) for o in "ab" for c in (1, 6, 11)]
    return Case(f"{'M1' if hot == 'a' else 'M2'}-{fmt}", fmt, ops["a"][0], ops["b"][0],
                ops["a"][1], ops["b"][1], slips=slips)


def _hot_codes(fmt, rows, seed):
    """Non-zero finite codes of both signs whose products are exact in bf16: e4m3 codes with
    exponents -1 … 2 (4-bit significands, products of 8 bits), any non-zero e2m1 nibble."""
    i = (np.arange(rows) * 7 + seed) % 61
    if fmt == "mxfp8":
        return (0x30 + i % 32 + 0x80 * (i // 32 % 2)).astype(np.uint8)
    return (1 + i % 7 + 8 * (i // 7 % 2)).astype(np.uint8)


def m3(fmt):
    """M3: both operands one-hot, A row i at p(i), Bt row j at q(j) = p(σ(j)) for a permutation
    σ, over three K-tiles; every block of every row under a scale 120 … 134 that differs from its
    neighbours'. C[i, j] is non-zero exactly where i = σ(j), with the scales of that block."""
    k, rows = 3 * TILE_K[fmt], 256
    p = _perm(k, 17)[:rows]
    sigma = _perm(rows, 19)
    a, bt = np.zeros((rows, k), np.uint8), np.zeros((rows, k), np.uint8)
    a[np.arange(rows), p] = _hot_codes(fmt, rows, 0)
    bt[np.arange(rows), p[sigma]] = _hot_codes(fmt, rows, 29)
    kinds = ("scale", "reverse", "parity") + (("chunks",) if fmt == "mxfp8" else ("nibbles",))
    slips = _both(*kinds) + [Slip("entry", "a", int(a[0, p[0]])),
                             Slip("entry", "b", int(bt[0, p[sigma[0]]]))]
    return Case(f"M3-{fmt}", fmt, a, bt, _block_scales(rows, k // BLOCK, 120, 13, 1),
                _block_scales(rows, k // BLOCK, 122, 13, 6), slips=slips)


def m4_positions(fmt):
    """(K-tile, scale block of the tile) of M4's launches: every block position in both stages."""
    return [(t, s) for t in (0, 1) for s in range(TILE_K[fmt] // BLOCK)]


def m4(fmt, tile, block, nan=False):
    """M4: every row of A and of Bt is hot at the same k, in scale block ``block`` of K-tile
    ``tile``, with ±1.0 or ±1.5; A's row i has scale byte i there (row 255: 127), Bt's row j has
    254 - j (row 255: 127), so C[i, j] = ±{1, 1.5, 2.25} · 2^(i - j). The other blocks hold zeros
    under scales 0 … 254. Compared: the band 2^±100. ``nan``: additionally byte 255 in a zero block
    of A's row 77 and in the hot block of Bt's row 200."""
    tk, rows = TILE_K[fmt], 256
    k = 2 * tk
    hot_block = tile * (tk // BLOCK) + block
    k0 = hot_block * BLOCK + (5 * block + 11 * tile + 3) % BLOCK
    r = np.arange(rows)
    vals = np.array([1.0, -1.5, 1.5, -1.0])
    a, bt = np.zeros((rows, k), np.uint8), np.zeros((rows, k), np.uint8)
    a[:, k0] = [code_of(fmt, v) for v in vals[r % 4]]
    bt[:, k0] = [code_of(fmt, v) for v in vals[(r // 4 + r) % 4]]
    # zero blocks: any byte but 255, different from the hot block's in the neighbouring block
    sa = ((r[:, None] * 3 + np.arange(k // BLOCK)[None, :] * 37 + 101) % 255).astype(np.uint8)
    sb = ((r[:, None] * 7 + np.arange(k // BLOCK)[None, :] * 53 + 19) % 255).astype(np.uint8)
    sa[:, hot_block] = np.where(r < 255, r, 127)
    sb[:, hot_block] = np.where(r < 255, 254 - r, 127)
    for s, col in ((sa, hot_block), (sb, hot_block)):          # the scale slip must show
        clash = s[:, col ^ 1] == s[:, col]
        s[clash, col ^ 1] = (s[clash, col] + 9) % 255
    if nan:
        sa[77, hot_block ^ 2], sb[200, hot_block] = 255, 255
    kinds = ("scale", "reverse", "parity") + (("chunks",) if fmt == "mxfp8" else ("nibbles",))
    return Case(f"M4-{fmt}-t{tile}s{block}{'-nan' if nan else ''}", fmt, a, bt, sa, sb, band=True,
                slips=_both(*kinds))


M5_VALUES = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0, 6.0, -6.0)


def m5(fmt, m, n):
    """M5: dense; values 0, ±.5 … ±6 by a torch generator (fp8: their e4m3 bytes, found by value
    in the decoder above), block scales 126 … 129, three K-tiles. Exact by
    :func:`exact_in_fp32`, so the expected bits are the exact sum rounded once."""
    k = 3 * TILE_K[fmt]
    lut = np.array([code_of(fmt, v) for v in M5_VALUES], np.uint8)
    a = lut[_randint(0, len(lut), (m, k), 41 + m)]
    bt = lut[_randint(0, len(lut), (n, k), 43 + n)]
    sa = _randint(126, 130, (m, k // BLOCK), 47).astype(np.uint8)
    sb = _randint(126, 130, (n, k // BLOCK), 53).astype(np.uint8)
    kinds = ("scale", "reverse", "parity") + (("chunks",) if fmt == "mxfp8" else ("nibbles",))
    slips = _both(*kinds) + [Slip("trunc"), Slip("entry", "a", code_of(fmt, 1.5)),
                             Slip("entry", "b", code_of(fmt, -3.0))]
    return Case(f"M5-{fmt}-{m}x{n}", fmt, a, bt, sa, sb, slips=slips)


def m6(fmt):
    """M6: dense, every non-NaN code drawn uniformly, block scales 120 … 134, 512 × 512 × three
    K-tiles; compared under :func:`mx_bound`."""
    m = n = 512
    k = 3 * TILE_K[fmt]
    if fmt == "mxfp8":
        lut = np.array([b for b in range(256) if b & 0x7F != 0x7F], np.uint8)
    else:
        lut = np.arange(16, dtype=np.uint8)
    a, bt = lut[_randint(0, len(lut), (m, k), 59)], lut[_randint(0, len(lut), (n, k), 61)]
    sa = _randint(120, 135, (m, k // BLOCK), 67).astype(np.uint8)
    sb = _randint(120, 135, (n, k // BLOCK), 71).astype(np.uint8)
    kinds = ("scale", "reverse", "parity") + (("chunks",) if fmt == "mxfp8" else ("nibbles",))
    return Case(f"M6-{fmt}", fmt, a, bt, sa, sb, exact=False, slips=_both(*kinds))


def mx_bound(e):
    """The project's allowance for the MX pipe: 2^-9 of the sum of |products| for what the
    matrix core drops inside its sums, 2^-8 relative for the bf16 rounding of the result."""
    return 2.0 ** -9 * e.s + 2.0 ** -8 * np.abs(e.ref)


# ------------------------------------------------------------------ bf16 cases
BF16_NORMALS = np.array([b for b in range(65536) if 0 < (b >> 7) & 0xFF < 255], np.uint16)
BF16_SUBNORMALS = np.array([b for b in range(65536) if (b >> 7) & 0xFF == 0 and b & 0x7F],
                           np.uint16)
ONE = 0x3F80


def _one_hot(rows, k, seed):
    """[rows, k] bf16 bits: 1.0 at k = perm(row mod k), so every k is hot when rows ≥ k."""
    assert rows >= k
    a = np.zeros((rows, k), np.uint16)
    a[np.arange(rows), _perm(k, seed)[np.arange(rows) % k]] = ONE
    return a


def b1(hot="a", small=False, patterns=None):
    """B1: the hot operand one-hot 1.0 (256 rows; K = 192, three K-tiles), the other one holding
    every finite normal bf16 pattern of both signs and ±0, then repeats, in an order shuffled by
    a fixed permutation. ``small``: the 64² kernel's form, K = 96, 128 hot rows and 704 pattern
    rows. ``patterns``: other patterns to route instead (the subnormals)."""
    k, hot_rows, rows = (96, 128, 704) if small else (192, 256, 512)
    pats = np.concatenate([BF16_NORMALS, [0x0000, 0x8000]]) if patterns is None else patterns
    pats = pats.astype(np.uint16)
    assert rows * k >= len(pats)
    full = np.resize(pats, rows * k)[_perm(rows * k, 73)].reshape(rows, k)
    one = _one_hot(hot_rows, k, 79)
    a, bt = (one, full) if hot == "a" else (full, one)
    return Case(f"B1-{'small-' if small else ''}{hot}", "bf16", a, bt,
                slips=_both("reverse", "parity"), tile_k=32 if small else None)


B2_SHAPE = (512, 512, 192)
NAN, PINF, NINF = 0x7FC0, 0x7F80, 0xFF80
# (row, k, pattern): rows in both tile rows and both wave rows (row % 256 < 128 or not), k in all
# three K-tiles (so both LDS stages) and both 32-wide halves of a K-tile
B2_A = ((3, 5, NAN), (130, 70, PINF), (259, 40, NINF), (400, 150, PINF), (77, 100, NINF),
        (300, 190, NAN), (200, 33, PINF), (200, 129, NINF))          # row 200: +inf and -inf
# (col, k, pattern): columns in both tile columns and all four wave columns (col % 256 // 64)
B2_B = ((10, 64, NAN), (70, 5, PINF), (140, 70, NINF), (200, 170, PINF), (260, 40, PINF),
        (330, 150, NINF), (390, 96, NAN), (460, 33, NINF), (500, 100, PINF))
# meetings in one sum: A(130, 70)=+inf with Bt(140, 70)=-inf; A(259, 40)=-inf with Bt(260, 40)=+inf;
# A(400, 150)=+inf with Bt(330, 150)=-inf; A(200, 33)=+inf with Bt(460, 33)=-inf while A(200, 129)
# gives the same sum a second infinity; A(77, 100)=-inf with Bt(500, 100)=+inf


def b2():
    """B2: integers in [-3, 3] with NaN, +inf and -inf planted in A and Bt (B2_A, B2_B)."""
    m, n, k = B2_SHAPE
    lut = np.array([code_of("bf16", float(v)) for v in range(-3, 4)], np.uint16)
    a, bt = lut[_randint(0, 7, (m, k), 83)], lut[_randint(0, 7, (n, k), 89)]
    for op, plant in ((a, B2_A), (bt, B2_B)):
        for row, kk, pat in plant:
            op[row, kk] = pat
    return Case("B2", "bf16", a, bt, slips=_both("reverse", "parity"))


def b3_random():
    """B3's second operand set: normal draws times 2^randint(-8, 8), rounded to bf16."""
    m, n, k = 256, 512, 192
    out = []
    for rows, seed in ((m, 97), (n, 101)):
        x = torch.randn((rows, k), generator=_gen(seed))
        x = x * torch.exp2(torch.randint(-8, 9, (rows, k), generator=_gen(seed + 1)).float())
        out.append(x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy())
    return Case("B3-random", "bf16", out[0], out[1], exact=False,
                slips=_both("reverse", "parity"))


def bf16_bound(e, k, out="bf16"):
    """|C - ref| ≤ (K - 1) · 2^-23 · S + 2^-8 · |ref|: products of two bf16 are exact in fp32; each
    of the K - 1 additions loses at most one unit in the last place of a partial sum no larger than
    S, whether the pipe rounds or truncates; 2^-8 relative covers the one bf16 rounding and the
    second-order terms. An fp32 result has no second term."""
    return (k - 1) * 2.0 ** -23 * e.s + (2.0 ** -8 * np.abs(e.ref) if out == "bf16" else 0.0)


# fp32 bit patterns the epilogue must round: (name, fp32 bits, the bf16 bits it must become)
B4_EDGES = (("tie, down to even", 0x3F808000, 0x3F80),
            ("tie, up to even", 0x3F818000, 0x3F82),
            ("one ulp below a tie", 0x3F807FFF, 0x3F80),
            ("one ulp above a tie", 0x3F808001, 0x3F81),
            ("one ulp below a tie, odd", 0x3F817FFF, 0x3F81),
            ("one ulp above a tie, odd", 0x3F818001, 0x3F82),
            ("largest finite bf16", 0x7F7F0000, 0x7F7F),
            ("largest fp32 that rounds to it", 0x7F7F7FFF, 0x7F7F),
            ("first that rounds to +inf", 0x7F7F8000, 0x7F80))


def b4_edge_of_row(rows=256):
    """Which edge a row of C carries: chosen so that every edge meets all four accumulator
    registers (row mod 4, from tile_store's row = 4 (l >> 4) + reg) in both wave rows."""
    r = np.arange(rows)
    return (r // 4 + r) % len(B4_EDGES)


def b4():
    """B4: one 256² tile, K = 128. Row i of A holds the up to three bf16 pieces of its edge value
    (the fp32 cut into 8-bit slices, each exact in bf16), in three different 32-wide k steps;
    Bt is +1.0 in even rows and -1.0 in odd ones at every k. So C[i, j] = ±edge(i), a sum of
    products whose every partial sum is a subset of the edge's bits: exact in fp32."""
    rows, k = 256, 128
    a = np.zeros((rows, k), np.uint16)
    edge = b4_edge_of_row(rows)
    for i in range(rows):
        want = float(np.array([B4_EDGES[edge[i]][1]], np.uint32).view(np.float32)[0])
        pieces, rest = [], want
        while rest:
            cut = np.array([rest], np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
            pieces.append(float(cut.view(np.float32)[0]))              # the top 8 bits of the rest
            rest -= pieces[-1]
        if len(pieces) == 1:                                           # two products at least
            low = float(np.ldexp(1.0, _lsb_exponent(np.array(want))))
            pieces = [want - low, low]
        steps = _perm(4, 200 + i)
        for n, piece in enumerate(pieces):
            a[i, 32 * steps[n] + (i * 7 + n * 5) % 32] = f32_bits(np.array([piece]))[0] >> 16
        assert 2 <= len(pieces) <= 3 and bf16_table()[a[i]].sum() == want, (i, want)
    bt = np.where(np.arange(rows)[:, None] % 2 == 0, ONE, ONE | 0x8000) * np.ones((1, k), int)
    return Case("B4", "bf16", a, bt.astype(np.uint16), slips=[Slip("trunc")])


# ------------------------------------------------------------------ the list the CPU tests walk
def mx_cases(fmt):
    m4s = [m4(fmt, t, s) for t, s in m4_positions(fmt)] + [m4(fmt, 1, 2, nan=True)]
    return [m1(fmt, "a"), m1(fmt, "b"), m3(fmt)] + m4s + [m5(fmt, 256, 256), m5(fmt, 512, 768),
                                                          m6(fmt)]


def bf16_cases():
    return [b1("a"), b1("b"), b1("a", small=True), b1("b", small=True), b2(), b3_random(), b4()]
