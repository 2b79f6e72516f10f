"""Lane scan without a GPU (gpumounter_amd/ops/lanescan.py, native/include/gm_lanescan_ref.h):
the host table of every test against an independent numpy / pure-Python reference with its own
lane model, the DPP masks and bound_ctrl on hand-made cases, the parsers and refusals, the
command lines and the doctor wording."""
import ctypes as C
import inspect

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import cuscan, lanescan
from gpumounter_amd.ops.probe import ProbeError

SEEDS = (0, 0x0123456789ABCDEF)
ITERS = (1, 3, lanescan.MAX_ITERS)
M32 = 0xFFFFFFFF
T = np.arange(256, dtype=np.uint64)         # thread ids
L = T % 64                                  # lane ids


# ---------------------------------------------------------------- the reference's own pieces
def H(seed, test, idx):
    """The CU scan's hash (gm_probe.h), on an int or a numpy array of indices, in uint64."""
    idx = np.asarray(idx, dtype=np.uint64) & M32
    h = (np.uint64(seed & M32) ^ (idx * np.uint64(0x9E3779B1) & M32))
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x85EBCA6B) & M32
    h ^= h >> np.uint64(13)
    h = (h + np.uint64(((seed >> 32) ^ (test * 0xC2B2AE35)) & M32)) & M32
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0xC2B2AE35) & M32
    h ^= h >> np.uint64(13)
    h = h * np.uint64(0x27D4EB2F) & M32
    h ^= h >> np.uint64(16)
    return h


def Hi(seed, test, idx):
    return int(H(seed, test, idx))


def rotl(v, s):
    v = np.asarray(v, dtype=np.uint64)
    return ((v << np.uint64(s)) | (v >> np.uint64(32 - s))) & M32


def fold(s, v):
    return (rotl(s, 5) + (np.asarray(v, dtype=np.uint64) & M32)) & M32


def f32_bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)


def f64_word(v):
    u = np.asarray(v, dtype=np.float64).view(np.uint64)
    return (u & M32) ^ rotl(u >> np.uint64(32), 16)


def f16_bits(v):
    return np.asarray(v, dtype=np.float16).view(np.uint16).astype(np.uint64)


# ---------------------------------------------------------------- xlane: the lane model
def dpp_sources(ctrl):
    """For each of the 64 lanes: the lane a DPP control reads, or None when there is none."""
    out = []
    for lane in range(64):
        row, pos = divmod(lane, 16)
        n = ctrl & 15
        if ctrl < 0x100:
            src = lane - lane % 4 + ((ctrl >> 2 * (lane % 4)) & 3)
        elif 0x101 <= ctrl <= 0x10F:                       # row_shl: towards lane 0
            src = lane + n if pos + n < 16 else None
        elif 0x111 <= ctrl <= 0x11F:                       # row_shr: towards lane 15
            src = lane - n if pos - n >= 0 else None
        elif 0x121 <= ctrl <= 0x12F:                       # row_ror
            src = 16 * row + (pos - n) % 16
        else:
            src = {0x130: lane + 1 if lane < 63 else None, 0x134: (lane + 1) % 64,
                   0x138: lane - 1 if lane > 0 else None, 0x13C: (lane - 1) % 64,
                   0x140: 16 * row + 15 - pos, 0x141: lane - lane % 8 + 7 - lane % 8,
                   0x142: 16 * row - 1 if row else None, 0x143: 31 if lane >= 32 else None}[ctrl]
        out.append(src)
    return out


def dpp(ctrl, row_mask, bank_mask, bound_ctrl, old, src):
    """old and src: arrays whose last axis is the 64 lanes."""
    take, keep, zero = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=bool), np.zeros(64, dtype=bool)
    for lane, frm in enumerate(dpp_sources(ctrl)):
        if not (row_mask >> lane // 16 & 1 and bank_mask >> lane % 16 // 4 & 1):
            keep[lane] = True                              # a disabled lane keeps old
        elif frm is not None:
            take[lane] = frm
        elif bound_ctrl:
            zero[lane] = True                              # out of range reads 0 ...
        else:
            keep[lane] = True                              # ... or, without bound_ctrl, keeps old
    return np.where(zero, 0, np.where(keep, old, src[..., take]))


def swizzle(off, src):
    if off & 0x8000:
        return src[..., [l - l % 4 + ((off >> 2 * (l % 4)) & 3) for l in range(64)]]
    a, o, x = off & 31, off >> 5 & 31, off >> 10 & 31
    return src[..., [l // 32 * 32 + ((l % 32 & a | o) ^ x) for l in range(64)]]


def move(entry, g, old, src):
    """One movement on uint64 arrays [waves, 64 lanes]."""
    kind, imm = entry["kind"], entry["imm"]
    if kind == 0:
        return dpp(imm, entry["row_mask"], entry["bank_mask"], entry["bound_ctrl"], old, src)
    if kind == 1:
        return swizzle(imm, src)
    affine = [(l * (g | 1) + (g >> 8)) % 64 for l in range(64)]
    if kind == 34:
        return src[:, affine]
    if kind == 35:
        return src[:, [((l & g >> 14) + (g >> 20)) % 64 for l in range(64)]]
    if kind == 36:
        assert sorted(affine) == list(range(64))           # no two lanes write one destination
        out = np.zeros_like(src)
        out[:, affine] = src
        return out
    if kind == 37:
        return np.repeat(src[:, g % 64:g % 64 + 1], 64, axis=1)
    if kind == 38:
        return np.repeat(src[:, :1], 64, axis=1)
    if kind == 39:
        out = old.copy()
        out[:, 21 * (g % 4)] = src[:, (g >> 8) % 64]
        return out
    if kind in (40, 41):                                   # v_permlane16_swap, v_permlane32_swap
        n = 16 if kind == 40 else 32
        a, b = old.copy(), src.copy()
        for base in range(0, 64, 2 * n):
            a[:, base + n:base + 2 * n] = src[:, base:base + n]
            b[:, base:base + n] = old[:, base + n:base + 2 * n]
        return (a + rotl(b, 13)) & M32
    assert kind == 42
    votes = src >> np.uint64(g % 32) & np.uint64(1)
    ballot = (votes << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)[:, None]
    below = np.cumsum(votes, axis=1, dtype=np.uint64) - votes
    return ((old ^ (ballot & M32) ^ (ballot >> np.uint64(32))) + below) & M32


def ref_xlane(seed, iters):
    menu, _ = lanescan.lanes()
    first = Hi(seed, 0x301, 0) % len(menu)
    lane = np.arange(64, dtype=np.uint64)
    x = [H(seed, 0x300, 4 * T + j).reshape(4, 64) for j in range(4)]
    for s in range(iters * len(menu)):
        moved = move(menu[(first + s) % len(menu)], Hi(seed, 0x301, 1 + s), x[(s + 1) % 4], x[s % 4])
        x[s % 4] = (rotl((moved + rotl(x[s % 4], 16)) & M32, 9) ^ ((lane * np.uint64(0x85EBCA6B) + np.uint64(s)) & M32)) \
            * np.uint64(0x9E3779B1) & M32
    return np.array([v.reshape(256) for v in x]).T


# ---------------------------------------------------------------- the other five
def ref_regfile(seed, iters):
    reg = H(seed, 0x310, T[:, None] * 384 + np.arange(384, dtype=np.uint64)[None, :])   # [256, 384]
    s = np.zeros((4, 256), dtype=np.uint64)
    rows = np.arange(256)
    for rnd in range(iters):
        for k in range(16):
            g = Hi(seed, 0x311, 16 * rnd + k)
            r = np.full(256, g % 192) if k < 12 else 32 * (g % 6) + ((g >> 8) + L.astype(np.int64)) % 32
            r = r.astype(np.int64)
            s[k % 4] = fold(s[k % 4], reg[rows, r])
            reg[rows, r] ^= np.uint64(M32)
        for r in list(range(192)) + list(range(192, 384)):
            s[r % 4] = fold(s[r % 4], reg[:, r])
            reg[:, r] ^= np.uint64(M32)
    for r in range(384):
        s[r % 4] = fold(s[r % 4], reg[:, r])
    return s.T


def signed32(v):
    return v - (1 << 32) if v >> 31 else v


def ref_salu(seed, iters):
    out = np.zeros((256, 4), dtype=np.uint64)
    for w in range(4):
        v = [H(seed, 0x322, 4 * (64 * w + np.arange(64, dtype=np.uint64)) + i) for i in range(4)]
        lane = np.arange(64, dtype=np.uint64)
        a, b = Hi(seed, 0x321, 4 * w), Hi(seed, 0x321, 4 * w + 1)
        c = Hi(seed, 0x321, 4 * w + 2) << 32 | Hi(seed, 0x321, 4 * w + 3)
        for s in range(iters * 16):
            k = Hi(seed, 0x320, (a ^ s) % 1024)
            m = a * k
            a ^= m >> 32
            b = (b + m) & M32
            c = (c + (b << 32 | a) - k) % (1 << 64)
            a ^= b << k % 32 & M32
            b ^= a >> (k >> 5) % 32
            a = (a + (signed32(b) >> (k >> 10) % 32)) & M32          # Python's >> floors
            r = (k >> 15) % 32 + 1
            c = (c << r | c >> 64 - r) % (1 << 64)
            off, wd = (k >> 20) % 16, (k >> 24) % 16 + 1
            e = (a >> off) % (1 << wd)
            se = (b >> off) % (1 << wd)
            se -= (1 << wd) if se >> wd - 1 else 0
            b = (b + bin(a).count("1") + 33 * ((a & -a).bit_length() - 1 if a else 32)
                 + 97 * (32 - b.bit_length())) & M32
            a ^= int(f"{b:032b}"[::-1], 2)
            a = (a + e) & M32 if a < b else (a - se) & M32
            b = (max(b, k) - min(signed32(a), signed32(k))) & M32
            a = (a + abs(signed32(a) - signed32(b))) & M32
            a ^= c & M32
            b ^= c >> 32
            i, j = s % 4, (s + 2) % 4
            v[i] = (rotl(v[i], 7) + (np.uint64(a) ^ (lane * np.uint64(0x01000193) & M32))) & M32
            v[j] = v[j] ^ ((np.uint64(b) + lane) & M32)
        out[64 * w:64 * w + 64] = np.array(v).T
    return out


def ref_trans(seed, iters):
    _, ops = lanescan.lanes()
    g = [H(seed, 0x331, 4 * T + i) for i in range(4)]
    sin_of = np.array([0.0, 1.0, 0.0, -1.0])
    for s in range(iters * 8):
        h = H(seed, 0x330, 256 * s + T).astype(np.int64)
        carry = (g[0] & np.uint64(1)).astype(np.int64)
        n = h % 32 - 16 + carry
        sign = np.where(h >> 5 & 1, -1.0, 1.0)
        k, k16, m = (h >> 6) % 16 - 8, (h >> 6) % 8 - 3, (h >> 10) % 4096
        a = (h >> 22) % 128 - 64 + carry
        two = np.float64(2.0)
        results = [  # (operation bit, word, value bits); every value is exact in float64
            (0, 0, f32_bits(two ** n)), (1, 0, f32_bits(n)), (2, 0, f32_bits(sign * two ** -n)),
            (3, 0, f32_bits(two ** -k)), (4, 0, f32_bits(m)),
            (5, 1, f32_bits(sin_of[a % 4])), (6, 1, f32_bits(sin_of[(a + 1) % 4])),
            (7, 2, f64_word(sign * two ** -n)), (8, 2, f64_word(two ** k)), (9, 2, f64_word(two ** -k)),
            (10, 3, f16_bits(two ** -k)), (11, 3, f16_bits(two ** k16)), (12, 3, f16_bits(two ** -k16))]
        for op, word, bits in results:
            if ops >> op & 1:
                g[word] = fold(g[word], bits)
    return np.array(g).T


def ref_f64(seed, iters):
    out = np.zeros((256, 4), dtype=np.uint64)
    x = (H(seed, 0x340, T) >> np.uint64(6)).astype(np.int64)
    total = np.zeros(256, dtype=np.int64)
    g = [np.zeros(256, dtype=np.uint64) for _ in range(4)]
    for s in range(iters * 8):
        h1 = H(seed, 0x341, 2 * (256 * s + T)).astype(np.int64)
        h2 = H(seed, 0x341, 2 * (256 * s + T) + 1).astype(np.int64)
        a, b = h1 % 65536 - 32768, h2 % (1 << 24) - (1 << 23)
        e, c, d = (h1 >> 16) % 4, (h1 >> 18) % 64 + 1, h2 >> 24
        p = x * a + b
        assert np.abs(p).max() < 1 << 42
        total += p
        r8 = p * c * (1 << e) + d                      # eighths; below 2^52
        assert np.abs(r8).max() < 1 << 52
        x = (r8 >> 3) % (1 << 26)                      # numpy's >> and % floor
        trunc = np.sign(p) * (np.abs(p) >> 12)         # conversion rounds toward zero
        g[0] = fold(g[0], f64_word(p.astype(np.float64)))
        g[1] = fold(g[1], f64_word(r8.astype(np.float64) / 8))
        g[2] = fold(g[2], ((x ^ (r8 % 8) << 28) + trunc) % (1 << 32))
    assert np.abs(total).max() < 1 << 53
    g[3] = f64_word(total.astype(np.float64))
    out[:] = np.array(g).T
    return out


def ref_packed(seed, iters):
    acc = [np.zeros(256, dtype=np.int64) for _ in range(2)]
    sdot, udot, fdot, bdot = (np.zeros(256, dtype=np.int64) for _ in range(4))
    g = [np.zeros(256, dtype=np.uint64) for _ in range(4)]

    def s8(v):
        return (v & 255) - 2 * (v & 128)

    def s16(v):
        return (v & 0xFFFF) - 2 * (v & 0x8000)

    for s in range(iters * 16):
        h = [H(seed, 0x350, 4 * (256 * s + T) + q).astype(np.int64) for q in range(4)]
        for i in range(2):
            acc[i] += s8(h[0] >> 8 * i) * s8(h[0] >> 16 + 8 * i)
        fm = ad = ml = np.zeros(256, dtype=np.uint64)
        for i in range(2):
            a, b = (h[1] >> 6 * i) % 64 - 32, (h[1] >> 12 + 6 * i) % 64 - 32
            c = (h[1] >> 24 + 4 * i) % 16 - 8
            assert max(np.abs(a * b + c).max(), np.abs(a * b + c + b).max()) <= 2048
            # float16 arithmetic on these integers is exact, and gives the IEEE sign of a zero
            fa, fb, fc = (v.astype(np.float16) for v in (a, b, c))
            fm = fm | f16_bits((a * b + c).astype(np.float16)) << np.uint64(16 * i)
            ad = ad | f16_bits((a * b + c + b).astype(np.float16)) << np.uint64(16 * i)
            ml = ml | f16_bits(fa * fc) << np.uint64(16 * i)
            fdot += a * b
            bdot += a * c
        g[0] = fold(fold(fold(g[0], fm), ad), ml)
        lo = [(h[2] >> 16 * i) & 0xFFFF for i in range(2)], [(h[3] >> 16 * i) & 0xFFFF for i in range(2)]
        packed = lambda f: sum((f(lo[0][i], lo[1][i]) & 0xFFFF) << 16 * i for i in range(2))  # noqa: E731
        for f in (lambda p, q: p * q, lambda p, q: p + q, lambda p, q: p - q,
                  lambda p, q: np.maximum(s16(p), s16(q)), lambda p, q: np.minimum(p, q)):
            g[1] = fold(g[1], packed(f))
        for i in range(4):
            sdot += s8(h[2] >> 8 * i) * s8(h[3] >> 8 * i)
            udot += (h[2] >> 8 * i & 255) * (h[3] >> 8 * i & 255)
    for v in (*acc, fdot, bdot):
        assert np.abs(v).max() < 1 << 24
    assert np.abs(sdot).max() < 1 << 31 and udot.max() < 1 << 32
    g[2] = (f32_bits(acc[0]) + rotl(f32_bits(acc[1]), 11)) & M32
    g[3] = (sdot % (1 << 32)).astype(np.uint64) ^ rotl(udot, 8) ^ f32_bits(fdot) ^ rotl(f32_bits(bdot), 24)
    return np.array(g).T


REFERENCE = {"xlane": ref_xlane, "regfile": ref_regfile, "salu": ref_salu, "trans": ref_trans,
             "f64": ref_f64, "packed": ref_packed}


@pytest.fixture(scope="module")
def tables():
    """expected() for every test, seed and iters, computed once."""
    return {(t, s, i): lanescan.expected(t, s, i)
            for t in lanescan.ALL_TESTS for s in SEEDS for i in ITERS}


# ---------------------------------------------------------------- the tables
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("test", lanescan.ALL_TESTS)
def test_expected_equals_the_reference(tables, test, seed, iters):
    got = tables[test, seed, iters]
    assert got.shape == (256, 4) and got.dtype == np.uint32
    want = REFERENCE[test](seed, iters).astype(np.uint32)
    print(test, hex(seed), iters, "words that differ:", int((got != want).sum()))
    np.testing.assert_array_equal(got, want)


def test_tables_differ_between_tests_seeds_and_iters(tables):
    flat = {k: v.tobytes() for k, v in tables.items()}
    assert len(set(flat.values())) == len(flat)
    for v in tables.values():
        assert len({bytes(r) for r in v}) == 256          # the threads differ too


def test_one_unit_of_iters_passes_the_whole_menu_once(tables):
    """No prefix property holds between tables: every word folds every step, so the table of
    iters 1 is not part of the table of iters 3. What does hold is on the step sequence: the steps
    of each unit of iters are a permutation of the menu, whatever the seed, and a longer run
    starts with the steps of a shorter one."""
    menu, _ = lanescan.lanes()
    for seed in SEEDS + (5,):
        first = Hi(seed, 0x301, 0) % len(menu)
        steps = [(first + s) % len(menu) for s in range(3 * len(menu))]
        for unit in range(3):
            assert sorted(steps[unit * len(menu):(unit + 1) * len(menu)]) == list(range(len(menu)))
    for t in lanescan.ALL_TESTS:
        assert not (tables[t, 0, 1] == tables[t, 0, 3]).all(axis=1).any()


# ---------------------------------------------------------------- the lane model by hand
def test_dpp_masks_and_bound_ctrl_by_hand():
    old, src = np.arange(1000, 1064, dtype=np.uint64), np.arange(1, 65, dtype=np.uint64)

    def at(out, *lanes):
        return tuple(int(out[l]) for l in lanes)
    assert at(dpp(0x111, 0xF, 0xF, 0, old, src), 0, 16, 1, 17, 63) == (1000, 1016, 1, 17, 63)   # row_shr:1
    assert at(dpp(0x111, 0xF, 0xF, 1, old, src), 0, 16, 32, 1) == (0, 0, 0, 1)
    # rows 0 and 2 only, and of each row only lanes 4..7
    assert at(dpp(0x111, 0x5, 0x2, 1, old, src), 0, 4, 7, 8, 20, 36) == (1000, 4, 7, 1008, 1020, 36)
    assert at(dpp(0x142, 0xA, 0xF, 0, old, src), 5, 16, 31, 32, 48) == (1005, 16, 16, 1032, 48)  # row_bcast:15
    assert at(dpp(0x143, 0xC, 0xF, 0, old, src), 31, 32, 63) == (1031, 32, 32)                   # row_bcast:31
    out = dpp(0x10F, 0xF, 0xF, 1, old, src)              # row_shl:15: only lane 0 has a source
    assert int(out[0]) == 16 and not out[1:16].any()
    out = dpp(0x10F, 0xF, 0xF, 0, old, src)
    assert int(out[0]) == 16 and (out[1:16] == old[1:16]).all()
    assert at(dpp(0x138, 0xF, 0xF, 1, old, src), 0, 16, 63) == (0, 16, 63)                        # wave_shr:1
    assert at(dpp(0x121, 0xF, 0xF, 0, old, src), 0, 16, 1) == (16, 32, 1)                         # row_ror:1
    assert at(swizzle(0x401F, src), 0, 1) == (17, 18) and int(swizzle(0x7C1F, src)[32]) == 64
    assert at(swizzle(0x8039, src), 0, 1, 2, 3) == (2, 3, 4, 1) and at(swizzle(0x0078, src), 8, 9) == (12, 12)


def test_the_menu_covers_what_the_scan_claims():
    menu, ops = lanescan.lanes()
    assert len(menu) == 43 and ops & 0x1FFF == ops
    ctrls = {m["imm"] for m in menu if m["kind"] == 0}
    for lo, hi in ((0, 0xFF), (0x101, 0x10F), (0x111, 0x11F), (0x121, 0x12F)):
        assert any(lo <= c <= hi for c in ctrls)
    assert {0x140, 0x141, 0x142, 0x143, 0x130, 0x134, 0x138, 0x13C} <= ctrls
    dpps = [m for m in menu if m["kind"] == 0]
    assert any(m["row_mask"] != 15 for m in dpps) and any(m["bank_mask"] != 15 for m in dpps)
    assert {m["bound_ctrl"] for m in dpps} == {0, 1}
    swz = [m["imm"] for m in menu if m["kind"] == 1]
    assert any(o & 0x8000 for o in swz) and any(not o & 0x8000 for o in swz)
    assert [m["kind"] for m in menu if m["kind"] > 1] == list(range(34, 43))


# ---------------------------------------------------------------- parsers and refusals
def test_parsers():
    assert lanescan.ALL_TESTS == ("xlane", "regfile", "salu", "trans", "f64", "packed")
    assert (lanescan.DEFAULT_ITERS, lanescan.MAX_ITERS) == (16, 63)
    assert lanescan.parse_tests("xlane, salu") == ("xlane", "salu")
    assert lanescan.parse_inject("any:xlane:0:0:1") == ("any", "xlane", 0, 0, 1)
    assert lanescan.parse_inject("0x123:packed:130:2:0x10000") == (0x123, "packed", 130, 2, 0x10000)
    for bad in ("nope", "xlane,nope", ""):
        with pytest.raises(ProbeError):
            lanescan.parse_tests(bad)
    for bad in ("any:xlane:0:0", "any:nope:0:0:1", "any:xlane:256:0:1", "any:xlane:0:4:1",
                "any:xlane:0:0:0", "4096:xlane:0:0:1", "any:xlane:x:0:1", "any:xlane:0:0:0x100000000"):
        with pytest.raises(ProbeError):
            lanescan.parse_inject(bad)


def test_scan_validates_before_any_hip_call(monkeypatch):
    """Every refusal below is made in Python with the native library unreachable."""
    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    for kw in (dict(tests=()), dict(tests=("xlane", "nope")), dict(tests=64), dict(iters=0),
               dict(iters=lanescan.MAX_ITERS + 1), dict(iters=1.5), dict(iters=True), dict(seed=-1),
               dict(seed=1 << 64), dict(min_rounds=0), dict(min_rounds=3, max_rounds=2),
               dict(max_rounds=1025), dict(_inject=("any", "salu", 0, 0, 0)),
               dict(_inject=("any", "salu", 256, 0, 1)), dict(_inject=("any", "salu", 0, 4, 1)),
               dict(_inject=(4096, "salu", 0, 0, 1)), dict(_inject=("any", "salu", 0, 0)),
               dict(tests=("xlane",), _inject=("any", "salu", 0, 0, 1))):
        with pytest.raises(ProbeError):
            lanescan.scan(0, **kw)
    with pytest.raises(ProbeError):
        lanescan.scan(-1)
    for call in (lambda: lanescan.expected("nope", 0, 1), lambda: lanescan.expected("f64", 0, 0),
                 lambda: lanescan.expected("f64", 0, 64), lambda: lanescan.signature("f64", 0, 0),
                 lambda: lanescan.signature(3, 0, 1), lambda: lanescan.signature("f64", 0, 64)):
        with pytest.raises(ProbeError):
            call()
    with pytest.raises(AssertionError):                  # a good call does get there
        lanescan.scan(0)


def test_native_entry_points_validate_before_selecting_a_device():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    res, n = _native.CuscanResult(), C.c_int(7)
    cus = (_native.CuscanCu * 4)()
    out = (C.c_uint32 * 1024)()
    P, W = C.c_void_p(4096), C.c_void_p(8192)   # never dereferenced: every call is refused first
    for test, iters in ((0, 1), (3, 1), (64, 1), (1, 0), (1, 64), (32, 64)):
        assert lib.gm_probe_lanescan_expected(test, 0, iters, out) == 1
        assert lib.gm_probe_lanescan_signature(test, 0, iters, P, W, None) == 1
    assert lib.gm_probe_lanescan_expected(1, 0, 1, None) == 1
    assert lib.gm_probe_lanescan_expected(32, 0, 63, out) == 0
    for o, w in ((None, W), (P, None), (C.c_void_p(4096 + 4), W), (P, C.c_void_p(8194))):
        assert lib.gm_probe_lanescan_signature(1, 0, 1, o, w, None) == 1
    menu, k, ops = (C.c_uint32 * 320)(), C.c_int(0), C.c_uint32(0)
    assert lib.gm_probe_lanescan_lanes(menu, 64, C.byref(k), C.byref(ops)) == 0 and k.value == 43
    assert lib.gm_probe_lanescan_lanes(menu, 42, C.byref(k), C.byref(ops)) == 1
    assert lib.gm_probe_lanescan_lanes(None, 64, C.byref(k), C.byref(ops)) == 1
    assert lib.gm_probe_lanescan_kernel_info(None, None) == 1

    def scan(mask=63, iters=1, lo=1, hi=1, inj=None, cap=4, table=cus):
        return lib.gm_probe_lanescan(0, mask, iters, 0, lo, hi,
                                     C.byref(inj) if inj is not None else None, C.byref(res),
                                     table, cap, C.byref(n))
    assert scan(mask=0) == 1 and n.value == 0
    assert scan(mask=64) == 1
    assert scan(iters=0) == 1 and scan(iters=64) == 1
    assert scan(lo=0) == 1 and scan(lo=2, hi=1) == 1 and scan(hi=1025) == 1
    assert scan(cap=-1) == 1 and scan(cap=4, table=None) == 1
    inject = _native.CuscanInject
    for inj in (inject(0, 32, 0, 0, 0), inject(0, 6, 0, 0, 1), inject(0, 32, 256, 0, 1),
                inject(0, 32, 0, 4, 1), inject(4096, 32, 0, 0, 1), inject(0, 64, 0, 0, 1)):
        assert scan(inj=inj) == 1
    assert scan(mask=1, inj=inject(0, 32, 0, 0, 1)) == 1         # a test that is not selected
    assert lib.gm_probe_lanescan(0, 63, 1, 0, 1, 1, None, None, cus, 4, C.byref(n)) == 1


# ---------------------------------------------------------------- command lines
def test_command_lines_parse_the_lane_scan_options():
    from gpumounter_amd.cli import build_parser, cmd_probe

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.lane_scan is False and a.lane_scan_inject is None and a.lane_scan_tests is None
    assert a.lane_scan_iters is None and a.lane_scan_rounds is None
    a = ap.parse_args(["probe", "--lane-scan", "--lane-scan-tests", "xlane,trans",
                       "--lane-scan-iters", "3", "--lane-scan-rounds", "2", "--lane-scan-inject",
                       "any:trans:0:0:1"])
    assert a.lane_scan and tuple(a.lane_scan_tests) == ("xlane", "trans")
    assert a.lane_scan_iters == 3 and a.lane_scan_rounds == 2
    assert a.lane_scan_inject == ("any", "trans", 0, 0, 1)
    for bad in (["--lane-scan-tests", "xlane,nope"], ["--lane-scan-inject", "any:xlane:0:0"],
                ["--lane-scan-inject", "any:xlane:0:0:0"], ["--lane-scan-iters", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--lane-scan", *bad])
    # usage errors (2), not a failed scan (1), before any GPU work
    assert cmd_probe(ap.parse_args(["probe", "--lane-scan-inject", "any:xlane:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--lane-scan-iters", "3"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--lane-scan", "--lane-scan-tests", "salu",
                                    "--lane-scan-inject", "any:xlane:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--lane-scan", "--lane-scan-iters", "64"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--lane-scan", "--lane-scan-rounds", "0"])) == 2
    d = ap.parse_args(["doctor", "--gpu", "--lane-scan", "--lane-scan-inject", "any:f64:1:2:4"])
    assert d.lane_scan is True and d.lane_scan_inject == ("any", "f64", 1, 2, 4)
    assert ap.parse_args(["doctor", "--gpu"]).lane_scan is False


def test_probe_passes_the_options_on(monkeypatch, capsys):
    from gpumounter_amd.cli import build_parser, cmd_probe
    from gpumounter_amd.ops import probe

    class Res:
        def to_dict(self):
            return {"device": 0}
    calls = []

    def fake_scan(dev, **kw):
        calls.append((dev, kw))
        return {"ok": kw["_inject"] is None}
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Res()])
    monkeypatch.setattr(lanescan, "scan", fake_scan)
    ap = build_parser()
    assert cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--lane-scan"])) == 0
    assert calls[-1] == (0, dict(tests=lanescan.ALL_TESTS, iters=16, min_rounds=1, max_rounds=16,
                                 _inject=None))
    assert cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--lane-scan",
                                    "--lane-scan-tests", "packed", "--lane-scan-iters", "63",
                                    "--lane-scan-rounds", "20", "--lane-scan-inject",
                                    "any:packed:0:0:1"])) == 1
    assert calls[-1] == (0, dict(tests=("packed",), iters=63, min_rounds=20, max_rounds=20,
                                 _inject=("any", "packed", 0, 0, 1)))
    assert '"lanescan"' in capsys.readouterr().out


def test_validate_parses_the_lane_scan_options():
    from gpumounter_amd.parallel import validate

    with pytest.raises(SystemExit):
        validate.main(["--lane-scan-inject", "any:xlane:0:0:1"])         # needs --lane-scan
    with pytest.raises(SystemExit):
        validate.main(["--lane-scan", "--lane-scan-inject", "any:nope:0:0:1"])


def test_doctor_passes_the_scan_on_and_names_the_unit_and_test(monkeypatch):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["lane_scan"].default is False and sig["lane_scan"].kind is sig["lane_scan"].KEYWORD_ONLY
    assert sig["lane_scan_inject"].default is None
    assert inspect.signature(doctor.run).parameters["lane_scan"].default is False

    calls = []

    def fake_scan(dev, _inject=None):
        calls.append((dev, _inject))
        bad = _inject is not None
        failed = [{"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "runs": 1, "failed_runs": 1,
                   "tests_failed": ["regfile"], "simds_failed": [2]}] if bad else []
        return {"tests": list(lanescan.ALL_TESTS), "cus_seen": 250, "cus_expected": 256,
                "complete": False, "rounds": 16, "kernel_ms": 1.0, "words_in_error": int(bad),
                "ok": not bad, "failed": failed}
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(lanescan, "scan", fake_scan)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "lane-scan" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, lane_scan=True) if c.name == "gpu0"]
    assert ok.status == "ok" and "lane-scan 6 tests 250/256 CUs" in ok.detail      # stated, not failed
    assert "incomplete" in ok.detail and " 0 wrong words" in ok.detail
    inj = (0x123, "regfile", 130, 2, 0x10000)
    (bad,) = [c for c in doctor.check_gpus(cfg, lane_scan=True, lane_scan_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail" and bad.detail.endswith("xcc 1 se 1 sh 0 cu 3 (id 0x123) simd 2 regfile")
    assert calls == [(0, None), (0, inj)]


def test_the_result_decoder_is_shared_with_the_cu_scan():
    unit = {"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "simds_failed": [1, 3],
            "tests_failed": ["xlane", "trans"]}
    assert lanescan.describe_failed({"failed": [unit]}) == (
        "xcc 2 se 1 sh 0 cu 5 (id 0x225) simd 1,3 xlane+trans")
    assert cuscan.describe_failed({"failed": [unit]}) == lanescan.describe_failed({"failed": [unit]})
