"""What the post-attach validation kernels do to data, on the MI355X (``pytest -m gpu``): the
burn-in's difference counter and its negative control, the operand fill, the seven HBM copy
variants, the read stream and the 256²-tile GEMM, each on caller-owned buffers through the entry
points the shipped drivers call (native/include/gm_probe.h). Every comparison is exact; no rate is
asserted. Nothing here holds more than a few tens of MiB, except the two command-line cases that
run the default 8192² burn-in.

Geometry the shapes rely on:
* k_count_diff: 2048 blocks × 256 threads, grid-stride over 16-byte words (footprint 8 MiB);
* k_fill_bf16: 4096 blocks × 256 threads, grid-stride over bf16 elements;
* copy: CUs × blocks_per_cu blocks, each a contiguous chunk rounded up to 1024 elements of 16 B,
  walked in steps of 4 × 256 or 8 × 256 (chunked) or 4 × 256 or 2 × 256 (pipelined), then a
  256-element tail loop;
* read: the same with chunks rounded up to 2048 elements, steps of 8 × 256;
* gemm_nt: 256² tiles, K-tiles of 64, tile rows grouped 8 deep, block ids dealt over 8 XCDs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import probe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a host without a GPU")


def _rand_i32(n: int, seed: int):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-2**31, 2**31, (n,), dtype=torch.int64, device=DEV,
                         generator=g).to(torch.int32)


# ------------------------------------------------------------------ liveness probe
def test_quick_raw_words_are_the_expected_table():
    words, salt = probe.quick_words(0)
    assert salt == 0x9E3779B9                       # device 0
    want = probe.quick_expected(salt)
    bad = [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(words, want)) if g != w]
    assert not bad, bad
    assert words[65] == 64 and probe.quick_verdict(words, salt) == 0


def test_quick_negative_control_fails_each_check_and_leaves_nothing_behind():
    assert probe.quick(0) < 1e6
    for flip, name in (((0, 0x1), "lane words"), ((63, 0x80000000), "lane words"),
                       ((37, 0xFFFFFFFF), "lane words"), ((64, 0x1), "reduction sum"),
                       ((64, 0x80000000), "reduction sum"), ((65, 0x40), "ballot count"),
                       ((65, 0x60), "ballot count")):        # 64 ^ 0x60 = 32: a wave32 answer
        with pytest.raises(probe.ProbeError, match=rf"wrong results \({name}\)"):
            probe.quick(0, _flip=flip)
        # the flip touched the host copy of that run only: the cached scratch serves a clean run
        assert probe.quick(0) < 1e6
        assert probe.quick_words(0)[0] == probe.quick_expected(0x9E3779B9)
    for flip in ((66, 1), (0, 0)):
        with pytest.raises(probe.ProbeError, match="hip error 1 "):
            probe.quick(0, _flip=flip)
    assert probe.quick(0) < 1e6


# ------------------------------------------------------------------ MFMA peak kernels' values
# The reference is written from the kernel source (native/hip/gm_probe.hip) and the lane maps in
# gm_probe.h: per wave and chain one tile product, accumulated `iters` times.
PEAK_BLOCKS = 3                                  # blockIdx enters b of the 16x16x32 kernels
PEAK_GUARD, PEAK_SENTINEL = 1024, -12345.0       # floats on each side of the output
PEAK_CHAINS = ("ab", "ba", "aa", "bb")
_peak_cache = {}


def _bf16_rne(x: np.ndarray) -> np.ndarray:
    """float32 → bf16 (round to nearest even) → the value as float64."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    bits = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)
    return (bits << np.uint32(16)).view(np.float32).astype(np.float64)


def _peak_lane_operands(variant: int, block: int, seed: float):
    """a[t][j], b[t][j] of the 256 threads of one block, as the kernels form them."""
    t = np.arange(256)[:, None]
    j = np.arange(8)[None, :]
    if variant == 0:
        na, nb = t + j, np.broadcast_to(j + 1, (256, 8))
    else:
        na, nb = t * 7 + j, np.broadcast_to(j * 3 + 1 + block, (256, 8))
    s = np.float32(seed)
    return _bf16_rne(s * na.astype(np.float32)), _bf16_rne(s * nb.astype(np.float32))


def _peak_terms(variant: int, seed: float):
    """For one iteration: terms[block, thread, chain, register, k], the K products a·b that the
    register's output element sums (float64, exact: two bf16 factors)."""
    key = (variant, float(np.float32(seed)))
    if key in _peak_cache:
        return _peak_cache[key]
    rows, shift, regs = (32, 5, 16) if variant == 0 else (16, 4, 4)
    kdim = 8 * (64 >> shift)
    nchains = 8 if variant == 2 else 4
    lane = np.arange(64)
    out = np.zeros((PEAK_BLOCKS, 256, nchains, regs, kdim))
    for blk in range(PEAK_BLOCKS):
        a, b = _peak_lane_operands(variant, blk, seed)
        for w in range(4):
            ops = {"a": a[64 * w:64 * w + 64], "b": b[64 * w:64 * w + 64]}
            for ch in range(nchains):
                x, y = (ops[c] for c in PEAK_CHAINS[ch % 4])
                A, B = np.zeros((rows, kdim)), np.zeros((kdim, rows))
                for j in range(8):
                    A[lane & (rows - 1), 8 * (lane >> shift) + j] = x[:, j]
                    B[8 * (lane >> shift) + j, lane & (rows - 1)] = y[:, j]
                terms = A[:, :, None] * B[None, :, :]             # [row, k, col]
                for i in range(regs):
                    row = ((i & 3) + 8 * (i >> 2) + 4 * (lane >> 5) if variant == 0
                           else 4 * (lane >> 4) + i)
                    out[blk, 64 * w + lane, ch, i, :] = terms[row, :, lane & (rows - 1)]
    _peak_cache[key] = out
    return out


def _peak_run(variant: int, iters: int, seed: float) -> np.ndarray:
    """One values launch between sentinel guards; asserts the guards, returns the values."""
    per = probe.MFMA_PEAK_FLOATS[variant]
    n = PEAK_BLOCKS * 256 * per
    big = torch.full((n + 2 * PEAK_GUARD,), PEAK_SENTINEL, dtype=torch.float32, device=DEV)
    got = probe.mfma_peak_values(variant, iters, seed, PEAK_BLOCKS,
                                 out=big[PEAK_GUARD:PEAK_GUARD + n])
    assert got.data_ptr() == big.data_ptr() + 4 * PEAK_GUARD
    assert tuple(got.shape) == (PEAK_BLOCKS, 256, per // (16 if variant == 0 else 4),
                                16 if variant == 0 else 4)
    host = big.cpu().numpy()
    assert (host[:PEAK_GUARD] == PEAK_SENTINEL).all(), "guard below the output overwritten"
    assert (host[PEAK_GUARD + n:] == PEAK_SENTINEL).all(), "guard above the output overwritten"
    return host[PEAK_GUARD:PEAK_GUARD + n].reshape(got.shape)


def _assert_peak_exact(variant: int, iters: int):
    terms = _peak_terms(variant, 1.0)
    ints = terms.astype(np.int64)
    assert (ints == terms).all()                                   # seed 1.0: integer terms
    # exact in any accumulation order: every partial sum is a multiple of the lowest set bit
    # among the element's terms and smaller than 2^24 of them
    low = np.where(ints != 0, ints & -ints, np.int64(1) << 62).min(axis=-1).astype(np.float64)
    assert (iters * np.abs(ints).sum(axis=-1) / low < 1 << 24).all(), \
        f"variant {variant}: iters {iters} is not exact in fp32"
    ref = (iters * terms.sum(axis=-1)).astype(np.float32)
    assert (ref.astype(np.float64) == iters * terms.sum(axis=-1)).all()
    got = _peak_run(variant, iters, 1.0)
    wrong = got.view(np.uint32) != ref.view(np.uint32)
    if wrong.any():
        first = tuple(int(v) for v in np.argwhere(wrong)[0])
        pytest.fail(f"variant {variant}, iters {iters}: {int(wrong.sum())} of {wrong.size} "
                    f"accumulator registers wrong; chains hit {sorted(set(np.argwhere(wrong)[:, 2]))}; "
                    f"first [block, thread, chain, register] = {first}: got {got[first]!r}, "
                    f"want {ref[first]!r}")


@pytest.mark.parametrize("variant,iters", [(0, 1), (0, 3), (0, 16), (1, 1), (1, 3), (1, 4),
                                           (2, 1), (2, 3), (2, 4)])
def test_mfma_peak_values_are_exact_on_integer_operands(variant, iters):
    _assert_peak_exact(variant, iters)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_mfma_peak_values_on_the_shipped_operands(variant):
    """seed = 1e-3f as the timed driver passes it. |got − ref| ≤ γ·iters·Σ|a·b| with
    γ = n·u/(1 − n·u), n = K·iters + 1 additions per element, u = 2^-23: the bound for any
    order of additions, each rounded or truncated to fp32. One iteration missed or doubled is
    off by 1/50 of Σ|a·b| where the terms share a sign (they all do: the operands are positive)."""
    iters, seed = 50, np.float32(1e-3)
    terms = _peak_terms(variant, seed)
    kdim = terms.shape[-1]
    n, u = kdim * iters + 1, 2.0 ** -23
    gamma = n * u / (1 - n * u)
    ref = iters * terms.sum(axis=-1)
    bound = gamma * iters * np.abs(terms).sum(axis=-1)
    assert gamma < 4e-4 and (np.abs(ref) > 50 * bound).all()    # a lost iteration is far outside
    got = _peak_run(variant, iters, float(seed)).astype(np.float64)
    err = np.abs(got - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"variant {variant}: max |err|/bound = {(err / bound).max():.3g}")
    assert (err <= bound).all(), (f"[block, thread, chain, register] = {worst}: got {got[worst]}, "
                                  f"want {ref[worst]}, bound {bound[worst]}")


def test_mfma_peak_values_still_match_after_a_timed_run():
    """The rate and the values meet: the timed driver leaves nothing behind that a values
    launch of the kernel it times (variant 2) could see."""
    assert probe.mfma_tflops(0, 2000) > 0
    _assert_peak_exact(2, 3)


# ------------------------------------------------------------------ 64² tile GEMM on exact data
GEMM64_SHAPES = [(64, 64, 32),       # one block, one K-tile
                 (64, 192, 64),      # bn runs, bm does not
                 (192, 64, 96),      # the reverse, with an odd number of K-tiles
                 (128, 192, 160)]    # both run, the grid is not square
GEMM64_GUARD = 64


def _gemm64_guarded(a, b, ref):
    """Runs gemm_bf16 into a C between NaN guard rows; asserts C fully written, equal to ref bit
    for bit, and the guards untouched."""
    m, n = ref.shape
    big = torch.full((m + 2 * GEMM64_GUARD, n), float("nan"), dtype=torch.float32, device=DEV)
    nan_bits = big[:GEMM64_GUARD].view(torch.int32).clone()
    out = big[GEMM64_GUARD:GEMM64_GUARD + m]
    got = probe.gemm_bf16(a, b, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    unwritten = torch.isnan(out)
    if unwritten.any():
        tiles = sorted({(r // 64, c // 64) for r, c in unwritten.nonzero()[:4096].tolist()})
        pytest.fail(f"{int(unwritten.sum())} elements of C never written, in tiles {tiles}")
    wrong = out.view(torch.int32) != ref.view(torch.int32)
    assert not wrong.any(), (f"{int(wrong.sum())} wrong elements, first at "
                             f"{wrong.nonzero()[0].tolist()}")
    assert torch.equal(big[:GEMM64_GUARD].view(torch.int32), nan_bits)
    assert torch.equal(big[GEMM64_GUARD + m:].view(torch.int32), nan_bits)


@pytest.mark.parametrize("m,n,k", GEMM64_SHAPES)
def test_gemm_bf16_is_exact_on_small_integers_and_stays_inside_c(m, n, k):
    """Integer operands in [-3, 3]: every partial sum is an integer of magnitude ≤ 9·K < 2^24,
    exact in fp32 in any order, so C is the double product cast to fp32."""
    g = torch.Generator(device=DEV).manual_seed(m * 31 + n * 7 + k)
    a = torch.randint(-3, 4, (m, k), device=DEV, generator=g).to(torch.bfloat16)
    b = torch.randint(-3, 4, (k, n), device=DEV, generator=g).to(torch.bfloat16)
    assert 9 * k < 1 << 24
    ref = (a.double() @ b.double()).to(torch.float32)
    assert ref.abs().max() > 0
    _gemm64_guarded(a, b, ref)


def test_gemm_bf16_routes_every_row_of_b_through_a_permutation():
    """A = a 64-row permutation matrix spread over K = 96 columns (32 of them empty), B with
    12288 distinct bf16 entries: C[i] must be row perm[i] of B, bit for bit. Any slip in the
    fragment maps, the two 8-wide k halves of a lane group included, pairs a row of A with the
    wrong row of B, and no two rows or entries of B look alike."""
    m, n, k = 64, 128, 96
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(96))[:m]
    assert len(set(perm.tolist())) == m and set((perm // 8 % 2).tolist()) == {0, 1}
    a = torch.zeros(m, k, dtype=torch.bfloat16)
    a[torch.arange(m), perm] = 1.0
    # bit patterns 0x3000 .. 0x5FFF: distinct, positive, finite and normal bf16 values
    bits = (0x3000 + torch.arange(k * n, dtype=torch.int32)).to(torch.int16).view(k, n)
    b = bits.view(torch.bfloat16)
    assert bits.max() < 0x7F80 and torch.unique(b.float()).numel() == k * n
    ref = b.float()[perm]
    _gemm64_guarded(a.to(DEV), b.to(DEV).contiguous(), ref.to(DEV))


def test_gemm_bf16_refuses_a_wrong_out_on_the_device():
    a = torch.zeros(64, 32, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(32, 64, dtype=torch.bfloat16, device=DEV)
    for out in (torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV),
                torch.zeros(64, 32, dtype=torch.float32, device=DEV),
                torch.zeros(64, 128, dtype=torch.float32, device=DEV)[:, ::2],
                torch.zeros(64, 64, dtype=torch.float32)):
        with pytest.raises(probe.ProbeError, match="out must be"):
            probe.gemm_bf16(a, b, out=out)


# ------------------------------------------------------------------ difference counter
GRID = 2048 * 256                       # threads of k_count_diff = words per grid-stride sweep
DIFF_SIZES = (16, 4096 - 16, (32 << 20) + 4112)
_diff_cache = {}


def _diff_base(nbytes: int):
    """One random buffer per size, shared by every case and never written."""
    if nbytes not in _diff_cache:
        _diff_cache[nbytes] = _rand_i32(nbytes // 4, nbytes)
    return _diff_cache[nbytes]


def _flip_sets(n: int):
    """name → [(word, 32-bit lane, mask)] for a buffer of n 16-byte words; positions past the
    buffer are left out, so the small sizes keep the cases that fit."""
    rng = np.random.default_rng(n)
    many = rng.choice(n, size=min(1000, n), replace=False)
    sets = {
        "first_and_last": [(0, 0, 0x1), (n - 1, 3, 0x80000000)],
        "two_lanes_of_one_word": [(n // 2, 0, 0x10), (n // 2, 2, 0x10)],
        "each_lane": [(n // 5 + k, k, 1 << (7 * k)) for k in range(4)],
        "wave_boundary": [(63, 1, 0x2), (64, 2, 0x4)],
        "block_boundary": [(255, 3, 0x8), (256, 0, 0x100)],
        "grid_stride_wrap": [(GRID - 1, 1, 0x40), (GRID, 2, 0x4000)],
        "last_sweep": [(4 * GRID, 0, 0x1), (n - 2, 1, 0x1)],
        "many": [(int(w), int(w) % 4, 1 << (int(w) % 31)) for w in many],
    }
    return {k: [(w, l, m) for w, l, m in v if 0 <= w < n] for k, v in sets.items()}


@pytest.mark.parametrize("nbytes", DIFF_SIZES)
def test_count_diff_counts_exactly_the_words_that_differ(nbytes):
    n = nbytes // 16
    a = _diff_base(nbytes)
    b = a.clone()
    assert probe.count_diff(a, b) == 0
    assert probe.count_diff(a, a) == 0
    ran = 0
    for name, flips in _flip_sets(n).items():
        if not flips:
            continue
        b.copy_(a)
        words = torch.tensor([w for w, _, _ in flips], device=DEV)
        lanes = torch.tensor([l for _, l, _ in flips], device=DEV)
        masks = torch.tensor([m - (1 << 32) if m >= 1 << 31 else m for _, _, m in flips],
                             dtype=torch.int32, device=DEV)
        # index_put_ with accumulate would add; distinct (word, lane) pairs make plain XOR safe
        assert len({(w, l) for w, l, _ in flips}) == len(flips)
        v = b.view(-1, 4)
        v[words, lanes] = v[words, lanes] ^ masks
        want = len({w for w, _, _ in flips})
        got = probe.count_diff(b, a)
        assert got == want, f"{name} at {nbytes} B: counted {got}, {want} words differ"
        assert probe.count_diff(a, b) == want, f"{name} at {nbytes} B, operands swapped"
        ran += 1
    assert ran >= 3                      # even 16 bytes keep the cases on word 0
    if n > 4 * GRID:
        assert ran == 8                  # the large size runs every case


@pytest.mark.parametrize("nbytes", DIFF_SIZES)
def test_count_diff_when_every_word_differs(nbytes):
    """One flipped bit in every 16-byte word, the lane rotating with the word index."""
    n = nbytes // 16
    a = _diff_base(nbytes)
    b = a.clone()
    idx = torch.arange(n, device=DEV)
    v = b.view(-1, 4)
    v[idx, idx % 4] = v[idx, idx % 4] ^ 0x10000
    assert probe.count_diff(a, b) == n


# ------------------------------------------------------------------ burn-in negative control
BURN_N, BURN_S = 512, 0.05
LAST = BURN_N * BURN_N - 1


def test_burn_in_without_flips_counts_nothing():
    r = probe.burn_in(0, seconds=BURN_S, n=BURN_N)
    assert r["iterations"] >= 8 and r["iterations"] % 8 == 0, r
    assert r["mismatches"] == 0 and r["ok"] is True, r
    assert "flipped_words" not in r


def test_burn_in_counts_one_flipped_word_in_every_iteration():
    r = probe.burn_in(0, seconds=BURN_S, n=BURN_N, _flips=[(12345, 0x0001)])
    assert r["iterations"] >= 8, r
    assert r["mismatches"] == r["iterations"], r
    assert r["ok"] is False and r["flipped_words"] == 1, r


def test_burn_in_counts_distinct_words_not_flipped_elements():
    """Elements 0 and 1 share a 16-byte word; 8 and n² − 1 are two more."""
    flips = [(0, 0x8000), (1, 0x0001), (8, 0x0100), (LAST, 0x7fff)]
    r = probe.burn_in(0, seconds=BURN_S, n=BURN_N, _flips=flips)
    assert r["iterations"] >= 8, r
    assert r["mismatches"] == 3 * r["iterations"], r
    assert r["ok"] is False and r["flipped_words"] == 3, r
    json.dumps(r)


def test_burn_in_refuses_bad_flips():
    lib = _native.probe()
    for flips in ([(LAST + 1, 1)], [(0, 0)], [(0, 1 << 16)], [(-1, 1)], [(5, 1), (5, 2)]):
        with pytest.raises(probe.ProbeError):
            probe.burn_in(0, seconds=BURN_S, n=BURN_N, _flips=flips)
    # and the C entry point itself, which the wrapper's own checks shield
    import ctypes as C
    tf, bad, it = C.c_double(0), C.c_uint64(0), C.c_int(0)
    out = (C.byref(tf), C.byref(bad), C.byref(it))
    for elems, masks in (([LAST + 1], [1]), ([0], [0]), ([5, 5], [1, 2])):
        fe, fm = (C.c_uint64 * len(elems))(*elems), (C.c_uint16 * len(elems))(*masks)
        assert lib.gm_probe_burn_in_flip(0, BURN_N, BURN_S, len(elems), fe, fm, *out) == 1
    assert lib.gm_probe_burn_in_flip(0, BURN_N, BURN_S, 1, None, None, *out) == 1
    assert lib.gm_probe_burn_in_flip(0, BURN_N, BURN_S, -1, None, None, *out) == 1


def _cli(*args, env=None):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=180,
                          env={**os.environ, **(env or {})})


def test_probe_cli_burn_in_flip_fails():
    res = _cli("probe", "--burn-in", "1", "--burn-in-flip", "0:0x1", "--burn-in-flip", "1:0x8000",
               "--burn-in-flip", "4096:0x10")
    assert res.returncode == 1, (res.stdout[-2000:], res.stderr[-2000:])
    out = json.loads(res.stdout)
    assert out
    for r in out:
        b = r["burn_in"]
        assert b["ok"] is False and b["iterations"] >= 8, b
        assert b["mismatches"] == 2 * b["iterations"], b


def test_doctor_reports_a_flipped_burn_in_as_failed():
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    cfg = Config.load(env={}, amdsmi_lib="mock")
    checks = [c for c in doctor.check_gpus(cfg, burn_in_s=1.0, burn_in_flip=[(77, 0x4000)])
              if c.name != "gpu"]
    assert checks
    for c in checks:
        m = re.search(r" (\d+) mismatching words", c.detail)
        assert c.status == "fail" and m and int(m.group(1)) >= 8, c


# ------------------------------------------------------------------ operand fill
def _fill_reference(n: int, seed: int) -> np.ndarray:
    """bf16 bit patterns of k_fill_bf16 in numpy: the hash in wrapping uint32 arithmetic, the
    value exact in fp32 (a 24-bit integer times 2^-23, minus 1), then round-to-nearest-even."""
    u32 = np.uint32
    h = (np.arange(n, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(u32)
    h = (h * u32(2654435761)) ^ u32(seed)
    h ^= h >> u32(15)
    h *= u32(2246822519)
    h ^= h >> u32(13)
    f = (h >> u32(8)).astype(np.float32) * np.float32(2.0 / 16777216.0) - np.float32(1.0)
    u = f.view(u32)
    return ((u + (u32(0x7FFF) + ((u >> u32(16)) & u32(1)))) >> u32(16)).astype(np.uint16)


def _bf16_value(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


@pytest.mark.parametrize("seed", [0x5151, 0xA3A3C0DE])
def test_fill_bf16_matches_the_documented_hash(seed):
    guard, sentinel = 64, 0x7E57
    for n in (1, 255, 4096 * 256 + 3):
        t = torch.full((n + 2 * guard,), sentinel, dtype=torch.int16, device=DEV)
        probe.fill_bf16(t[guard:guard + n], seed)
        got = t.cpu().numpy().view(np.uint16)
        want = _fill_reference(n, seed)
        np.testing.assert_array_equal(got[guard:guard + n], want, err_msg=f"n={n} seed={seed:#x}")
        assert (got[:guard] == sentinel).all() and (got[guard + n:] == sentinel).all(), n
        vals = _bf16_value(got[guard:guard + n])
        assert vals.min() >= -1.0 and vals.max() <= 1.0, (n, vals.min(), vals.max())
    # the range is closed at both ends: about one value in 2^10 lies within half a bf16 step of
    # 1 and rounds up to exactly 1.0, so "[-1, 1)" would be wrong
    assert (vals == 1.0).any() and (vals == -1.0).any()


def test_fill_bf16_is_the_same_through_a_bf16_tensor():
    t = torch.zeros(4099, dtype=torch.bfloat16, device=DEV)
    probe.fill_bf16(t, 7)
    np.testing.assert_array_equal(t.view(torch.int16).cpu().numpy().view(np.uint16),
                                  _fill_reference(4099, 7))


# ------------------------------------------------------------------ copy variants
GUARD, SENTINEL = 4096, 0xA5
_src_cache = {}


def _cus() -> int:
    return probe.props(0)["cu_count"]


def _big_elems() -> int:
    """With one block per CU every chunk is 3072 elements: the 4-deep loop runs three times, the
    8-deep one once and then the tail, the pipelined ones prologue, steady state and epilogue;
    the last block is partial and ends on a lone element."""
    return (_cus() - 1) * 3072 + 2305


def _copy_cases():
    return [(1, 8), (255, 8), (257, 8), (3 * 1024 + 1, 8), (_big_elems(), 1)]


def _src(elems: int):
    """Random bytes per size, shared by all variants; a second copy proves nobody wrote them."""
    if elems not in _src_cache:
        g = torch.Generator(device=DEV).manual_seed(elems)
        s = torch.randint(0, 256, (elems * 16,), dtype=torch.uint8, device=DEV, generator=g)
        _src_cache[elems] = (s, s.clone())
    return _src_cache[elems]


def test_copy_geometry_of_the_large_case():
    elems, b = _big_elems(), _cus()
    per_block = -(-(-(-elems // b)) // 1024) * 1024
    assert per_block == 3072 and elems - (b - 1) * per_block == 2305
    assert elems * 16 < 64 << 20


@pytest.mark.parametrize("variant", range(7))
def test_copy_variant_moves_every_byte_once_and_nothing_else(variant):
    for elems, bpc in _copy_cases():
        nbytes = elems * 16
        src, src_copy = _src(elems)
        big = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        dst = big[GUARD:GUARD + nbytes]
        probe.copy(variant, src, dst, blocks_per_cu=bpc)
        what = f"variant {variant}, {elems} elements, {bpc} blocks/CU"
        if not torch.equal(dst, src):
            bad = (dst != src).nonzero().flatten()
            pytest.fail(f"{what}: {bad.numel()} bytes differ, first at {bad[0].item()} "
                        f"(element {bad[0].item() // 16}), last at {bad[-1].item()}")
        assert (big[:GUARD] == SENTINEL).all() and (big[GUARD + nbytes:] == SENTINEL).all(), what
        assert torch.equal(src, src_copy), what


def test_copy_refuses_unknown_variants_and_ragged_sizes():
    import ctypes as C

    src, _ = _src(257)
    dst = torch.empty_like(src)
    for variant in (7, -1):
        with pytest.raises(probe.ProbeError):
            probe.copy(variant, src, dst)
    with pytest.raises(probe.ProbeError):
        probe.copy(2, src[:24], dst[:24])
    lib = _native.probe()
    s, d = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    assert lib.gm_probe_copy(2, s, d, 24, 8, None) == 1          # not truncated to 16
    assert lib.gm_probe_copy(2, s, d, 0, 8, None) == 1
    assert lib.gm_probe_copy(2, s, d, 64, 0, None) == 1
    assert lib.gm_probe_copy(7, s, d, 64, 8, None) == 1
    assert lib.gm_probe_copy(2, s, C.c_void_p(src.data_ptr() + 32), 64, 8, None) == 1   # overlap
    assert lib.gm_probe_copy(2, C.c_void_p(src.data_ptr() + 8), d, 64, 8, None) == 1
    g = C.c_double(0)
    assert lib.gm_probe_hbm_copy_variant(0, 7, 1 << 20, 1, 8, C.byref(g)) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------ read stream
MAGIC = probe.READ_MAGIC


def _read_geometry(elems: int, bpc: int):
    blocks = _cus() * bpc
    per_block = -(-(-(-elems // blocks)) // 2048) * 2048
    return blocks, per_block


def _in_tail_loop(length: int, e: int) -> bool:
    """Whether element e of a block of `length` elements is read by the 256-stride tail loop:
    thread e % 256 runs the 8-deep loop from i while i + 7·256 < length, in steps of 2048."""
    i = e % 256
    while i + 7 * 256 < length:
        i += 2048
    return e >= i


def _run_read(elems: int, bpc: int, plants):
    """Zero buffer with MAGIC planted at [(element, lane)]; returns the sink as uint32."""
    buf = torch.zeros(elems * 4, dtype=torch.int32, device=DEV)
    sink = torch.zeros(probe.READ_SINK_WORDS, dtype=torch.int32, device=DEV)
    for e, lane in plants:
        buf[4 * e + lane] = MAGIC - (1 << 32)
    probe.read(buf, sink, blocks_per_cu=bpc)
    return sink.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("bpc", [2, 1])
def test_read_stream_reads_every_word_once(bpc):
    elems = _big_elems()
    blocks, per_block = _read_geometry(elems, bpc)
    last_block = (elems - 1) // per_block
    last_len = elems - last_block * per_block
    assert per_block % 2048 == 0 and 1 <= last_block < blocks and 0 < last_len < per_block
    # a tail-loop element: in the partial last block, the first one the 8-deep loop leaves
    # (full blocks are a whole number of 8-deep steps and have no tail)
    tails = [e for e in range(last_len - 1) if _in_tail_loop(last_len, e)]
    assert tails, f"a last block of {last_len} elements has no tail loop"
    tail = tails[0]
    main = per_block + 3 * 256 + 17           # block 1 is full: its first 2048 are the 8-deep loop
    assert not _in_tail_loop(per_block, main - per_block)
    cases = {
        "first word": (0, 0),
        "8-deep loop": (main, 2),
        "tail loop": (last_block * per_block + tail, 1),
        "last word of the partial last block": (elems - 1, 3),
    }
    for name, (e, lane) in cases.items():
        sink = _run_read(elems, bpc, [(e, lane)])
        want = np.zeros(probe.READ_SINK_WORDS, dtype=np.uint32)
        want[(e // per_block) & 1023] = MAGIC
        np.testing.assert_array_equal(sink, want, err_msg=f"{name}: element {e} lane {lane}, "
                                      f"{blocks} blocks of {per_block}")
    # nothing planted: nothing stored
    assert not _run_read(elems, bpc, []).any()
    # The fold is per thread: two plants that one thread of a block reads (256 elements apart,
    # or two lanes of one element) cancel. A word read an even number of times looks like this.
    for pair in ([(main, 2), (main + 256, 0)], [(main, 0), (main, 1)]):
        sink = _run_read(elems, bpc, pair)
        assert not sink.any(), (pair, np.flatnonzero(sink))
    # two threads of one block that each fold to the constant store the same word
    sink = _run_read(elems, bpc, [(main, 2), (main + 5, 0)])
    assert list(np.flatnonzero(sink)) == [1] and sink[1] == MAGIC
    # two plants in different blocks do not
    sink = _run_read(elems, bpc, [(0, 0), (main, 2)])
    assert sorted(np.flatnonzero(sink)) == [0, 1] and (sink[:2] == MAGIC).all()


def test_read_refuses_bad_arguments():
    import ctypes as C

    buf = torch.zeros(1024, dtype=torch.int32, device=DEV)
    sink = torch.zeros(probe.READ_SINK_WORDS, dtype=torch.int32, device=DEV)
    with pytest.raises(probe.ProbeError):
        probe.read(buf, sink[:512])
    with pytest.raises(probe.ProbeError):
        probe.read(buf[:6], sink)
    lib = _native.probe()
    s, k = C.c_void_p(buf.data_ptr()), C.c_void_p(sink.data_ptr())
    assert lib.gm_probe_read(s, k, 24, 2, None) == 1
    assert lib.gm_probe_read(s, None, 64, 2, None) == 1
    assert lib.gm_probe_read(s, k, 64, 0, None) == 1


# ------------------------------------------------------------------ gemm_nt on exact data
GEMM_SHAPES = [(256, 256, 128),      # two K-tiles: V5's stage(1, TK) fires, stage(cur, ..) never
               (256, 256, 192),      # three, an odd depth above 1: V5's stage(cur, (t+2)*TK)
                                     # fires exactly once and the loop ends on buffer 0
               (256, 512, 256),      # four K-tiles, an even depth above 2
               (2560, 512, 64),      # ten tile rows: a full group of 8, then a partial one of 2;
                                     # 20 blocks, not a multiple of the 8 XCDs
               (2304, 256, 128)]     # nine tile rows: a partial group of 1
GUARD_ROWS = 256
_gemm_cache = {}


def _gemm_case(m: int, n: int, k: int):
    """Integer operands in [-3, 3]: every partial sum is an integer of magnitude ≤ 9·K < 2^24,
    exact in fp32 in any order, so the bf16 result is the same as rounding the double product."""
    if (m, n, k) not in _gemm_cache:
        g = torch.Generator(device=DEV).manual_seed(m * 31 + n * 7 + k)
        a = torch.randint(-3, 4, (m, k), device=DEV, generator=g).to(torch.bfloat16)
        bt = torch.randint(-3, 4, (n, k), device=DEV, generator=g).to(torch.bfloat16)
        ref = (a.double() @ bt.double().T).to(torch.bfloat16)
        _gemm_cache[(m, n, k)] = (a, bt, ref)
    return _gemm_cache[(m, n, k)]


@pytest.mark.parametrize("variant", [None, 1, 5])
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_nt256_is_exact_on_small_integers_and_stays_inside_c(m, n, k, variant):
    a, bt, ref = _gemm_case(m, n, k)
    big = torch.full((m + 2 * GUARD_ROWS, n), float("nan"), dtype=torch.bfloat16, device=DEV)
    nan_bits = big[:GUARD_ROWS].view(torch.int16).clone()
    out = big[GUARD_ROWS:GUARD_ROWS + m]
    got = probe.gemm_nt(a, bt, out=out, variant=variant)
    assert got.data_ptr() == out.data_ptr()
    unwritten = torch.isnan(out)
    if unwritten.any():
        tiles = sorted({(r // 256, c // 256) for r, c in unwritten.nonzero()[:4096].tolist()})
        pytest.fail(f"{int(unwritten.sum())} elements of C never written, in tiles {tiles}")
    wrong = out.view(torch.int16) != ref.view(torch.int16)
    assert not wrong.any(), (f"{int(wrong.sum())} wrong elements, first at "
                             f"{wrong.nonzero()[0].tolist()}")
    assert torch.equal(big[:GUARD_ROWS].view(torch.int16), nan_bits)
    assert torch.equal(big[GUARD_ROWS + m:].view(torch.int16), nan_bits)


@pytest.mark.parametrize("variant", [None, 1, 5])
def test_gemm_nt256_is_deterministic_on_the_burn_in_operands(variant):
    """The burn-in compares every result with the first bit for bit; that is only a hardware
    check if two runs on the same operands agree. Operands: the burn-in's own fill, where the
    accumulation order matters."""
    n = 512
    a = probe.fill_bf16(torch.empty(n, n, dtype=torch.bfloat16, device=DEV), 0x5151)
    bt = probe.fill_bf16(torch.empty(n, n, dtype=torch.bfloat16, device=DEV), 0xA3A3)
    first = probe.gemm_nt(a, bt, variant=variant)
    second = probe.gemm_nt(a, bt, out=torch.full_like(first, float("nan")), variant=variant)
    assert not torch.isnan(first).any()
    assert torch.equal(first.view(torch.int16), second.view(torch.int16))
    assert probe.count_diff(first, second) == 0
