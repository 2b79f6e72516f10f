"""The five GEMM kernels on caller-built operands (``pytest -m gpu``): the bf16 256² kernel in its
three schedules, the 64² bf16 kernel and the MX fp8 / fp4 kernels, against the independent
reference of tests/gemm_operands.py. Every expected value comes from there; what each case
covers and that the modelled slips move it is proved without a GPU in tests/test_gemm_operands.py.

Every launch writes into a slice of a larger tensor filled with a NaN sentinel, 256 guard rows
before and after; a check asserts that C is fully written and the guards untouched, that NaN
stands exactly where the reference has it, and that every other compared element is bit-equal
(±inf is an ordinary pattern) or, for the two real-valued cases, within the stated bound.

Shapes are the smallest that take each path: 256² tiles; K-tiles of 64 (bf16), 128 (mxfp8) and
256 (mxfp4) elements; two LDS stages, so three K-tiles is the smallest odd count that uses
buffer 0 again."""
import functools

import numpy as np
import pytest

import gemm_operands as go
from gpumounter_amd.ops import mxgemm, probe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
GUARD = 256
SENTINEL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5}     # NaNs no kernel produces
FORMATS = ("mxfp8", "mxfp4")
KERNELS = (None, 1, 5, "64")          # gemm_nt's default, V1 and V5; the 64² gemm_bf16


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a host without a GPU")


# the cases are built, and their references computed, once per session and never written to
case = functools.lru_cache(maxsize=None)(lambda builder, *args: getattr(go, builder)(*args))


def dev(arr):
    """A numpy array of codes, scales (uint8) or bf16 bits (uint16) on the device."""
    if arr.dtype == np.uint16:
        return torch.from_numpy(arr.view(np.int16).copy()).to(DEV).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)


def guarded(m, n, dtype):
    """(big, out): out the [m, n] slice of a sentinel-filled tensor between its guard rows."""
    ints = torch.int16 if dtype == torch.bfloat16 else torch.int32
    big = torch.full((m + 2 * GUARD, n), SENTINEL[dtype], dtype=ints, device=DEV).view(dtype)
    return big, big[GUARD:GUARD + m]


def read_back(big, out, what):
    """C's bits on the host, after asserting the guards untouched and C fully written."""
    torch.cuda.synchronize()
    ints, np_bits = ((torch.int16, np.uint16) if out.dtype == torch.bfloat16
                     else (torch.int32, np.uint32))
    host = big.view(ints).cpu().numpy().view(np_bits)
    m, sentinel = out.shape[0], SENTINEL[out.dtype]
    assert (host[:GUARD] == sentinel).all(), f"{what}: guard rows before C overwritten"
    assert (host[GUARD + m:] == sentinel).all(), f"{what}: guard rows after C overwritten"
    got = host[GUARD:GUARD + m]
    unwritten = np.argwhere(got == sentinel)
    assert not len(unwritten), (f"{what}: {len(unwritten)} elements of C never written, first "
                                f"{unwritten[:8].tolist()}")
    return got


def is_nan(bits):
    if bits.dtype == np.uint16:
        return (bits & 0x7FFF) > 0x7F80
    return (bits & 0x7FFFFFFF) > 0x7F800000


def value(bits):
    if bits.dtype == np.uint16:
        return go.bf16_table()[bits]
    return bits.view(np.float32).astype(np.float64)


def first_eight(where, got, want):
    return [(int(i), int(j), hex(got[i, j]), hex(want[i, j]) if want is not None else None)
            for i, j in np.argwhere(where)[:8]]


def check(c, e, got, what, bound=None):
    """NaN exactly where the reference has it; every other compared element bit-equal, or within
    ``bound`` for a case that is not exact. Returns max error / bound for the latter."""
    nan = is_nan(got)
    off = (nan != e.nan) & e.compared
    first = [(int(i), int(j), bool(nan[i, j]), bool(e.nan[i, j])) for i, j in np.argwhere(off)[:8]]
    assert not off.any(), (f"{what}: NaN mask differs at {int(off.sum())} elements, first (row, "
                           f"col, got NaN, want NaN): {first}")
    cmp = e.compared & ~e.nan
    if c.exact:
        bad = (got != e.bits) & cmp
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {int(cmp.sum())} compared elements "
                               f"differ, first (row, col, got, want): "
                               f"{first_eight(bad, got, e.bits)}")
        return None
    err, lim = np.abs(value(got) - e.ref), bound(e)
    assert np.all(lim[cmp] > 0)
    ratio = err[cmp] / lim[cmp]
    print(f"{what}: max err / bound = {ratio.max():.4f}, max err / S = "
          f"{(err[cmp] / e.s[cmp]).max():.3e}")
    bad = np.zeros_like(cmp)
    bad[cmp] = ~(ratio <= 1.0)
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements beyond the bound, worst ratio "
                           f"{ratio.max():.4f}, first {first_eight(bad, got, None)}")
    return float(ratio.max())


# ------------------------------------------------------------------ launches
def run_mx(c, traced_r=None):
    a, sa, bt, sb = (dev(x) for x in c.packed())
    big, out = guarded(c.m, c.n, torch.bfloat16)
    if traced_r is None:
        ret = mxgemm.gemm_nt(c.fmt, a, sa, bt, sb, out=out)
    else:
        ret, cus = mxgemm.gemm_nt_traced(c.fmt, a, sa, bt, sb, r=traced_r, out=out)
    assert ret.data_ptr() == out.data_ptr()
    got = read_back(big, out, f"{c.name} r={traced_r}")
    if traced_r is not None:
        assert (cus.cpu().numpy() >= 0).all()
    return got


def run_bf16(c, kernel):
    a, bt = dev(c.a), dev(c.bt)
    if kernel == "64":
        big, out = guarded(c.m, c.n, torch.float32)
        ret = probe.gemm_bf16(a, bt.T.contiguous(), out=out)
    else:
        big, out = guarded(c.m, c.n, torch.bfloat16)
        ret = probe.gemm_nt(a, bt, out=out, variant=kernel)
    assert ret.data_ptr() == out.data_ptr()
    return read_back(big, out, f"{c.name} kernel={kernel}")


def out_of(kernel):
    return "fp32" if kernel == "64" else "bf16"


# ------------------------------------------------------------------ MX kernels
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("which", ("M1", "M2", "M3"))
@pytest.mark.parametrize("path", ("plain", "traced"))
def test_mx_one_hot_cases_are_bit_equal(fmt, which, path):
    """M1: every code pair with A hot; M2: Bt hot; M3: both hot under per-block scales. The
    traced kernel at rotation 0 and at the last one must give the same."""
    c = {"M1": lambda: case("m1", fmt, "a"), "M2": lambda: case("m1", fmt, "b"),
         "M3": lambda: case("m3", fmt)}[which]()
    grid = (c.m // 256) * (c.n // 256)
    for r in [None] if path == "plain" else sorted({0, grid - 1}):
        check(c, c.expected(), run_mx(c, r), f"{c.name} r={r}")


def ieee_bf16_bits(x):
    """float64 → fp32 → bf16, each rounded to nearest even with gradual underflow and overflow to
    infinity: what IEEE arithmetic would give for a one-product result."""
    with np.errstate(over="ignore", under="ignore"):
        f = torch.from_numpy(x.astype(np.float32))
    return f.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_every_scale_byte_in_every_block_position(fmt):
    """M4. Outside the 2^±100 band nothing is asserted; the number of those elements that equal
    the IEEE result is printed."""
    outside = same = 0
    for tile, block in go.m4_positions(fmt):
        c = case("m4", fmt, tile, block)
        e = c.expected()
        got = run_mx(c)
        check(c, e, got, c.name)
        free = ~e.compared
        outside += int(free.sum())
        same += int((got[free] == ieee_bf16_bits(e.ref)[free]).sum())
    print(f"M4 {fmt}: {same} of {outside} elements outside the 2^±100 band equal the IEEE result "
          f"(gradual underflow, overflow to ±inf)")


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_scale_byte_255_makes_its_row_and_column_nan(fmt):
    c = case("m4", fmt, 1, 2, True)
    e = c.expected()
    assert e.nan[77].all() and e.nan[:, 200].all() and e.nan.sum() == 511
    check(c, e, run_mx(c), c.name)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("m,n", ((256, 256), (512, 768)))
def test_mx_dense_exact_operands_are_bit_equal(fmt, m, n):
    """M5: the exact sum rounded once to bf16."""
    c = case("m5", fmt, m, n)
    check(c, c.expected(), run_mx(c), c.name)


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_dense_all_codes_within_the_pipes_allowance(fmt):
    """M6: |C - ref| ≤ 2^-9 · S + 2^-8 · |ref|, the allowance tests/test_mxgemm_gpu.py uses for
    the random class, taken over unchanged."""
    c = case("m6", fmt)
    check(c, c.expected(), run_mx(c), c.name, go.mx_bound)


# ------------------------------------------------------------------ bf16 kernels
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("hot", "ab")
def test_bf16_routes_every_finite_normal_pattern(kernel, hot):
    """B1: a one-hot 1.0 in one operand, all 65024 finite normal patterns and ±0 in the other."""
    c = case("b1", hot, kernel == "64")
    check(c, c.expected(out=out_of(kernel)), run_bf16(c, kernel), f"{c.name} {kernel}")


def test_bf16_subnormal_inputs_are_treated_alike():
    """B1's extra launch: the 254 subnormal patterns. Not asserted which, only that every kernel
    treats every pattern the same way, preserved or flushed to zero, and again on a second run;
    the outcome is printed (docs/FAQ.md records it)."""
    for kernel in KERNELS:
        c = go.b1("a", kernel == "64", patterns=go.BF16_SUBNORMALS)
        want = c.expected(out=out_of(kernel)).bits
        first, second = run_bf16(c, kernel), run_bf16(c, kernel)
        assert np.array_equal(first, second), kernel
        live = want != 0
        if np.array_equal(first, want):
            outcome = "preserved"
        elif not (first & (0x7FFF if first.dtype == np.uint16 else 0x7FFFFFFF)).any():
            outcome = "flushed to zero"
        else:
            pytest.fail(f"kernel {kernel}: subnormal inputs treated unevenly: "
                        f"{int((first[live] == want[live]).sum())} of {int(live.sum())} preserved")
        print(f"bf16 subnormal inputs, kernel {kernel}: {outcome}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_bf16_nan_and_infinity_stay_in_their_row_and_column(kernel):
    """B2."""
    c = case("b2")
    check(c, c.expected(out=out_of(kernel)), run_bf16(c, kernel), f"B2 {kernel}")


@functools.lru_cache(maxsize=None)
def burn_in_fill_case():
    """The burn-in's own operands at n = 512, filled on the device and read back."""
    n, ops = 512, []
    for seed in (0x5151, 0xA3A3):
        t = probe.fill_bf16(torch.empty(n, n, dtype=torch.bfloat16, device=DEV), seed)
        ops.append(t.view(torch.int16).cpu().numpy().view(np.uint16).copy())
    return go.Case("B3-burn-in-fill", "bf16", ops[0], ops[1], exact=False)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("operands", ("burn-in fill", "random"))
def test_bf16_real_valued_operands_within_the_derived_bound(kernel, operands):
    """B3: |C - ref| ≤ (K - 1) · 2^-23 · S + 2^-8 · |ref| (derivation: go.bf16_bound); the second
    term only for the bf16 result."""
    c = burn_in_fill_case() if operands == "burn-in fill" else case("b3_random")
    e = c.expected(out=out_of(kernel))
    assert np.isfinite(e.ref).all() and e.compared.all()
    check(c, e, run_bf16(c, kernel), f"{c.name} {kernel}",
          lambda x: go.bf16_bound(x, c.k, out_of(kernel)))


@pytest.mark.parametrize("kernel", KERNELS)
def test_bf16_epilogue_at_ties_and_the_overflow_edge(kernel):
    """B4: sums that are exact in fp32 and land on ties, their neighbours and the edge of the
    bf16 range, in every accumulator register of both wave rows; the fp32 kernel must return
    them unrounded."""
    c = case("b4")
    check(c, c.expected(out=out_of(kernel)), run_bf16(c, kernel), f"B4 {kernel}")
