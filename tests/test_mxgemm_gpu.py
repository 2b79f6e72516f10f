"""The block-scaled (MX) GEMM burn-in on the MI355X (``pytest -m gpu``): the fill kernel against
the formulas, the GEMM bit for bit against the host's exact result at every K-tile count and grid
shape at which the kernel takes another path, the random class within the pipe's allowance and
deterministic, the burn-in with and without its flip control, and the kernel's scratch use.
Nothing here asserts a rate. K is given in K-tiles: 128 elements for mxfp8, 256 for mxfp4.

Geometry the shapes rely on: 256² tiles, two LDS stages (so 1 tile: no pipelining; 2: one stage
swap; 3: an odd count, the first buffer used again), tile rows grouped 8 deep, block ids dealt
over 8 XCDs (so a grid of 6 and a grid of 9, whose second group holds one tile row)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpumounter_amd.ops import mxgemm, probe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_A, SEED_B = 0x5151, 0xA3A3
EXACT_SHAPES = ((256, 256, 1), (256, 256, 2), (256, 256, 3), (512, 768, 4), (2304, 256, 2))
RANDOM_SHAPE = (512, 512, 8)
BURN_N, BURN_S = 512, 0.05


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a host without a GPU")


@functools.lru_cache(maxsize=None)
def expected(fmt, cls, m, n, k):
    """The host's result, computed once per case and shared; never written to."""
    got = mxgemm.expected(fmt, cls, SEED_A, SEED_B, m, n, k)
    for arr in got if isinstance(got, tuple) else (got,):
        arr.setflags(write=False)
    return got


def run(fmt, cls, m, n, k):
    a, sa = mxgemm.fill(fmt, cls, SEED_A, m, k)
    bt, sb = mxgemm.fill(fmt, cls, SEED_B, n, k)
    return a, sa, bt, sb, mxgemm.gemm_nt(fmt, a, sa, bt, sb)


def bits(c):
    return c.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
@pytest.mark.parametrize("cls", mxgemm.CLASSES)
def test_fill_kernel_writes_the_formulas(fmt, cls):
    """The device fill against the numpy model of tests/test_mxgemm.py, at a size with more bytes
    than the fill's grid has threads (4096 × 256) and a row count that is no power of two."""
    import test_mxgemm as model

    rows, k = 768, 4096
    elems, scales = mxgemm.fill(fmt, cls, SEED_A, rows, k)
    codes = model.codes(fmt, cls, SEED_A, rows, k).astype(np.uint8)
    packed = codes if fmt == "mxfp8" else codes[:, 0::2] | codes[:, 1::2] << 4   # low nibble first
    assert elems.shape == packed.shape and np.array_equal(elems.cpu().numpy(), packed)
    want = model.scales(cls, SEED_A, rows, k // 32).astype(np.uint8)
    assert scales.shape == want.shape and np.array_equal(scales.cpu().numpy(), want)


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
@pytest.mark.parametrize("cls", ("exact", "blocks"))
@pytest.mark.parametrize("m,n,tiles", EXACT_SHAPES)
def test_gemm_is_bit_equal_to_the_hosts_exact_result(fmt, cls, m, n, tiles):
    k = tiles * mxgemm.TILE_K[fmt]
    got, want = bits(run(fmt, cls, m, n, k)[4]), expected(fmt, cls, m, n, k)
    bad = np.argwhere(got != want)
    assert not len(bad), (len(bad), [(int(i), int(j), hex(got[i, j]), hex(want[i, j]))
                                     for i, j in bad[:8]])


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
def test_random_class_is_within_the_pipes_allowance_and_deterministic(fmt):
    """|C - ref| <= 2^-9 * S + 2^-8 * |ref| per element: 2^-9 of the sum of |products| is the
    project's allowance for what the matrix core drops inside its sums (measured 1.0-1.4e-4 of S
    on single instructions), 2^-8 the bf16 rounding of the result."""
    m, n, tiles = RANDOM_SHAPE
    k = tiles * mxgemm.TILE_K[fmt]
    a, sa, bt, sb, c = run(fmt, "random", m, n, k)
    ref, s = expected(fmt, "random", m, n, k)
    err = np.abs(c.float().cpu().numpy().astype(np.float64) - ref)
    bound = 2.0 ** -9 * s + 2.0 ** -8 * np.abs(ref)
    worst = float(np.max(err / bound))
    print(f"mxgemm random {fmt} {m}x{n}x{k}: max error / bound = {worst:.4f}, "
          f"max error / S = {float(np.max(err / s)):.3e}")
    assert np.isfinite(err).all() and worst <= 1.0, worst
    again = mxgemm.gemm_nt(fmt, a, sa, bt, sb)
    assert probe.count_diff(c, again) == 0


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
def test_burn_in_counts_nothing_without_flips_and_every_flipped_word_with(fmt):
    r = mxgemm.burn_in(0, BURN_S, fmt, n=BURN_N)
    assert r["iterations"] >= 1 and r["mismatches"] == 0 and r["ok"] is True, r
    assert r["format"] == fmt and r["n"] == BURN_N and "flipped_words" not in r
    # elements 9 and 15 share a 16-byte word
    r = mxgemm.burn_in(0, BURN_S, fmt, n=BURN_N, _flips=[(0, 1), (9, 0x8000), (15, 4)])
    assert r["iterations"] >= 1 and r["mismatches"] == 2 * r["iterations"], r
    assert r["ok"] is False and r["flipped_words"] == 2, r
    json.dumps(r)


def test_probe_cli_fails_a_flipped_mxfp4_burn_in():
    res = subprocess.run([sys.executable, "-m", "gpumounter_amd", "probe", "--burn-in", "0.05",
                          "--burn-in-format", "mxfp4", "--burn-in-flip", "0:0x1"], cwd=ROOT,
                         capture_output=True, text=True, timeout=180)
    assert res.returncode == 1, (res.stdout[-2000:], res.stderr[-2000:])
    out = json.loads(res.stdout)
    assert out
    for r in out:
        b = r["burn_in_mxfp4"]
        assert "burn_in" not in r and b["format"] == "mxfp4" and b["ok"] is False, r
        assert b["iterations"] >= 1 and b["mismatches"] == b["iterations"], b


@pytest.mark.parametrize("fmt", mxgemm.FORMATS)
def test_kernel_keeps_its_accumulators_in_registers(fmt):
    info = mxgemm.kernel_info(fmt)
    assert info["scratch_bytes"] == 0 and 128 < info["num_regs"] <= 512, info
