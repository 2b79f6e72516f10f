"""Host-link (PCIe) test on the MI355X (``pytest -m gpu``): the gfx950 kernels of
native/hip/gm_hostlink.hip on pinned host memory against the host evaluation of the memtest
pattern function, their error path against planted bit flips, the driver's six legs with its
negative control, and the command lines. Nothing here holds more than 16 MiB of pinned memory.

Geometry the shapes rely on (gm_hostlink.hip): 16-byte elements, 256-thread blocks, a step of
``STEP`` bytes per block, each block's chunk a whole number of steps, blocks whose chunk starts
past the end are not launched. ``BIG`` = 6 steps + 4112 bytes runs, with 3 blocks, as two blocks of three
full steps and one block that has only the 16-byte tail loop (257 elements); with the default
grid as six one-step blocks and the tail-only block; with 1 block as one chunk."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import hostlink, memtest
from gpumounter_amd.ops.probe import ProbeError

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
STEP = hostlink.STEP_BYTES
BIG = 2 * STEP * 3 + 4112
SIZES = (16, 4096 - 16, STEP + 16, BIG)
BLOCKS = (1, 3, None)
GUARD = 64                           # bytes before and after a body
GUARD_WORD = np.uint64(0xFEEDFACECAFEBEEF)
M64 = (1 << 64) - 1
MIB = 1 << 20


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a host without a GPU")


class Pinned:
    """A pinned buffer with guard words around a body of ``nbytes``."""

    def __init__(self, nbytes: int):
        self.whole = torch.empty((nbytes + 2 * GUARD) // 8, dtype=torch.int64, pin_memory=True)
        self.body = self.whole[GUARD // 8:-(GUARD // 8)]
        self.words = self.whole.numpy().view(np.uint64)
        self.data = self.words[GUARD // 8:-(GUARD // 8)]
        self.words[:] = GUARD_WORD
        assert self.body.is_pinned() and self.body.data_ptr() % 16 == 0

    def guards_intact(self) -> bool:
        g = GUARD // 8
        return bool((self.words[:g] == GUARD_WORD).all() and (self.words[-g:] == GUARD_WORD).all())


@pytest.fixture(scope="module")
def bufs():
    """One source and one destination per size, shared by the kernel tests."""
    return {n: (Pinned(n), Pinned(n)) for n in SIZES}


def _want(pattern, invert, pass_, base, nbytes) -> np.ndarray:
    e = memtest.expected(pattern, SEED, pass_, base, nbytes // 8)
    return ~e if invert else e


def _records(res):
    return {(r["offset"], int(r["expected"], 16), int(r["got"], 16)) for r in res["first_errors"]}


# ------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("invert", (False, True))
@pytest.mark.parametrize("pattern", memtest.ALL_PATTERNS)
def test_kwrite_matches_the_host_reference(bufs, pattern, invert):
    for nbytes in SIZES:
        want = _want(pattern, invert, 3, 4096, nbytes)
        for blocks in BLOCKS:
            p = bufs[nbytes][0]
            p.words[:] = GUARD_WORD
            hostlink.kwrite(p.body, pattern, invert=invert, seed=SEED, pass_=3, base_offset=4096,
                            blocks=blocks)
            torch.cuda.synchronize()
            assert np.array_equal(p.data, want), (nbytes, blocks)
            assert p.guards_intact(), (nbytes, blocks)


@pytest.mark.parametrize("pattern", ("addr", "random"))
def test_kread_is_clean_on_a_numpy_filled_buffer(bufs, pattern):
    for nbytes in SIZES:
        p = bufs[nbytes][0]
        p.data[:] = _want(pattern, False, 1, 0, nbytes)
        for blocks in BLOCKS:
            r = hostlink.kread(p.body, pattern, seed=SEED, pass_=1, blocks=blocks)
            assert r["ok"] and r["errors"] == 0 and r["bit_errors"] == 0, (nbytes, blocks, r)
            assert r["first_errors"] == [] and r["bytes"] == nbytes
        # the other polarity is wrong in every bit of every word
        r = hostlink.kread(p.body, pattern, invert=True, seed=SEED, pass_=1, blocks=3)
        assert r["errors"] == nbytes // 8 and r["bit_errors"] == 8 * nbytes, (nbytes, r)
        assert int(r["stuck_mask"], 16) == M64 and len(r["first_errors"]) == min(16, nbytes // 8)


def _flip_words(nbytes: int, count: int):
    """`count` distinct (word index, mask): the first word, the last word, then words spread over
    every block's chunk, full steps and tail alike."""
    n = nbytes // 8
    idx = [0, n - 1][:count]
    k = 1
    while len(idx) < count:
        w = (k * 2654435761) % n
        if w not in idx:
            idx.append(w)
        k += 1
    return [(w, 1 << ((7 * i + 3) % 64) | (0x8000000000000001 if i == 1 else 0))
            for i, w in enumerate(idx)]


@pytest.mark.parametrize("invert", (False, True))
@pytest.mark.parametrize("count", (1, 2, 20))
def test_kread_reports_exactly_the_planted_flips(bufs, count, invert):
    for nbytes in (STEP + 16, BIG):
        p = bufs[nbytes][0]
        want = _want("random", invert, 2, 8192, nbytes)
        flips = _flip_words(nbytes, count)
        p.data[:] = want
        for w, m in flips:
            p.data[w] ^= np.uint64(m)
        planted = {(8192 + 8 * w, int(want[w]), int(want[w]) ^ m) for w, m in flips}
        for blocks in BLOCKS:
            r = hostlink.kread(p.body, "random", invert=invert, seed=SEED, pass_=2,
                               base_offset=8192, blocks=blocks)
            assert not r["ok"] and r["errors"] == count, (nbytes, blocks, r)
            assert r["bit_errors"] == sum(bin(m).count("1") for _, m in flips)
            stuck = 0
            for _, m in flips:
                stuck |= m
            assert int(r["stuck_mask"], 16) == stuck
            got = _records(r)
            assert len(r["first_errors"]) == len(got) == min(count, 16)    # all distinct
            assert got <= planted and (count > 16 or got == planted), (nbytes, blocks)
            assert all(x["pattern"] == "random" and x["pass"] == 2 for x in r["first_errors"])


def _every_load_of_a_step_is_compared(bufs, step_bytes):
    """``bufs``: (source, destination) by size, for one step + 16 B and six steps + 4112 B."""
    loads = step_bytes // 4096                                   # U: 4 KiB per load and block
    for nbytes, step in ((step_bytes + 16, 0), (6 * step_bytes + 4112, 1)):
        src, dst = bufs[nbytes]
        want = _want("random", False, 0, 0, nbytes)
        for c in range(loads):
            off = step * step_bytes + c * 4096 + 16 * ((37 * c + 5) % 256) + 8 * (c & 1)
            src.data[:] = want
            src.data[off // 8] ^= np.uint64(1 << c)
            planted = {(off, int(want[off // 8]), int(want[off // 8]) ^ (1 << c))}
            for blocks in (1, 3):
                r = hostlink.kread(src.body, "random", seed=SEED, blocks=blocks)
                assert r["errors"] == 1 and _records(r) == planted, (nbytes, c, blocks, r)
                r = hostlink.kcopy(src.body, dst.body, "random", seed=SEED, blocks=blocks)
                assert r["errors"] == 1 and _records(r) == planted, (nbytes, c, blocks, r)
                assert np.array_equal(dst.data, src.data)


def test_every_load_of_a_step_is_compared(bufs):
    """One flip at a time in each of the U loads a lane has in flight in a full step (the first
    word, the last word and the tail are covered above), in both words of the 16-byte element,
    for the reading kernel and for the copying one."""
    assert BIG == 6 * STEP + 4112
    _every_load_of_a_step_is_compared(bufs, STEP)


@pytest.fixture
def unroll4():
    """The kernels with 4 loads in flight (bench/hostlink_rates.py sweeps both); yields their
    step in bytes and puts the unroll back."""
    lib = _native.probe()
    was = lib.gm_probe_hostlink_unroll(4)
    try:
        step = hostlink.geometry()["step_bytes"]
        assert step == 4 * 256 * 16
        yield step
    finally:
        lib.gm_probe_hostlink_unroll(was)
        assert hostlink.geometry()["step_bytes"] == STEP


@pytest.mark.parametrize("pattern", memtest.ALL_PATTERNS)
def test_unroll_4_kernels_write_read_and_copy(unroll4, pattern):
    """Every size class again with the 16 KiB step: only a tail, less than a step, one step and
    a tail element, and six steps + 4112 B (with 3 blocks: two of three steps and a tail-only
    one)."""
    for nbytes in (16, 4096 - 16, unroll4 + 16, 6 * unroll4 + 4112):
        src, dst = Pinned(nbytes), Pinned(nbytes)
        want = _want(pattern, False, 3, 4096, nbytes)
        for blocks in BLOCKS:
            src.words[:] = GUARD_WORD
            dst.words[:] = GUARD_WORD
            hostlink.kwrite(src.body, pattern, seed=SEED, pass_=3, base_offset=4096, blocks=blocks)
            torch.cuda.synchronize()
            assert np.array_equal(src.data, want) and src.guards_intact(), (nbytes, blocks)
            r = hostlink.kread(src.body, pattern, seed=SEED, pass_=3, base_offset=4096,
                               blocks=blocks)
            assert r["ok"] and r["errors"] == 0 and r["bytes"] == nbytes, (nbytes, blocks, r)
            r = hostlink.kcopy(src.body, dst.body, pattern, seed=SEED, pass_=3, base_offset=4096,
                               blocks=blocks)
            assert r["ok"] and r["errors"] == 0 and r["bytes"] == nbytes, (nbytes, blocks, r)
            assert np.array_equal(dst.data, want) and np.array_equal(src.data, want)
            assert dst.guards_intact() and src.guards_intact(), (nbytes, blocks)


def test_unroll_4_every_load_of_a_step_is_compared(unroll4):
    sizes = (unroll4 + 16, 6 * unroll4 + 4112)
    _every_load_of_a_step_is_compared({n: (Pinned(n), Pinned(n)) for n in sizes}, unroll4)


@pytest.mark.parametrize("pattern", ("addr", "walk", "random"))
def test_kcopy_copies_checks_and_leaves_the_guards(bufs, pattern):
    for nbytes in SIZES:
        src, dst = bufs[nbytes]
        want = _want(pattern, False, 0, 0, nbytes)
        for blocks in BLOCKS:
            src.words[:] = GUARD_WORD
            dst.words[:] = GUARD_WORD
            src.data[:] = want
            r = hostlink.kcopy(src.body, dst.body, pattern, seed=SEED, blocks=blocks)
            assert r["ok"] and r["errors"] == 0 and r["bytes"] == nbytes, (nbytes, blocks, r)
            assert np.array_equal(dst.data, want) and np.array_equal(src.data, want)
            assert dst.guards_intact() and src.guards_intact(), (nbytes, blocks)


def test_kcopy_reports_a_flipped_source_word_and_delivers_it(bufs):
    for nbytes in (16, BIG):
        src, dst = bufs[nbytes]
        want = _want("random", False, 0, 0, nbytes)
        for w in (0, nbytes // 8 - 1):
            src.data[:] = want
            src.data[w] ^= np.uint64(0x10)
            dst.data[:] = GUARD_WORD
            r = hostlink.kcopy(src.body, dst.body, "random", seed=SEED, blocks=3)
            assert r["errors"] == 1 and r["bit_errors"] == 1 and int(r["stuck_mask"], 16) == 0x10
            assert _records(r) == {(8 * w, int(want[w]), int(want[w]) ^ 0x10)}
            assert np.array_equal(dst.data, src.data)          # what was read is what arrives


def test_kernel_flip_argument_changes_exactly_one_written_word(bufs):
    nbytes = BIG
    src, dst = bufs[nbytes]
    want = _want("addr", False, 0, 4096, nbytes)
    src.data[:] = want
    for w in (0, 2 * STEP // 8 + 5, nbytes // 8 - 1):           # a full step, another, the tail
        flip = (4096 + 8 * w, 0x8000000000000001)                # a global offset, as records are
        after = want.copy()
        after[w] ^= np.uint64(flip[1])
        for blocks in BLOCKS:
            dst.words[:] = GUARD_WORD
            r = hostlink.kcopy(src.body, dst.body, "addr", seed=SEED, base_offset=4096,
                               blocks=blocks, flip=flip)
            assert r["ok"] and r["errors"] == 0, r              # the source check is not affected
            assert np.array_equal(dst.data, after) and dst.guards_intact(), (w, blocks)
            dst.words[:] = GUARD_WORD
            hostlink.kwrite(dst.body, "addr", seed=SEED, base_offset=4096, blocks=blocks,
                            flip=flip)
            torch.cuda.synchronize()
            assert np.array_equal(dst.data, after) and dst.guards_intact(), (w, blocks)
    # a flip offset outside the buffer, or a zero mask, changes nothing
    for flip in ((4096 + nbytes, 1), (0, 1), (4096, 0)):
        hostlink.kwrite(dst.body, "addr", seed=SEED, base_offset=4096, blocks=3, flip=flip)
        torch.cuda.synchronize()
        assert np.array_equal(dst.data, want), flip


def test_kernels_use_64_bit_offsets():
    nbytes, base = 128 << 10, (1 << 35) - (64 << 10)
    p, q = Pinned(nbytes), Pinned(nbytes)
    for pattern in ("addr", "walk", "random"):
        want = _want(pattern, False, 1, base, nbytes)
        hostlink.kwrite(p.body, pattern, seed=SEED, pass_=1, base_offset=base, blocks=3)
        torch.cuda.synchronize()
        assert np.array_equal(p.data, want) and p.guards_intact(), pattern
        assert hostlink.kread(p.body, pattern, seed=SEED, pass_=1, base_offset=base)["ok"]
        w = nbytes // 8 - 3                                      # beyond 2^35
        p.data[w] ^= np.uint64(4)
        r = hostlink.kcopy(p.body, q.body, pattern, seed=SEED, pass_=1, base_offset=base,
                           blocks=3, flip=(base + 8 * (w + 1), 2))
        assert r["errors"] == 1 and r["first_errors"][0]["offset"] == base + 8 * w > 1 << 35
        after = want.copy()
        after[w] ^= np.uint64(4)
        after[w + 1] ^= np.uint64(2)
        assert np.array_equal(q.data, after) and q.guards_intact(), pattern


def test_uint8_and_uint64_tensors_are_accepted():
    for dtype in (torch.uint8, torch.uint64):
        t = torch.empty(4096 // torch.empty(0, dtype=dtype).element_size(), dtype=dtype,
                        pin_memory=True)
        hostlink.kwrite(t, "random", seed=SEED)
        torch.cuda.synchronize()
        assert np.array_equal(t.numpy().view(np.uint64), _want("random", False, 0, 0, 4096))
        assert hostlink.kread(t, "random", seed=SEED)["ok"]


def test_a_device_tensor_is_refused_and_nothing_is_launched():
    """The one refusal tried on the GPU: harmless even if the check were wrong, since the
    pointer is valid device memory of the right size."""
    nbytes = 4096
    dev = torch.full((nbytes // 8,), 0x5A5A, dtype=torch.int64, device="cuda")
    pinned = Pinned(nbytes)
    pinned.data[:] = _want("addr", False, 0, 0, nbytes)
    for call in (lambda: hostlink.kwrite(dev, "addr"), lambda: hostlink.kread(dev, "addr"),
                 lambda: hostlink.kcopy(dev, pinned.body, "addr"),
                 lambda: hostlink.kcopy(pinned.body, dev, "addr")):
        with pytest.raises(ProbeError, match="pinned host memory"):
            call()
    # and below Python, where only hipPointerGetAttributes stands in the way
    lib, res = _native.probe(), _native.MemtestResult()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.gm_probe_hostlink_kwrite(dev.data_ptr(), nbytes, 1, 0, SEED, 0, 0, 4, 0, 0, s) != 0
    assert lib.gm_probe_hostlink_kread(dev.data_ptr(), nbytes, 1, 0, SEED, 0, 0, 4, s, res) != 0
    assert lib.gm_probe_hostlink_kcopy(pinned.body.data_ptr(), dev.data_ptr(), nbytes, 1, 0, 0,
                                       0, 0, 4, 0, 0, s, res) != 0
    assert lib.gm_probe_hostlink_kcopy(dev.data_ptr(), pinned.body.data_ptr(), nbytes, 1, 0, 0,
                                       0, 0, 4, 0, 0, s, res) != 0
    torch.cuda.synchronize()
    assert bool((dev == 0x5A5A).all())                           # nothing wrote to it
    assert np.array_equal(pinned.data, _want("addr", False, 0, 0, nbytes))
    assert pinned.guards_intact()


# ------------------------------------------------------------------------------------- driver
def test_driver_all_legs_all_patterns_clean():
    iters = 2
    r = hostlink.hostlink(0, 4 * MIB, patterns=memtest.ALL_PATTERNS, iters=iters)
    print(json.dumps({n: round(leg["gbps"], 2) for n, leg in r["legs"].items()}),
          json.dumps(r["link"]))
    assert r["ok"] and r["errors"] == 0 and r["bit_errors"] == 0 and r["first_errors"] == [], r
    assert r["bytes"] == 4 * MIB and r["pinned_bytes"] == 8 * MIB
    assert list(r["legs"]) == list(hostlink.ALL_LEGS) and r["patterns"] == list(memtest.ALL_PATTERNS)
    for name, leg in r["legs"].items():
        ways = 2 if name in hostlink.TWO_WAY_LEGS else 1
        assert leg["bytes"] == 4 * MIB * iters * 5 * ways, (name, leg)
        assert leg["errors"] == 0 and leg["ms"] > 0
        assert math.isfinite(leg["gbps"]) and leg["gbps"] > 0, (name, leg)
    for side in ("h2d", "d2h"):
        leg = r["legs"]["bidir"][side]
        assert leg["bytes"] == 4 * MIB * iters * 5 and math.isfinite(leg["gbps"]) and leg["gbps"] > 0
    assert r["seconds"] > 0 and r["host_seconds"] >= 0 and r["link"]["samples"] >= 1


@pytest.mark.parametrize("off", (BIG - 8, STEP + 5 * 4096 + 24))
@pytest.mark.parametrize("leg", hostlink.ALL_LEGS)
def test_driver_books_one_flipped_word_under_its_leg(leg, off):
    """BIG bytes: several full chunks and a tail; the flipped word is the last one (in the tail),
    or the second word of a lane's sixth load in the second full step of the first block."""
    mask = 0x0000100000000010
    r = hostlink.hostlink(0, BIG, patterns=("addr", "random"), passes=2, iters=1, blocks=3,
                          seed=SEED, _flip=(leg, off, mask))
    assert not r["ok"] and r["errors"] == 4 and r["bit_errors"] == 8, r
    assert int(r["stuck_mask"], 16) == mask
    for name, entry in r["legs"].items():
        assert entry["errors"] == (4 if name == leg else 0), (name, r)
    recs = r["first_errors"]
    assert len(recs) == 4 and all(x["leg"] == leg and x["offset"] == off and
                                  int(x["xor"], 16) == mask for x in recs), recs
    assert sorted((x["pattern"], x["pass"]) for x in recs) == \
        [("addr", 0), ("addr", 1), ("random", 0), ("random", 1)]
    for x in recs:
        want = int(memtest.expected(x["pattern"], SEED, x["pass"], off, 1)[0])
        assert int(x["expected"], 16) == want and int(x["got"], 16) == want ^ mask
    if leg == "bidir":                                  # the flip rides the H2D half
        assert r["legs"]["bidir"]["h2d"]["errors"] == 4 and r["legs"]["bidir"]["d2h"]["errors"] == 0


def test_driver_runs_only_the_selected_legs():
    r = hostlink.hostlink(0, STEP + 16, legs=("d2h", "kwrite"), patterns=("walk",), iters=1)
    assert r["ok"] and list(r["legs"]) == ["d2h", "kwrite"], r
    assert all(leg["bytes"] == STEP + 16 for leg in r["legs"].values())
    r = hostlink.hostlink(0, 16, legs=("kduplex",), patterns=("solid",), iters=1, blocks=1)
    assert r["ok"] and list(r["legs"]) == ["kduplex"] and r["legs"]["kduplex"]["bytes"] == 32


# ------------------------------------------------------------------------------ command lines
def _cli(*args, env=None):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=180,
                          env={**os.environ, **(env or {})})


def test_probe_cli_host_link():
    res = _cli("probe", "--host-link", "4M")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["hostlink"]["ok"] and r["hostlink"]["bytes"] == 4 * MIB for r in out), out
    assert all(list(r["hostlink"]["legs"]) == list(hostlink.ALL_LEGS) for r in out)


def test_probe_cli_host_link_flip_fails_and_names_the_leg():
    res = _cli("probe", "--host-link", "4M", "--host-link-flip", "kread:4096:0x10")
    assert res.returncode == 1, (res.stdout[-2000:], res.stderr[-2000:])
    out = json.loads(res.stdout)
    for r in out:
        h = r["hostlink"]
        assert not h["ok"] and h["errors"] == 2 and h["legs"]["kread"]["errors"] == 2, h
        assert all(x["leg"] == "kread" and x["offset"] == 4096 and int(x["xor"], 16) == 0x10
                   for x in h["first_errors"]) and len(h["first_errors"]) == 2


def test_doctor_reports_the_flipped_leg_as_failed():
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    cfg = Config.load(env={}, amdsmi_lib="mock")
    checks = [c for c in doctor.check_gpus(cfg, host_link_bytes=4 * MIB,
                                           host_link_flip=("kduplex", 4096, 0x10))
              if c.name != "gpu"]
    assert checks and all(c.status == "fail" for c in checks), checks
    assert all("kduplex: 2 wrong word(s) first at offset 4096" in c.detail for c in checks), checks
    clean = [c for c in doctor.check_gpus(cfg, host_link_bytes=4 * MIB) if c.name != "gpu"]
    assert clean and all(c.status in ("ok", "warn") and " 0 wrong words" in c.detail
                         for c in clean), clean
