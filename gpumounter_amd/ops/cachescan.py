"""Per-CU cache scan of an attached GPU (native/hip/gm_cachescan.hip): which CU's vector L1,
which XCC's L2, which scalar data cache or instruction cache hands back a wrong word?

The fourth scan in the CU scan's frame (one 256-thread block per CU, the CU id read from the
hardware registers, a table computed on the host and compared bit for bit). Every block owns a
64 KiB segment of an arena in device memory and touches no other byte of it. Four known-answer
tests of 4 signature words per thread:

``l2``      a march over the segment (write, read and invert through an odd-stride permutation,
            read back what another wave wrote) in which every load bypasses the vector L1
``l1``      hit passes over 16 KiB and a replacement sweep over all 64 KiB with plain loads, each
            word also read past the L1: word 0 folds the L1's values, word 1 the bypass's, so word
            0 wrong with word 1 right names the CU's L1 and both wrong the L2 or memory
``scalar``  a pointer chase per wave through a 32 KiB table by scalar loads
``icache``  a straight-line body of distinct steps, each with literals of its own, that spans
            more than twice the instruction cache

The formulas are written out in native/include/gm_probe.h and implemented once for the host and
the kernel (native/include/gm_cachescan_ref.h). :func:`expected` evaluates them without a GPU,
with or without a poked word, and :func:`signature` returns what one block computed.

Two negative controls: ``_inject`` flips a word of a computed signature as in the other scans,
and ``_poke=(test, word offset, mask)`` flips a word of the data itself after the test's fill, so
that the real detection path finds it.

``scan`` also returns ``"timing"``: per test the shader-clock counts of the first and the last
pass as min / median / max over the blocks of the last round. They are the only evidence of where
a load was served; they are reported and never judged.

What it cannot tell: the Infinity Cache cannot be targeted; residency is observed, not
guaranteed; the L1 and instruction-cache sizes are assumptions; a corrupted instruction may fault
rather than miscompute; clocks and thermals are not covered (LDS atomics are in
:mod:`gpumounter_amd.ops.ldsscan`). No silent fallback: a
missing ``libgm_probe.so`` or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe
from gpumounter_amd.ops.cuframe import ANY, DEFAULT_SEED, _ref
from gpumounter_amd.ops.probe import ProbeError, _check

TESTS = {"l2": 1, "l1": 2, "scalar": 4, "icache": 8}
TEST_NAMES = {v: k for k, v in TESTS.items()}
ALL_TESTS = tuple(TESTS)
DEFAULT_ITERS = 4             # native/include/gm_cachescan_ref.h GM_CACHESCAN_DEFAULT_ITERS
MAX_ITERS = 63                # GM_CACHESCAN_MAX_ITERS
SEG_WORDS = 16384             # GM_CACHESCAN_SEG_WORDS
TABLE_WORDS = 8192            # GM_CACHESCAN_TABLE_WORDS
ICACHE_MIN_BODY_BYTES = 131072    # twice the 64 KiB taken for the instruction cache

__all__ = ["TESTS", "ALL_TESTS", "DEFAULT_ITERS", "MAX_ITERS", "ANY", "ProbeError", "parse_tests",
           "parse_inject", "parse_poke", "expected", "signature", "scan", "kernel_info",
           "geometry", "describe_failed"]


SCAN = cuframe.Scan(
    label="cache-scan", key="cachescan", bits=TESTS, selection="tests",
    default_iters=DEFAULT_ITERS, max_iters=MAX_ITERS, title="per-CU cache scan",
    covers=" (vector L1, L2, scalar and instruction caches)",
    does="a march served by the L2, hit and replacement passes through the vector L1, a pointer "
         "chase through the scalar data cache and a body larger than the instruction cache",
    flips="signature word of that test", iters_unit="units of work per test",
    more_controls={"poke": (
        "TEST:WORD_OFFSET:MASK",
        "negative control: flip that word of the test's data (l2, l1: of every block's segment "
        "after the fill; scalar: of the table); the test must find it", "data poke")})
bit_of, mask_of, parse_tests, parse_inject = (SCAN.bit_of, SCAN.mask_of, SCAN.parse_list,
                                              SCAN.parse_inject)
describe_failed = SCAN.describe_failed
_int = SCAN.check_int


def _poke_arg(poke, mask: int):
    """(test, word offset, xor mask) → the C struct; None stays None. ``mask``: the tests that
    run."""
    if poke is None:
        return None
    try:
        test, offset, xor = poke
    except (TypeError, ValueError):
        raise ProbeError(f"cache-scan: poke {poke!r} is not (test, word offset, mask)") from None
    bit = bit_of(test)
    if bit == TESTS["icache"]:
        raise ProbeError("cache-scan: icache has no data to poke")
    if not bit & mask:
        raise ProbeError(f"cache-scan: poke of {TEST_NAMES[bit]!r}, which is not run")
    words = TABLE_WORDS if bit == TESTS["scalar"] else SEG_WORDS
    _int(offset, 0, words - 1, f"poke word offset of {TEST_NAMES[bit]}")
    _int(xor, 1, 0xFFFFFFFF, "poke mask")
    return _native.CachescanPoke(bit, offset, xor)


def parse_poke(text):
    """``"TEST:WORD_OFFSET:MASK"`` (integers as Python literals, e.g. ``l1:4099:0x10``) →
    (test name, word offset, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    if len(parts) != 3:
        raise ProbeError(f"cache-scan: cannot read {text!r} as TEST:WORD_OFFSET:MASK")
    try:
        offset, xor = (int(p, 0) for p in parts[1:])
    except ValueError:
        raise ProbeError(f"cache-scan: {text!r} holds something that is not an integer") from None
    poke = (TEST_NAMES[bit_of(parts[0])], offset, xor)
    _poke_arg(poke, TESTS[poke[0]])
    return poke


def expected(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, poke=None):
    """numpy uint32[256, 4]: word i of thread t of ``test``'s signature, in a run with ``poke``
    (a poke of another test leaves it alone). Host only, no GPU."""
    return SCAN.expected(test, seed, iters,
                         lambda bit: (_ref(_poke_arg(poke, mask_of(ALL_TESTS))),))


def signature(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None, poke=None):
    """One block of the scan's device code on the current device, on an arena of its own:
    (uint32[256, 4] raw signature, where), ``where`` as
    :func:`gpumounter_amd.ops.cuscan.signature` gives it. ``poke`` must name ``test``."""
    return SCAN.signature(test, seed, iters, stream, lambda bit: (_ref(_poke_arg(poke, bit)),))


def decode_timing(mask: int, timing) -> Dict:
    """The C timing struct → {"blocks": n, test: {"first": {min, median, max}, "last": ...}}."""
    out: Dict = {"blocks": int(timing.blocks)}
    for ix, name in enumerate(TESTS):
        if mask & TESTS[name]:
            out[name] = {which: dict(zip(("min", "median", "max"),
                                         (int(v) for v in getattr(timing, which)[ix])))
                         for which in ("first", "last")}
    return out


def scan(dev: int, tests=ALL_TESTS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None, _poke=None) -> Dict:
    """The scan of device ``dev``; rounds, ``ok``, ``complete`` and the result shape as in
    :func:`gpumounter_amd.ops.cuscan.scan` (``tests``, ``tests_failed`` per CU by name, ``test``
    in a record), plus ``timing`` (:func:`decode_timing`; shader-clock counts, reported and never
    judged). ``_inject=(id or "any", test, thread, word, mask)`` and ``_poke=(test, word offset,
    mask)`` are the negative controls."""
    timing = _native.CachescanTiming()
    out = SCAN.scan(dev, tests, iters, seed, min_rounds, max_rounds, _inject,
                    lambda mask: (_ref(_poke_arg(_poke, mask)),), (C.byref(timing),))
    out["timing"] = decode_timing(mask_of(tests), timing)
    return out


def kernel_info() -> Dict[str, int]:
    """``num_regs`` and ``scratch_bytes`` of the scan kernel as the HIP runtime reports them on
    the current device, and ``icache_body_bytes``, the span of the ``icache`` test's body between
    the program-counter readings at its two ends (one block runs it once). The body is larger than
    the instruction cache only while that is at least :data:`ICACHE_MIN_BODY_BYTES`."""
    regs, scratch, body = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(_native.probe().gm_probe_cachescan_kernel_info(
        C.byref(regs), C.byref(scratch), C.byref(body)), "cache-scan kernel info")
    return {"num_regs": regs.value, "scratch_bytes": scratch.value,
            "icache_body_bytes": body.value}


def geometry() -> Dict[str, int]:
    """The build's constants: ``seg_bytes``, ``l1_hit_bytes``, ``table_bytes``, ``icache_steps``.
    Host only, no GPU."""
    v = [C.c_uint32(0) for _ in range(4)]
    _check(_native.probe().gm_probe_cachescan_geometry(*(C.byref(x) for x in v)),
           "cache-scan geometry")
    return dict(zip(("seg_bytes", "l1_hit_bytes", "table_bytes", "icache_steps"),
                    (x.value for x in v)))
