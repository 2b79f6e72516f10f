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
rather than miscompute; LDS atomics, clocks and thermals are not covered. No silent fallback: a
missing ``libgm_probe.so`` or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops import cuscan
from gpumounter_amd.ops.cuscan import ANY, DEFAULT_SEED, MAX_ROUNDS, THREADS, WORDS
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


def bit_of(test) -> int:
    """The bit of one test, given by name or by bit."""
    if isinstance(test, str) and test in TESTS:
        return TESTS[test]
    if isinstance(test, int) and not isinstance(test, bool) and test in TEST_NAMES:
        return test
    raise ProbeError(f"unknown cache-scan test {test!r} (one of {', '.join(TESTS)})")


def mask_of(tests: Iterable) -> int:
    if isinstance(tests, (str, int)):
        tests = (tests,)
    mask = 0
    for t in tests:
        mask |= bit_of(t)
    if not mask:
        raise ProbeError("cache-scan needs at least one test")
    return mask


def parse_tests(text) -> Tuple[str, ...]:
    """``"l2,icache"`` → ("l2", "icache"); every name is checked."""
    names = tuple(t.strip() for t in str(text).split(",") if t.strip())
    mask_of(names)
    return names


def _int(v, lo: int, hi: int, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ProbeError(f"cache-scan: {what} must be an integer in [{lo}, {hi}], got {v!r}")
    return v


def _inject_arg(inject, mask: int):
    """(id or "any", test, thread, word, xor mask) → the C struct; None stays None."""
    if inject is None:
        return None
    try:
        cu_id, test, thread, word, xor = inject
    except (TypeError, ValueError):
        raise ProbeError(f"cache-scan: injection {inject!r} is not (id, test, thread, word, "
                         f"mask)") from None
    bit = bit_of(test)
    if not bit & mask:
        raise ProbeError(f"cache-scan: injection into {TEST_NAMES[bit]!r}, which is not run")
    if cu_id != ANY:
        cuscan.decode_id(cu_id)
    _int(thread, 0, THREADS - 1, "injection thread")
    _int(word, 0, WORDS - 1, "injection word")
    _int(xor, 1, 0xFFFFFFFF, "injection mask")
    return _native.CuscanInject(_native.CUSCAN_ANY if cu_id == ANY else cu_id, bit, thread, word,
                                xor)


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


def parse_inject(text):
    """``"ID|any:TEST:THREAD:WORD:MASK"`` (integers as Python literals, e.g.
    ``0x123:l1:130:2:0x10000``) → (id or "any", test name, thread, word, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    if len(parts) != 5:
        raise ProbeError(f"cache-scan: cannot read {text!r} as ID|any:TEST:THREAD:WORD:MASK")
    try:
        cu_id = ANY if parts[0].lower() == ANY else int(parts[0], 0)
        thread, word, xor = (int(p, 0) for p in parts[2:])
    except ValueError:
        raise ProbeError(f"cache-scan: {text!r} holds something that is not an integer") from None
    inj = (cu_id, TEST_NAMES[bit_of(parts[1])], thread, word, xor)
    _inject_arg(inj, TESTS[inj[1]])
    return inj


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


def _ref(arg):
    return C.byref(arg) if arg is not None else None


def expected(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, poke=None):
    """numpy uint32[256, 4]: word i of thread t of ``test``'s signature, in a run with ``poke``
    (a poke of another test leaves it alone). Host only, no GPU."""
    import numpy as np

    bit = bit_of(test)
    _int(seed, 0, (1 << 64) - 1, "seed"), _int(iters, 1, MAX_ITERS, "iters")
    pk = _poke_arg(poke, TESTS["l2"] | TESTS["l1"] | TESTS["scalar"] | TESTS["icache"])
    out = np.empty(THREADS * WORDS, dtype=np.uint32)
    _check(_native.probe().gm_probe_cachescan_expected(
        bit, seed, iters, _ref(pk), out.ctypes.data_as(C.POINTER(C.c_uint32))),
        "cache-scan expected")
    return out.reshape(THREADS, WORDS)


def signature(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None, poke=None):
    """One block of the scan's device code on the current device, on an arena of its own:
    (uint32[256, 4] raw signature, where), ``where`` as
    :func:`gpumounter_amd.ops.cuscan.signature` gives it. ``poke`` must name ``test``."""
    bit = bit_of(test)
    _int(seed, 0, (1 << 64) - 1, "seed"), _int(iters, 1, MAX_ITERS, "iters")
    pk = _poke_arg(poke, bit)
    import numpy as np
    import torch

    out = torch.zeros(THREADS * WORDS, dtype=torch.int32, device="cuda")
    where = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream(out.device)
    if stream is not None:
        s.wait_stream(torch.cuda.current_stream(out.device))   # out and where are filled there
    with torch.cuda.device(out.device):
        _check(_native.probe().gm_probe_cachescan_signature(
            bit, seed, iters, _ref(pk), out.data_ptr(), where.data_ptr(),
            C.c_void_p(s.cuda_stream)), "cache-scan signature")
    s.synchronize()
    w = [int(v) & 0xFFFFFFFF for v in where.cpu().tolist()]
    sig = out.cpu().numpy().view(np.uint32).reshape(THREADS, WORDS)
    return sig, {"id": w[0], **cuscan.decode_id(w[0] & (_native.CUSCAN_IDS - 1)), "simds": w[1:]}


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
    mask = mask_of(tests)
    _int(iters, 1, MAX_ITERS, "iters")
    _int(dev, 0, (1 << 31) - 1, "device")
    _int(seed, 0, (1 << 64) - 1, "seed")
    _int(min_rounds, 1, MAX_ROUNDS, "min_rounds")
    _int(max_rounds, min_rounds, MAX_ROUNDS, "max_rounds (at least min_rounds)")
    inj = _inject_arg(_inject, mask)
    pk = _poke_arg(_poke, mask)
    res = _native.CuscanResult()
    cus = (_native.CuscanCu * _native.CUSCAN_IDS)()
    n = C.c_int(0)
    timing = _native.CachescanTiming()
    _check(_native.probe().gm_probe_cachescan(
        dev, mask, iters, seed, min_rounds, max_rounds, _ref(inj), _ref(pk), C.byref(res), cus,
        _native.CUSCAN_IDS, C.byref(n), C.byref(timing)), "cache-scan")
    out = cuscan.decode_result(dev, mask, iters, res, cus, n.value, TESTS, "tests")
    out["timing"] = decode_timing(mask, timing)
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


def describe_failed(result: Dict) -> str:
    """One line naming the failed units of a :func:`scan` result as the CU scan names them, with
    the tests that failed there, for ``doctor``."""
    return cuscan.describe_failed(result, "tests")
