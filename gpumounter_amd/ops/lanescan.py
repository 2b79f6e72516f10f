"""Per-CU register, lane and scalar-unit scan of an attached GPU (native/hip/gm_lanescan.hip):
which CU's cross-lane network, register file, scalar unit, transcendental pipe, fp64 pipe or
packed arithmetic computes a wrong word?

The third scan in the CU scan's frame (one 256-thread block per CU, the CU id read from the
hardware registers, a table computed on the host and compared bit for bit). Six known-answer
tests of 4 signature words per thread:

``xlane``    DPP (quad_perm, row and wave shifts and rotates, mirrors, broadcasts, with row and
             bank masks and bound_ctrl), ds_bpermute, ds_permute, ds_swizzle in both modes,
             v_readlane / v_readfirstlane / v_writelane, v_permlane16_swap / v_permlane32_swap,
             ballot + mbcnt
``regfile``  a march over 192 run-time indexed VGPRs and 192 accumulation registers per lane
``salu``     a dependent chain on the scalar ALU with reads through the scalar data cache
``trans``    v_exp / log / rcp / rsq / sqrt / sin / cos in f32, rcp / sqrt / rsq in f64 and f16,
             at points where the exact result is representable
``f64``      v_fma / mul / add / ldexp / floor / cvt in fp64 on bounded integers
``packed``   v_pk_fma_f32, the packed f16 and 16-bit integer operations, v_dot4 and v_dot2

The data formulas are shared between the host and the kernel (native/include/gm_lanescan_ref.h,
written out in gm_probe.h); the operation under test is not: on the host it is a plain model of
what the ISA document says the instruction does. :func:`expected` evaluates it without a GPU and
:func:`signature` returns what one block computed.

What it cannot tell: the scaled conversion instructions, rounding, NaN, infinity and subnormal
behaviour, transcendental results at points that are not exact, the sign of a zero result, LDS
atomics, clocks and thermals are not covered (the vector L1, L2, scalar and instruction caches
are in :mod:`gpumounter_amd.ops.cachescan`); and as for the CU scan, a CU id is a label and ``complete`` says whether every CU was reached. No
silent fallback: a missing ``libgm_probe.so`` or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops import cuscan
from gpumounter_amd.ops.cuscan import ANY, DEFAULT_SEED, MAX_ROUNDS, THREADS, WORDS
from gpumounter_amd.ops.probe import ProbeError, _check

TESTS = {"xlane": 1, "regfile": 2, "salu": 4, "trans": 8, "f64": 16, "packed": 32}
TEST_NAMES = {v: k for k, v in TESTS.items()}
ALL_TESTS = tuple(TESTS)
DEFAULT_ITERS = 16            # native/include/gm_lanescan_ref.h GM_LANESCAN_DEFAULT_ITERS
MAX_ITERS = 63                # GM_LANESCAN_MAX_ITERS: packed's 16 * 2^14 * iters < 2^24
MENU_FIELDS = ("kind", "imm", "row_mask", "bank_mask", "bound_ctrl")

__all__ = ["TESTS", "ALL_TESTS", "DEFAULT_ITERS", "MAX_ITERS", "ANY", "ProbeError", "parse_tests",
           "parse_inject", "expected", "lanes", "signature", "scan", "kernel_info",
           "describe_failed"]


def bit_of(test) -> int:
    """The bit of one test, given by name or by bit."""
    if isinstance(test, str) and test in TESTS:
        return TESTS[test]
    if isinstance(test, int) and not isinstance(test, bool) and test in TEST_NAMES:
        return test
    raise ProbeError(f"unknown lane-scan test {test!r} (one of {', '.join(TESTS)})")


def mask_of(tests: Iterable) -> int:
    if isinstance(tests, (str, int)):
        tests = (tests,)
    mask = 0
    for t in tests:
        mask |= bit_of(t)
    if not mask:
        raise ProbeError("lane-scan needs at least one test")
    return mask


def parse_tests(text) -> Tuple[str, ...]:
    """``"xlane,salu"`` → ("xlane", "salu"); every name is checked."""
    names = tuple(t.strip() for t in str(text).split(",") if t.strip())
    mask_of(names)
    return names


def _int(v, lo: int, hi: int, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ProbeError(f"lane-scan: {what} must be an integer in [{lo}, {hi}], got {v!r}")
    return v


def _inject_arg(inject, mask: int):
    """(id or "any", test, thread, word, xor mask) → the C struct; None stays None."""
    if inject is None:
        return None
    try:
        cu_id, test, thread, word, xor = inject
    except (TypeError, ValueError):
        raise ProbeError(f"lane-scan: injection {inject!r} is not (id, test, thread, word, "
                         f"mask)") from None
    bit = bit_of(test)
    if not bit & mask:
        raise ProbeError(f"lane-scan: injection into {TEST_NAMES[bit]!r}, which is not run")
    if cu_id != ANY:
        cuscan.decode_id(cu_id)
    _int(thread, 0, THREADS - 1, "injection thread")
    _int(word, 0, WORDS - 1, "injection word")
    _int(xor, 1, 0xFFFFFFFF, "injection mask")
    return _native.CuscanInject(_native.CUSCAN_ANY if cu_id == ANY else cu_id, bit, thread, word,
                                xor)


def parse_inject(text):
    """``"ID|any:TEST:THREAD:WORD:MASK"`` (integers as Python literals, e.g.
    ``0x123:xlane:130:2:0x10000``) → (id or "any", test name, thread, word, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    if len(parts) != 5:
        raise ProbeError(f"lane-scan: cannot read {text!r} as ID|any:TEST:THREAD:WORD:MASK")
    try:
        cu_id = ANY if parts[0].lower() == ANY else int(parts[0], 0)
        thread, word, xor = (int(p, 0) for p in parts[2:])
    except ValueError:
        raise ProbeError(f"lane-scan: {text!r} holds something that is not an integer") from None
    inj = (cu_id, TEST_NAMES[bit_of(parts[1])], thread, word, xor)
    _inject_arg(inj, TESTS[inj[1]])
    return inj


def expected(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS):
    """numpy uint32[256, 4]: word i of thread t of ``test``'s signature. Host only, no GPU."""
    import numpy as np

    bit = bit_of(test)
    _int(seed, 0, (1 << 64) - 1, "seed"), _int(iters, 1, MAX_ITERS, "iters")
    out = np.empty(THREADS * WORDS, dtype=np.uint32)
    _check(_native.probe().gm_probe_lanescan_expected(
        bit, seed, iters, out.ctypes.data_as(C.POINTER(C.c_uint32))), "lane-scan expected")
    return out.reshape(THREADS, WORDS)


def lanes() -> Tuple[List[Dict[str, int]], int]:
    """(the ``xlane`` test's menu, the ``trans`` test's operation mask). Entry m of the menu is the
    movement of the steps with (s + H(0x301, 0)) % len(menu) == m: ``kind`` 0 is a DPP move with
    ``imm`` as its dpp_ctrl and the two masks and bound_ctrl, ``kind`` 1 a ds_swizzle with ``imm``
    as its offset, and any other ``kind`` names the movement itself (gm_probe.h lists them). Host
    only, no GPU."""
    cap = 64
    menu = (C.c_uint32 * (5 * cap))()
    n, ops = C.c_int(0), C.c_uint32(0)
    _check(_native.probe().gm_probe_lanescan_lanes(menu, cap, C.byref(n), C.byref(ops)),
           "lane-scan lanes")
    return ([dict(zip(MENU_FIELDS, menu[5 * i:5 * i + 5])) for i in range(n.value)], ops.value)


def signature(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None):
    """One block of the scan's device code on the current device: (uint32[256, 4] raw signature,
    where), ``where`` as :func:`gpumounter_amd.ops.cuscan.signature` gives it."""
    bit = bit_of(test)
    _int(seed, 0, (1 << 64) - 1, "seed"), _int(iters, 1, MAX_ITERS, "iters")
    import numpy as np
    import torch

    out = torch.zeros(THREADS * WORDS, dtype=torch.int32, device="cuda")
    where = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream(out.device)
    if stream is not None:
        s.wait_stream(torch.cuda.current_stream(out.device))   # out and where are filled there
    with torch.cuda.device(out.device):
        _check(_native.probe().gm_probe_lanescan_signature(
            bit, seed, iters, out.data_ptr(), where.data_ptr(), C.c_void_p(s.cuda_stream)),
            "lane-scan signature")
    s.synchronize()
    w = [int(v) & 0xFFFFFFFF for v in where.cpu().tolist()]
    sig = out.cpu().numpy().view(np.uint32).reshape(THREADS, WORDS)
    return sig, {"id": w[0], **cuscan.decode_id(w[0] & (_native.CUSCAN_IDS - 1)), "simds": w[1:]}


def scan(dev: int, tests=ALL_TESTS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None) -> Dict:
    """The scan of device ``dev``; rounds, ``ok``, ``complete`` and the result shape as in
    :func:`gpumounter_amd.ops.cuscan.scan` (``tests``, ``tests_failed`` per CU by name, ``test``
    in a record). ``_inject=(id or "any", test, thread, word, mask)`` is the negative control."""
    mask = mask_of(tests)
    _int(iters, 1, MAX_ITERS, "iters")
    _int(dev, 0, (1 << 31) - 1, "device")
    _int(seed, 0, (1 << 64) - 1, "seed")
    _int(min_rounds, 1, MAX_ROUNDS, "min_rounds")
    _int(max_rounds, min_rounds, MAX_ROUNDS, "max_rounds (at least min_rounds)")
    inj = _inject_arg(_inject, mask)
    res = _native.CuscanResult()
    cus = (_native.CuscanCu * _native.CUSCAN_IDS)()
    n = C.c_int(0)
    _check(_native.probe().gm_probe_lanescan(
        dev, mask, iters, seed, min_rounds, max_rounds,
        C.byref(inj) if inj is not None else None, C.byref(res), cus,
        _native.CUSCAN_IDS, C.byref(n)), "lane-scan")
    return cuscan.decode_result(dev, mask, iters, res, cus, n.value, TESTS, "tests")


def kernel_info() -> Dict[str, int]:
    """``num_regs`` and ``scratch_bytes`` of the scan kernel as the HIP runtime reports them on
    the current device. The register march is only a register march while ``scratch_bytes`` is 0."""
    regs, scratch = C.c_int(0), C.c_int(0)
    _check(_native.probe().gm_probe_lanescan_kernel_info(C.byref(regs), C.byref(scratch)),
           "lane-scan kernel info")
    return {"num_regs": regs.value, "scratch_bytes": scratch.value}


def describe_failed(result: Dict) -> str:
    """One line naming the failed units of a :func:`scan` result as the CU scan names them, with
    the tests that failed there, for ``doctor``."""
    return cuscan.describe_failed(result, "tests")
