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
from typing import Dict, List, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe
from gpumounter_amd.ops.cuframe import ANY, DEFAULT_SEED
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


SCAN = cuframe.Scan(
    label="lane-scan", key="lanescan", bits=TESTS, selection="tests", default_iters=DEFAULT_ITERS,
    max_iters=MAX_ITERS, title="per-CU register, lane and scalar-unit scan",
    does="bit-exact cross-lane moves, a register-file march, a scalar chain, transcendentals at "
         "exact points, fp64 and packed arithmetic", flips="signature word of that test",
    iters_unit="units of work per test")
bit_of, mask_of, parse_tests, parse_inject = (SCAN.bit_of, SCAN.mask_of, SCAN.parse_list,
                                              SCAN.parse_inject)
describe_failed = SCAN.describe_failed


def expected(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS):
    """numpy uint32[256, 4]: word i of thread t of ``test``'s signature. Host only, no GPU."""
    return SCAN.expected(test, seed, iters)


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
    return SCAN.signature(test, seed, iters, stream)


def scan(dev: int, tests=ALL_TESTS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None) -> Dict:
    """The scan of device ``dev``; rounds, ``ok``, ``complete`` and the result shape as in
    :func:`gpumounter_amd.ops.cuscan.scan` (``tests``, ``tests_failed`` per CU by name, ``test``
    in a record). ``_inject=(id or "any", test, thread, word, mask)`` is the negative control."""
    return SCAN.scan(dev, tests, iters, seed, min_rounds, max_rounds, _inject)


def kernel_info() -> Dict[str, int]:
    """``num_regs`` and ``scratch_bytes`` of the scan kernel as the HIP runtime reports them on
    the current device. The register march is only a register march while ``scratch_bytes`` is 0."""
    regs, scratch = C.c_int(0), C.c_int(0)
    _check(_native.probe().gm_probe_lanescan_kernel_info(C.byref(regs), C.byref(scratch)),
           "lane-scan kernel info")
    return {"num_regs": regs.value, "scratch_bytes": scratch.value}
