"""Per-CU matrix-core format scan of an attached GPU (native/hip/gm_mfmascan.hip): which CU's
matrix cores compute a wrong word, and in which number format?

The CU scan checks the matrix cores through one bf16 instruction. This scan uses its frame (one
256-thread block per CU, the CU id read from the hardware registers, a table computed on the host
and compared bit for bit) around the formats gfx950 was built for: f16, fp8 (e4m3), bf8 (e5m2),
i8, f32, f64 and the five block-scaled ``v_mfma_scale_f32_16x16x128_f8f6f4`` forms (fp8, bf8, fp6
e2m3, bf6 e3m2, fp4 e2m1) with E8M0 scales. Every wave runs ``iters`` dependent MFMAs per format on
operands chosen so that every product and partial sum is exact in the accumulator type: the
result is one definite bit pattern in any summation order (formulas: native/include/gm_probe.h).
:func:`expected` evaluates it without a GPU and :func:`signature` returns what one block computed.

What it cannot tell: mixed A/B formats, the 32x32 shapes, the sparse ``v_smfmac_*`` forms, a
different scale per K-block of a row, NaN / infinity / subnormal operands and rounding (nothing
here rounds) are not covered; and as for the CU scan, a CU id is a label and ``complete`` says
whether every CU was reached. No silent fallback: a missing ``libgm_probe.so`` or a HIP failure
raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe
from gpumounter_amd.ops.cuframe import ANY, DEFAULT_SEED
from gpumounter_amd.ops.probe import ProbeError, _check

FORMATS = {"f16": 1, "fp8": 2, "bf8": 4, "i8": 8, "f32": 16, "f64": 32, "mxfp8": 64,
           "mxbf8": 128, "mxfp6": 256, "mxbf6": 512, "mxfp4": 1024}
FORMAT_NAMES = {v: k for k, v in FORMATS.items()}
ALL_FORMATS = tuple(FORMATS)
K_PER_STEP = {"f16": 32, "fp8": 32, "bf8": 32, "i8": 64, "f32": 4, "f64": 4, "mxfp8": 128,
              "mxbf8": 128, "mxfp6": 128, "mxbf6": 128, "mxfp4": 128}
DEFAULT_ITERS = 16            # native/include/gm_mfmascan_ref.h GM_MFMASCAN_DEFAULT_ITERS
MAX_ITERS = 63                # GM_MFMASCAN_MAX_ITERS: f32's 4 * 255^2 * iters < 2^24

__all__ = ["FORMATS", "ALL_FORMATS", "DEFAULT_ITERS", "MAX_ITERS", "ANY", "ProbeError",
           "parse_formats", "parse_inject", "expected", "images", "signature", "scan",
           "describe_failed"]


SCAN = cuframe.Scan(
    label="mfma-scan", key="mfmascan", bits=FORMATS, selection="formats",
    default_iters=DEFAULT_ITERS, max_iters=MAX_ITERS, title="per-CU matrix-core format scan",
    does="bit-exact MFMAs in f16, fp8, bf8, i8, f32, f64 and the block-scaled fp8, bf8, fp6, bf6 "
         "and fp4 forms", flips="accumulator word of that format",
    iters_unit="dependent MFMAs per wave and format")
bit_of, mask_of, parse_formats, parse_inject = (SCAN.bit_of, SCAN.mask_of, SCAN.parse_list,
                                                SCAN.parse_inject)
describe_failed = SCAN.describe_failed


def expected(fmt, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS):
    """numpy uint32[256, 4]: word i of thread t of ``fmt``'s signature. Host only, no GPU."""
    return SCAN.expected(fmt, seed, iters)


def images(fmt, seed: int = DEFAULT_SEED, step: int = 0):
    """The operand register images of one step, as the kernel feeds them to the instruction:
    (uint32[4 waves, 2 operands, 64 lanes, 8 dwords], uint32[4, 2, 16] E8M0 scale bytes; 127 for
    a format without scales). Host only, no GPU."""
    import numpy as np

    bit = bit_of(fmt)
    SCAN.check_int(seed, 0, (1 << 64) - 1, "seed"), SCAN.check_int(step, 0, MAX_ITERS - 1, "step")
    img = np.empty(4 * 2 * 64 * 8, dtype=np.uint32)
    sc = np.empty(4 * 2 * 16, dtype=np.uint32)
    _check(_native.probe().gm_probe_mfmascan_images(
        bit, seed, step, img.ctypes.data_as(C.POINTER(C.c_uint32)),
        sc.ctypes.data_as(C.POINTER(C.c_uint32))), "mfma-scan images")
    return img.reshape(4, 2, 64, 8), sc.reshape(4, 2, 16)


def signature(fmt, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None):
    """One block of the scan's device code on the current device: (uint32[256, 4] raw signature,
    where), ``where`` as :func:`gpumounter_amd.ops.cuscan.signature` gives it."""
    return SCAN.signature(fmt, seed, iters, stream)


def scan(dev: int, formats=ALL_FORMATS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None) -> Dict:
    """The scan of device ``dev``; rounds, ``ok`` and ``complete`` as in
    :func:`gpumounter_amd.ops.cuscan.scan`, whose result shape this has with ``formats``,
    ``formats_failed`` and a record's ``format`` in place of ``tests``, ``tests_failed`` and
    ``test``. ``_inject=(id or "any", format, thread, word, mask)`` is the negative control."""
    return SCAN.scan(dev, formats, iters, seed, min_rounds, max_rounds, _inject)
