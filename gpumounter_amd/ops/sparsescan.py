"""Per-CU sparse (2:4) and 32x32 matrix-core scan of an attached GPU
(native/hip/gm_sparsescan.hip): which CU's sparse matrix path computes a wrong word, and in which
form?

The sixth scan in the CU scan's frame (one 256-thread block per CU that declares all 160 KiB of
LDS, the CU id read from the hardware registers, a table computed on the host and compared bit for
bit). The matrix-core format scan leaves out ``v_smfmac_*``: a datapath of its own, with an index
register, a 4:2 operand selector in front of the multipliers and an ``abid`` set selector. This
scan runs ``iters`` dependent SMFMACs per wave and form in all eleven forms gfx950 has: f16, bf16,
i8, fp8 (e4m3), bf8 (e5m2) and the two mixed fp8/bf8 forms at 16x16, and f16, bf16, i8 and fp8 at
32x32, the C/D layout with 16 accumulator registers per lane. A holds the kept half of a 2:4
pattern, the index register says where each kept element sat (every ordered pair of positions
occurs, in both halves of the register for the 16-bit forms), and the operands are the format
scan's sixteen exact values: every product and partial sum is exact, so the result is one definite
bit pattern in any summation order (model and premises: native/include/gm_probe.h).

:func:`expected` evaluates the model without a GPU, from the register images :func:`images`
returns; :func:`signature` returns what one block computed; :func:`apply` runs one instruction per
wave on images the caller built and returns the raw accumulator registers, which is how the model's
premises are checked against something other than the model, and how a wrong one is read off.

What it cannot tell: index pairs that are not ascending are never issued; ``cbsz`` other than 0,
``abid`` with an 8-bit form, the dense 32x32 ``v_mfma_*`` instructions, NaN / infinity / subnormal
operands and rounding (nothing here rounds) are not covered; a CU id is a label and ``complete``
says whether every CU was reached. No silent fallback: a missing ``libgm_probe.so`` or a HIP
failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe
from gpumounter_amd.ops.cuframe import ANY, DEFAULT_SEED
from gpumounter_amd.ops.probe import ProbeError, _check

FORMATS = {"f16": 1, "bf16": 2, "i8": 4, "fp8": 8, "bf8": 16, "fp8bf8": 32, "bf8fp8": 64,
           "f16-32x32": 128, "bf16-32x32": 256, "i8-32x32": 512, "fp8-32x32": 1024}
FORMAT_NAMES = {v: k for k, v in FORMATS.items()}
ALL_FORMATS = tuple(FORMATS)
K_PER_STEP = {"f16": 64, "bf16": 64, "i8": 128, "fp8": 128, "bf8": 128, "fp8bf8": 128,
              "bf8fp8": 128, "f16-32x32": 32, "bf16-32x32": 32, "i8-32x32": 64,
              "fp8-32x32": 64}          # dense K; half of it is kept in A
WIDE_FORMATS = ("f16", "bf16", "f16-32x32", "bf16-32x32")    # 16-bit: two index sets, abid 0 / 1
DEFAULT_ITERS = 16            # native/include/gm_sparsescan_ref.h GM_SPARSESCAN_DEFAULT_ITERS
MAX_ITERS = 63                # GM_SPARSESCAN_MAX_ITERS
A_DWORDS, B_DWORDS, ACC_WORDS = 4, 8, 16

__all__ = ["FORMATS", "ALL_FORMATS", "K_PER_STEP", "DEFAULT_ITERS", "MAX_ITERS", "ANY",
           "ProbeError", "parse_formats", "parse_inject", "expected", "images", "signature",
           "apply", "scan", "describe_failed"]


SCAN = cuframe.Scan(
    label="sparse-scan", key="sparsescan", bits=FORMATS, selection="formats",
    default_iters=DEFAULT_ITERS, max_iters=MAX_ITERS,
    title="per-CU sparse and 32x32 matrix-core scan",
    covers=" (the 2:4 v_smfmac forms, 16x16 and 32x32)",
    does="bit-exact 2:4 sparse SMFMACs in f16, bf16, i8, fp8, bf8 and mixed fp8/bf8 at 16x16 and "
         "in f16, bf16, i8 and fp8 at 32x32", flips="signature word of that format",
    iters_unit="dependent SMFMACs per wave and format")
bit_of, mask_of, parse_formats, parse_inject = (SCAN.bit_of, SCAN.mask_of, SCAN.parse_list,
                                                SCAN.parse_inject)
describe_failed = SCAN.describe_failed


def expected(fmt, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS):
    """numpy uint32[256, 4]: word i of thread t of ``fmt``'s signature (a 32x32 form's word i
    folds accumulator registers 4 i .. 4 i + 3). Host only, no GPU."""
    return SCAN.expected(fmt, seed, iters)


def images(fmt, seed: int = DEFAULT_SEED, step: int = 0):
    """The register images of one step, as the kernel feeds them to the instruction: (A
    uint32[4 waves, 64 lanes, 4 dwords] of kept elements, B uint32[4, 64, 8] dense, index words
    uint32[4, 64], the ``abid`` of that step). Host only, no GPU."""
    import numpy as np

    bit = bit_of(fmt)
    SCAN.check_int(seed, 0, (1 << 64) - 1, "seed")
    SCAN.check_int(step, 0, MAX_ITERS - 1, "step")
    a = np.empty(4 * 64 * A_DWORDS, dtype=np.uint32)
    b = np.empty(4 * 64 * B_DWORDS, dtype=np.uint32)
    idx = np.empty(4 * 64, dtype=np.uint32)
    abid = C.c_uint32(0)
    u32p = C.POINTER(C.c_uint32)
    _check(_native.probe().gm_probe_sparsescan_images(
        bit, seed, step, a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), idx.ctypes.data_as(u32p),
        C.byref(abid)), "sparse-scan images")
    return a.reshape(4, 64, A_DWORDS), b.reshape(4, 64, B_DWORDS), idx.reshape(4, 64), abid.value


def signature(fmt, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None):
    """One block of the scan's device code on the current device: (uint32[256, 4] raw signature,
    where), ``where`` as :func:`gpumounter_amd.ops.cuscan.signature` gives it."""
    return SCAN.signature(fmt, seed, iters, stream)


def _image_arg(x, shape, what):
    import numpy as np

    arr = np.asarray(x)
    if arr.shape != shape or arr.dtype != np.uint32:
        raise ProbeError(f"sparse-scan apply: {what} must be uint32{list(shape)}, got "
                         f"{arr.dtype}{list(arr.shape)}")
    return np.ascontiguousarray(arr)


def apply(fmt, abid: int, a, b, idx):
    """One instruction of ``fmt`` per wave on the current device, on register images the caller
    built (shaped as :func:`images` returns them), from a zero accumulator: numpy uint32[256, 16],
    the bit patterns of thread t's accumulator registers. A 16x16 form fills the first 4 and
    zeroes the rest. ``abid`` is 0 or 1, and 1 only for a 16-bit form."""
    import numpy as np

    bit = bit_of(fmt)
    SCAN.check_int(abid, 0, 1, "abid")
    if abid and FORMAT_NAMES[bit] not in WIDE_FORMATS:
        raise ProbeError(f"sparse-scan apply: {FORMAT_NAMES[bit]!r} has one index set, abid must "
                         f"be 0")
    a = _image_arg(a, (4, 64, A_DWORDS), "A")
    b = _image_arg(b, (4, 64, B_DWORDS), "B")
    idx = _image_arg(idx, (4, 64), "the index words")
    import torch        # only once every refusal is behind: a refused call needs no GPU stack

    dev = [torch.from_numpy(x.view(np.int32).reshape(-1)).to("cuda") for x in (a, b, idx)]
    out = torch.zeros(cuframe.THREADS * ACC_WORDS, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream(out.device)
    with torch.cuda.device(out.device):
        _check(_native.probe().gm_probe_sparsescan_apply(
            bit, abid, *(t.data_ptr() for t in dev), out.data_ptr(), C.c_void_p(s.cuda_stream)),
            "sparse-scan apply")
    s.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(cuframe.THREADS, ACC_WORDS)


def scan(dev: int, formats=ALL_FORMATS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None) -> Dict:
    """The scan of device ``dev``; rounds, ``ok`` and ``complete`` as in
    :func:`gpumounter_amd.ops.cuscan.scan`, whose result shape this has with ``formats``,
    ``formats_failed`` and a record's ``format`` in place of ``tests``, ``tests_failed`` and
    ``test``. ``_inject=(id or "any", format, thread, word, mask)`` is the negative control."""
    return SCAN.scan(dev, formats, iters, seed, min_rounds, max_rounds, _inject)
