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
from typing import Dict, Iterable, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops import cuscan
from gpumounter_amd.ops.cuscan import ANY, DEFAULT_SEED, MAX_ROUNDS, THREADS, WORDS
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


def bit_of(fmt) -> int:
    """The bit of one format, given by name or by bit."""
    if isinstance(fmt, str) and fmt in FORMATS:
        return FORMATS[fmt]
    if isinstance(fmt, int) and not isinstance(fmt, bool) and fmt in FORMAT_NAMES:
        return fmt
    raise ProbeError(f"unknown mfma-scan format {fmt!r} (one of {', '.join(FORMATS)})")


def mask_of(formats: Iterable) -> int:
    if isinstance(formats, (str, int)):
        formats = (formats,)
    mask = 0
    for f in formats:
        mask |= bit_of(f)
    if not mask:
        raise ProbeError("mfma-scan needs at least one format")
    return mask


def parse_formats(text) -> Tuple[str, ...]:
    """``"fp8,mxfp4"`` → ("fp8", "mxfp4"); every name is checked."""
    names = tuple(t.strip() for t in str(text).split(",") if t.strip())
    mask_of(names)
    return names


def _int(v, lo: int, hi: int, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ProbeError(f"mfma-scan: {what} must be an integer in [{lo}, {hi}], got {v!r}")
    return v


def _inject_arg(inject, mask: int):
    """(id or "any", format, thread, word, xor mask) → the C struct; None stays None."""
    if inject is None:
        return None
    try:
        cu_id, fmt, thread, word, xor = inject
    except (TypeError, ValueError):
        raise ProbeError(f"mfma-scan: injection {inject!r} is not (id, format, thread, word, "
                         f"mask)") from None
    bit = bit_of(fmt)
    if not bit & mask:
        raise ProbeError(f"mfma-scan: injection into {FORMAT_NAMES[bit]!r}, which is not run")
    if cu_id != ANY:
        cuscan.decode_id(cu_id)
    _int(thread, 0, THREADS - 1, "injection thread")
    _int(word, 0, WORDS - 1, "injection word")
    _int(xor, 1, 0xFFFFFFFF, "injection mask")
    return _native.CuscanInject(_native.CUSCAN_ANY if cu_id == ANY else cu_id, bit, thread, word,
                                xor)


def parse_inject(text):
    """``"ID|any:FORMAT:THREAD:WORD:MASK"`` (integers as Python literals, e.g.
    ``0x123:mxfp4:130:2:0x10000``) → (id or "any", format name, thread, word, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    if len(parts) != 5:
        raise ProbeError(f"mfma-scan: cannot read {text!r} as ID|any:FORMAT:THREAD:WORD:MASK")
    try:
        cu_id = ANY if parts[0].lower() == ANY else int(parts[0], 0)
        thread, word, xor = (int(p, 0) for p in parts[2:])
    except ValueError:
        raise ProbeError(f"mfma-scan: {text!r} holds something that is not an integer") from None
    inj = (cu_id, FORMAT_NAMES[bit_of(parts[1])], thread, word, xor)
    _inject_arg(inj, FORMATS[inj[1]])
    return inj


def expected(fmt, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS):
    """numpy uint32[256, 4]: word i of thread t of ``fmt``'s signature. Host only, no GPU."""
    import numpy as np

    bit = bit_of(fmt)
    _int(seed, 0, (1 << 64) - 1, "seed"), _int(iters, 1, MAX_ITERS, "iters")
    out = np.empty(THREADS * WORDS, dtype=np.uint32)
    _check(_native.probe().gm_probe_mfmascan_expected(
        bit, seed, iters, out.ctypes.data_as(C.POINTER(C.c_uint32))), "mfma-scan expected")
    return out.reshape(THREADS, WORDS)


def images(fmt, seed: int = DEFAULT_SEED, step: int = 0):
    """The operand register images of one step, as the kernel feeds them to the instruction:
    (uint32[4 waves, 2 operands, 64 lanes, 8 dwords], uint32[4, 2, 16] E8M0 scale bytes; 127 for
    a format without scales). Host only, no GPU."""
    import numpy as np

    bit = bit_of(fmt)
    _int(seed, 0, (1 << 64) - 1, "seed"), _int(step, 0, MAX_ITERS - 1, "step")
    img = np.empty(4 * 2 * 64 * 8, dtype=np.uint32)
    sc = np.empty(4 * 2 * 16, dtype=np.uint32)
    _check(_native.probe().gm_probe_mfmascan_images(
        bit, seed, step, img.ctypes.data_as(C.POINTER(C.c_uint32)),
        sc.ctypes.data_as(C.POINTER(C.c_uint32))), "mfma-scan images")
    return img.reshape(4, 2, 64, 8), sc.reshape(4, 2, 16)


def signature(fmt, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None):
    """One block of the scan's device code on the current device: (uint32[256, 4] raw signature,
    where), ``where`` as :func:`gpumounter_amd.ops.cuscan.signature` gives it."""
    bit = bit_of(fmt)
    _int(seed, 0, (1 << 64) - 1, "seed"), _int(iters, 1, MAX_ITERS, "iters")
    import numpy as np
    import torch

    out = torch.zeros(THREADS * WORDS, dtype=torch.int32, device="cuda")
    where = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream(out.device)
    with torch.cuda.device(out.device):
        _check(_native.probe().gm_probe_mfmascan_signature(
            bit, seed, iters, out.data_ptr(), where.data_ptr(), C.c_void_p(s.cuda_stream)),
            "mfma-scan signature")
    s.synchronize()
    w = [int(v) & 0xFFFFFFFF for v in where.cpu().tolist()]
    sig = out.cpu().numpy().view(np.uint32).reshape(THREADS, WORDS)
    return sig, {"id": w[0], **cuscan.decode_id(w[0] & (_native.CUSCAN_IDS - 1)), "simds": w[1:]}


def scan(dev: int, formats=ALL_FORMATS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None) -> Dict:
    """The scan of device ``dev``; rounds, ``ok`` and ``complete`` as in
    :func:`gpumounter_amd.ops.cuscan.scan`, whose result shape this has with ``formats``,
    ``formats_failed`` and a record's ``format`` in place of ``tests``, ``tests_failed`` and
    ``test``. ``_inject=(id or "any", format, thread, word, mask)`` is the negative control."""
    mask = mask_of(formats)
    _int(iters, 1, MAX_ITERS, "iters")
    _int(dev, 0, (1 << 31) - 1, "device")
    _int(seed, 0, (1 << 64) - 1, "seed")
    _int(min_rounds, 1, MAX_ROUNDS, "min_rounds")
    _int(max_rounds, min_rounds, MAX_ROUNDS, "max_rounds (at least min_rounds)")
    inj = _inject_arg(_inject, mask)
    res = _native.CuscanResult()
    cus = (_native.CuscanCu * _native.CUSCAN_IDS)()
    n = C.c_int(0)
    _check(_native.probe().gm_probe_mfmascan(
        dev, mask, iters, seed, min_rounds, max_rounds,
        C.byref(inj) if inj is not None else None, C.byref(res), cus,
        _native.CUSCAN_IDS, C.byref(n)), "mfma-scan")
    return cuscan.decode_result(dev, mask, iters, res, cus, n.value, FORMATS, "formats")


def describe_failed(result: Dict) -> str:
    """One line naming the failed units of a :func:`scan` result as the CU scan names them, with
    the formats that failed there, for ``doctor``."""
    return cuscan.describe_failed(result, "formats")
