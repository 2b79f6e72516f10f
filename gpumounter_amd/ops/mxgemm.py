"""The block-scaled (MX) GEMM burn-in (native/hip/gm_mxgemm.hip; value model in
native/include/gm_mxgemm_ref.h, formulas in native/include/gm_probe.h).

The bf16 burn-in (:func:`probe.burn_in`) loads only the bf16 matrix pipe. This is the same check
on the pipe inference tenants use: a real GEMM, HBM → LDS → ``v_mfma_scale_f32_16x16x128_f8f6f4``
→ HBM, on OCP fp8 (``mxfp8``, e4m3) or fp4 (``mxfp4``, e2m1) operands with one E8M0 scale per 32
elements of K, run for seconds with every result compared bit for bit with the first.

Operands are K-major and packed: ``A [M, K]`` and ``Bt [N, K]`` as uint8 tensors of ``K`` (fp8) or
``K / 2`` (fp4, low nibble first) bytes per row, scales as uint8 ``[rows, K / 32]``, 127 = 1.0;
``C [M, N]`` is bf16. Three operand classes (:data:`CLASSES`): ``exact`` and ``blocks`` have one
definite result in any summation order, which :func:`expected` gives bit for bit; ``random`` is
the burn-in's load, for which :func:`expected` gives the float64 sum and the sum of |products|.

Every refusal is raised here, as :class:`ProbeError`, before the native call.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops import probe
from gpumounter_amd.ops.probe import ProbeError, _check

FORMATS = ("mxfp8", "mxfp4")
CLASSES = ("exact", "blocks", "random")
FORMAT_CODE = {"mxfp8": 0, "mxfp4": 4}      # the instruction's format field
TILE_K = {"mxfp8": 128, "mxfp4": 256}       # elements of K in one K-tile (128 bytes of a row)
TILE_MN = 256
BLOCK = 32                                  # elements of K that share one scale


def _fmt(fmt) -> int:
    if fmt not in FORMAT_CODE:
        raise ProbeError(f"mxgemm: unknown format {fmt!r} (one of {', '.join(FORMATS)})")
    return FORMAT_CODE[fmt]


def _cls(cls) -> int:
    if cls not in CLASSES:
        raise ProbeError(f"mxgemm: unknown operand class {cls!r} (one of {', '.join(CLASSES)})")
    return CLASSES.index(cls)


def _seed(seed) -> int:
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 32:
        raise ProbeError("mxgemm: seed must be an integer in [0, 2^32)")
    return seed


def _dims(what: str, **dims) -> None:
    for name, v in dims.items():
        if not isinstance(v, int) or isinstance(v, bool) or not 0 < v < 1 << 31:
            raise ProbeError(f"{what}: {name} = {v!r} is not a positive 32-bit integer")


def row_bytes(fmt: str, k: int) -> int:
    """Bytes of one packed row of ``k`` elements."""
    return k // 2 if _fmt(fmt) == 4 else k


def check_shape(fmt: str, m: int, n: int, k: int) -> None:
    """Refuses what the kernel does not take: M, N multiples of 256, K of the format's K-tile."""
    _fmt(fmt)
    _dims("mxgemm", M=m, N=n, K=k)
    if m % TILE_MN or n % TILE_MN or k % TILE_K[fmt]:
        raise ProbeError(f"mxgemm: {fmt} needs M and N multiples of {TILE_MN} and K a multiple "
                         f"of {TILE_K[fmt]}, got M={m} N={n} K={k}")


def fill(fmt: str, cls: str, seed: int, rows: int, k: int, device=None, stream=None):
    """(elements, scales) of an operand of ``rows`` rows and ``k`` elements per row (a multiple
    of 32), filled on the device by the fill kernel: uint8 tensors ``[rows, row_bytes]`` and
    ``[rows, k / 32]``. Asynchronous."""
    import torch

    f, c, seed = _fmt(fmt), _cls(cls), _seed(seed)
    _dims("mxgemm fill", rows=rows, K=k)
    if k % BLOCK:
        raise ProbeError(f"mxgemm fill: K = {k} is not a multiple of {BLOCK}")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ProbeError(f"mxgemm fill: {device} is not a HIP device")
    elems = torch.empty((rows, row_bytes(fmt, k)), dtype=torch.uint8, device=device)
    scales = torch.empty((rows, k // BLOCK), dtype=torch.uint8, device=device)
    with torch.cuda.device(elems.device):
        _check(_native.probe().gm_probe_mx_fill(f, c, seed, rows, k, elems.data_ptr(),
                                                scales.data_ptr(),
                                                probe._stream_of(elems, stream)), "mxgemm fill")
    return elems, scales


def _operand(t, what: str, rows: Optional[int], cols: int):
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2:
        raise ProbeError(f"mxgemm: {what} must be a 2-D uint8 torch tensor")
    if t.device.type != "cuda" or not t.is_contiguous():
        raise ProbeError(f"mxgemm: {what} must be contiguous on a HIP device")
    if (rows is not None and t.shape[0] != rows) or t.shape[1] != cols:
        raise ProbeError(f"mxgemm: {what} is {tuple(t.shape)}, expected "
                         f"[{'rows' if rows is None else rows}, {cols}]")
    if t.data_ptr() % 16:
        raise ProbeError(f"mxgemm: {what}'s storage is not 16-byte aligned")


def _operands(fmt: str, a, sa, bt, sb, out):
    """The packed operands, their scales and ``out`` (made if None) of one GEMM, checked:
    (M, N, K, out)."""
    import torch

    _fmt(fmt)
    for t, what in ((a, "A"), (sa, "sA"), (bt, "Bt"), (sb, "sB")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ProbeError(f"mxgemm: {what} must be a 2-D uint8 torch tensor")
    m, n, k = int(a.shape[0]), int(bt.shape[0]), int(sa.shape[1]) * BLOCK
    check_shape(fmt, m, n, k)
    _operand(a, "A", m, row_bytes(fmt, k))
    _operand(bt, "Bt", n, row_bytes(fmt, k))
    _operand(sa, "sA", m, k // BLOCK)
    _operand(sb, "sB", n, k // BLOCK)
    if len({t.device for t in (a, sa, bt, sb)}) != 1:
        raise ProbeError("mxgemm: the operands are on different devices")
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    elif (not isinstance(out, torch.Tensor) or out.shape != (m, n) or out.dtype != torch.bfloat16
          or not out.is_contiguous() or out.device != a.device):
        raise ProbeError(f"mxgemm: out must be a contiguous bf16 [{m}, {n}] tensor on {a.device}")
    return m, n, k, out


def gemm_nt(fmt: str, a, sa, bt, sb, out=None, stream=None):
    """C (bf16 [M, N]) = A · Btᵀ for packed operands and their scales on a HIP device (the
    layouts of :func:`fill`). M and N multiples of 256; K = 32 × the scales' columns, a multiple
    of the format's K-tile. Asynchronous."""
    import torch

    m, n, k, out = _operands(fmt, a, sa, bt, sb, out)
    with torch.cuda.device(a.device):
        _check(_native.probe().gm_probe_mxgemm_nt(FORMAT_CODE[fmt], a.data_ptr(), sa.data_ptr(),
                                                  bt.data_ptr(), sb.data_ptr(), out.data_ptr(),
                                                  m, n, k, probe._stream_of(a, stream)),
               "mxgemm")
    return out


def expected(fmt: str, cls: str, seed_a: int, seed_b: int, m: int, n: int, k: int):
    """What the GEMM of operands filled with ``(fmt, cls, seed_a)`` and ``(fmt, cls, seed_b)``
    must give, computed on the host (no GPU), for any M, N and K a multiple of 32.

    ``exact`` and ``blocks``: a numpy uint16 array ``[m, n]`` of bf16 bit patterns, the exact
    integer sum rounded once. ``random``: ``(ref, abs_sum)``, two float64 arrays: the sum in k
    order and the sum of |products|."""
    import numpy as np

    f, c = _fmt(fmt), _cls(cls)
    seed_a, seed_b = _seed(seed_a), _seed(seed_b)
    _dims("mxgemm expected", M=m, N=n, K=k)
    if k % BLOCK:
        raise ProbeError(f"mxgemm expected: K = {k} is not a multiple of {BLOCK}")
    lib = _native.probe()
    if cls == "random":
        ref, s = np.empty((m, n), np.float64), np.empty((m, n), np.float64)
        _check(lib.gm_probe_mxgemm_expected(f, c, seed_a, seed_b, m, n, k, None,
                                            ref.ctypes.data, s.ctypes.data), "mxgemm expected")
        return ref, s
    out = np.empty((m, n), np.uint16)
    _check(lib.gm_probe_mxgemm_expected(f, c, seed_a, seed_b, m, n, k, out.ctypes.data, None,
                                        None), "mxgemm expected")
    return out


def kernel_info(fmt: str = "mxfp8") -> Dict[str, int]:
    """Registers and scratch bytes of the format's GEMM kernel: the accumulators must stay in
    registers, so ``scratch_bytes`` must be 0."""
    f, regs, scratch = _fmt(fmt), C.c_int(0), C.c_int(0)
    _check(_native.probe().gm_probe_mxgemm_kernel_info(f, C.byref(regs),
                                                       C.byref(scratch)), "mxgemm kernel info")
    return {"num_regs": regs.value, "scratch_bytes": scratch.value}


def gemm_nt_traced(fmt: str, a, sa, bt, sb, r: int = 0, out=None, _inject=None, stream=None):
    """:func:`gemm_nt` through the attributed burn-in's kernel at rotation ``r``: (C,
    cu_of_tile), as :func:`probe.gemm_nt_traced`. Asynchronous."""
    import torch

    m, n, k, out = _operands(fmt, a, sa, bt, sb, out)
    grid = (m // TILE_MN) * (n // TILE_MN)
    inj = probe._traced_args("mxgemm traced", r, grid, _inject)
    cus = torch.full((grid,), -1, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        _check(_native.probe().gm_probe_mxgemm_nt_traced(
            FORMAT_CODE[fmt], a.data_ptr(), sa.data_ptr(), bt.data_ptr(), sb.data_ptr(),
            out.data_ptr(), m, n, k, r, cus.data_ptr(), C.byref(inj) if inj else None,
            probe._stream_of(a, stream)), "mxgemm traced")
    return out, cus


def burn_in(dev: int, seconds: float, fmt: str, n: int = 8192,
            _flips: Optional[Sequence[Tuple[int, int]]] = None, attribute: bool = False,
            _inject=None) -> Dict:
    """:func:`probe.burn_in` on the block-scaled pipe: back-to-back n³ GEMMs of ``fmt`` on
    random-class operands for ``seconds``, each result compared bit for bit with the first.
    Returns :func:`probe.burn_in`'s dict plus ``"format"``; ``tflops`` counts 2 n³ per GEMM.
    ``_flips`` as there: bf16 elements of the n × n reference result. ``attribute`` and
    ``_inject`` as there too: the rotated tile map, the CU of every block and ``"attribution"``."""
    check_shape(fmt, n, n, n)
    if not isinstance(seconds, (int, float)) or isinstance(seconds, bool) or not seconds > 0:
        raise ProbeError(f"mx burn-in: seconds = {seconds!r} is not a positive number")
    out = probe._run_burn_in(f"{fmt} burn-in", "gm_probe_mx_burn_in", (dev, FORMAT_CODE[fmt]), dev,
                             n, seconds, _flips, attribute, _inject)
    out["format"] = fmt
    return out


BURN_IN_FORMATS = ("bf16",) + FORMATS


def parse_burn_in_formats(text) -> Tuple[str, ...]:
    """``"bf16,mxfp4"`` → the chosen burn-in formats, in the order of :data:`BURN_IN_FORMATS`."""
    names = [t.strip() for t in str(text).split(",")]
    for name in names:
        if name not in BURN_IN_FORMATS:
            raise ProbeError(f"burn-in: unknown format {name!r} (of "
                             f"{','.join(BURN_IN_FORMATS)})")
    return tuple(f for f in BURN_IN_FORMATS if f in names)


def burn_in_key(fmt: str) -> str:
    """The report key of a format's burn-in: bf16's stays ``burn_in``."""
    return "burn_in" if fmt == "bf16" else f"burn_in_{fmt}"


def run_burn_in(dev: int, seconds: float, fmt: str, _flips=None, attribute: bool = False,
                _inject=None) -> Dict:
    """One chosen format's burn-in at the default size: what probe, doctor and validate run.
    Only what was asked for is handed down: no keyword for a control that is not given."""
    more = {} if _flips is None else {"_flips": _flips}
    if attribute:
        more["attribute"] = True
    if _inject is not None:
        more["_inject"] = _inject
    if fmt == "bf16":
        return probe.burn_in(dev, seconds, **more)
    return burn_in(dev, seconds, fmt, **more)


def attribute_kwargs(attribute, inject) -> Dict:
    """The keyword arguments :func:`run_burn_in` takes for ``--burn-in-attribute`` and
    ``--burn-in-inject``: none where neither is given."""
    more = {"attribute": True} if attribute else {}
    if inject is not None:
        more["_inject"] = inject
    return more
