"""Python side of the gfx950 post-attach validation kernels (native/hip/gm_probe.hip; the burn-in
GEMM in native/hip/gm_gemm.hip).

An attach is only useful if the tenant can actually run work on the GPU. After the node operations
succeed, a tenant-side agent (or the bench ranks) call :func:`verify` on the newly attached devices:
a wave64 liveness kernel (every lane writes, a 64-lane shuffle reduction and a 64-bit ballot are
checked), and optionally an HBM3E stream, an MFMA bf16 peak and an MFMA GEMM numerics check.
No silent fallback: if ``libgm_probe.so`` is missing or HIP fails, this raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import asdict, dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

from gpumounter_amd import _native


class ProbeError(RuntimeError):
    pass


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = _native.probe().gm_probe_strerror(rc).decode(errors="replace")
        raise ProbeError(f"{what}: hip error {rc} ({msg})")


def device_count() -> int:
    n = C.c_int(0)
    _check(_native.probe().gm_probe_device_count(C.byref(n)), "hipGetDeviceCount")
    return n.value


def props(dev: int) -> Dict:
    p = _native.ProbeProps()
    _check(_native.probe().gm_probe_props(dev, C.byref(p)), "props")
    return {"name": p.name.decode(), "gcn_arch": p.gcn_arch.decode(),
            "pci_bus_id": p.pci_bus_id.decode().lower(), "cu_count": p.cu_count,
            "warp_size": p.warp_size, "total_mem": p.total_mem,
            "lds_per_block": p.lds_per_block, "clock_khz": p.clock_khz}


def find_device(bdf: str) -> int:
    """HIP device index of the GPU at PCI address ``bdf`` (-1 if not visible)."""
    d = C.c_int(-1)
    _check(_native.probe().gm_probe_find_device(bdf.encode(), C.byref(d)), "find_device")
    return d.value


QUICK_WORDS = 66              # 64 lane words, the reduction sum (word 64), the ballot count (65)
QUICK_BAD_LANES, QUICK_BAD_SUM, QUICK_BAD_BALLOT = 1, 2, 4
_QUICK_CHECKS = ((QUICK_BAD_LANES, "lane words"), (QUICK_BAD_SUM, "reduction sum"),
                 (QUICK_BAD_BALLOT, "ballot count"))


def quick(dev: int, _flip: Optional[Tuple[int, int]] = None) -> float:
    """Liveness kernel; returns launch→readback µs. Raises if the wave64 checks fail.
    ``_flip=(word, mask)`` is the negative control: that one of the 66 words read back is XORed
    with the nonzero 32-bit ``mask`` on the host before the verdict, so the call must raise."""
    ok, us = C.c_int(0), C.c_double(0)
    if _flip is None:
        _check(_native.probe().gm_probe_quick(dev, C.byref(ok), C.byref(us)), "quick probe")
        if not ok.value:
            raise ProbeError(f"device {dev}: liveness kernel produced wrong results")
        return us.value
    word, mask = _flip
    for v in (word, mask):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << 32:
            raise ProbeError(f"quick probe: flip {_flip!r} is not (word, mask) in 32 bits")
    failed = C.c_uint32(0)
    _check(_native.probe().gm_probe_quick_flip(dev, word, mask, C.byref(ok), C.byref(failed),
                                               C.byref(us)), "quick probe")
    if not ok.value:
        names = ", ".join(n for bit, n in _QUICK_CHECKS if failed.value & bit)
        raise ProbeError(f"device {dev}: liveness kernel produced wrong results ({names})")
    return us.value


def quick_expected(salt: int) -> List[int]:
    """The 66 words the liveness kernel must produce for ``salt`` (host only; gm_probe.h)."""
    words = (C.c_uint32 * QUICK_WORDS)()
    _check(_native.probe().gm_probe_quick_expected(salt, words), "quick expected")
    return list(words)


def quick_verdict(words: Sequence[int], salt: int) -> int:
    """The host verdict over 66 received words: 0 if healthy, else the QUICK_BAD_* bits of the
    checks that failed (host only)."""
    if len(words) != QUICK_WORDS:
        raise ProbeError(f"quick verdict: {len(words)} words, not {QUICK_WORDS}")
    failed = C.c_uint32(0)
    _check(_native.probe().gm_probe_quick_verdict((C.c_uint32 * QUICK_WORDS)(*words), salt,
                                                  C.byref(failed)), "quick verdict")
    return failed.value


def quick_words(dev: int) -> Tuple[List[int], int]:
    """One run of the liveness kernel on ``dev``: (the 66 raw words read back, the salt used)."""
    words, salt = (C.c_uint32 * QUICK_WORDS)(), C.c_uint32(0)
    _check(_native.probe().gm_probe_quick_words(dev, words, C.byref(salt)), "quick words")
    return list(words), salt.value


def hbm_gbps(dev: int, nbytes: int = 1 << 30, iters: int = 10) -> float:
    g = C.c_double(0)
    _check(_native.probe().gm_probe_hbm_copy(dev, nbytes, iters, C.byref(g)), "hbm copy")
    return g.value


def hbm_read_gbps(dev: int, nbytes: int = 1 << 30, iters: int = 10,
                  blocks_per_cu: int = 2) -> float:
    g = C.c_double(0)
    _check(_native.probe().gm_probe_hbm_read(dev, nbytes, iters, blocks_per_cu, C.byref(g)),
           "hbm read")
    return g.value


def mfma_tflops(dev: int, iters: int = 20000) -> float:
    t = C.c_double(0)
    _check(_native.probe().gm_probe_mfma_peak(dev, iters, C.byref(t)), "mfma peak")
    return t.value


MFMA_PEAK_FLOATS = (64, 16, 32)    # accumulator floats per thread: chains × registers


def mfma_peak_values(variant: int, iters: int, seed: float, blocks: int, out=None, stream=None):
    """What MFMA peak kernel ``variant`` (0..2) computes: one launch of ``blocks`` blocks through
    the timed driver's launch, every thread storing its accumulators after the loop. Returns an
    fp32 tensor [blocks, 256, chains, registers] (4×16, 4×4, 8×4; operands and lane maps in
    gm_probe.h). ``out``, if given, is a contiguous fp32 device tensor of exactly that many
    elements; otherwise one is made on the current device. Waits for the kernel."""
    import torch

    if variant not in (0, 1, 2) or not isinstance(blocks, int) or blocks <= 0:
        raise ProbeError(f"mfma_peak_values: variant {variant!r} or blocks {blocks!r}")
    per = MFMA_PEAK_FLOATS[variant]
    if out is None:
        out = torch.empty(blocks * 256 * per, dtype=torch.float32, device="cuda")
    elif out.dtype != torch.float32 or out.numel() != blocks * 256 * per:
        raise ProbeError(f"mfma_peak_values: out must hold {blocks * 256 * per} fp32")
    _dev_bytes(out, "mfma_peak_values")
    with torch.cuda.device(out.device):
        _check(_native.probe().gm_probe_mfma_peak_values(variant, iters, seed, blocks,
                                                         out.data_ptr(), _stream_of(out, stream)),
               "mfma peak values")
    return out.view(blocks, 256, 4 if variant < 2 else 8, 16 if variant == 0 else 4)


def gemm_check(dev: int, m: int = 256, n: int = 256, k: int = 256) -> Dict[str, float]:
    err, scale = C.c_double(0), C.c_double(0)
    _check(_native.probe().gm_probe_gemm_check(dev, m, n, k, C.byref(err), C.byref(scale)),
           "gemm check")
    return {"max_abs_err": err.value, "ref_scale": scale.value}


def gemm_bf16(a, b, out=None, stream=None):
    """C(fp32) = A(bf16) @ B(bf16) on MFMA for torch tensors on a HIP device.

    Shapes: A [M,K], B [K,N] contiguous; M, N multiples of 64 and K a multiple of 32.
    """
    import torch

    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise ProbeError("gemm_bf16 expects bf16 inputs")
    if not (a.is_contiguous() and b.is_contiguous()):
        raise ProbeError("gemm_bf16 expects contiguous inputs")
    m, k = a.shape
    k2, n = b.shape
    if k != k2 or m % 64 or n % 64 or k % 32:
        raise ProbeError(f"unsupported shape A{tuple(a.shape)} B{tuple(b.shape)}")
    if a.device != b.device:
        raise ProbeError(f"gemm_bf16: A on {a.device}, B on {b.device}")
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    elif (not isinstance(out, torch.Tensor) or out.shape != (m, n) or out.dtype != torch.float32
          or not out.is_contiguous() or out.device != a.device):
        raise ProbeError(f"gemm_bf16: out must be a contiguous fp32 [{m},{n}] tensor on "
                         f"{a.device}")
    s = stream if stream is not None else torch.cuda.current_stream(a.device)
    with torch.cuda.device(a.device):
        _check(_native.probe().gm_probe_gemm_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                  m, n, k, C.c_void_p(s.cuda_stream)),
               "gemm_bf16")
    return out


def _nt_operands(what: str, a, bt, out):
    """A bf16 NT operand pair, A [M,K] and Bt [N,K], and ``out`` (made if None), checked for the
    256²-tile GEMM: (M, N, K, out)."""
    import torch

    if a.dtype != torch.bfloat16 or bt.dtype != torch.bfloat16:
        raise ProbeError(f"{what} expects bf16 inputs")
    if not (a.is_contiguous() and bt.is_contiguous()):
        raise ProbeError(f"{what} expects contiguous inputs")
    m, k = a.shape
    n, k2 = bt.shape
    if k != k2 or m % 256 or n % 256 or k % 64:
        raise ProbeError(f"unsupported shape A{tuple(a.shape)} Bt{tuple(bt.shape)}")
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    elif out.shape != (m, n) or out.dtype != torch.bfloat16 or not out.is_contiguous():
        raise ProbeError(f"{what}: out must be a contiguous bf16 [M,N] tensor")
    return m, n, k, out


def gemm_nt(a, bt, out=None, stream=None, variant: Optional[int] = None):
    """C(bf16) = A @ Btᵀ for bf16 torch tensors on a HIP device: the 256²-tile
    global_load_lds MFMA GEMM (gm_probe_gemm_nt). Shapes: A [M,K], Bt [N,K] contiguous
    (both K-major); M, N multiples of 256 and K a multiple of 64. ``variant`` picks a schedule
    (1: whole K-tile of fragment reads up front, 5: local-read prefetch across the barrier;
    default: the faster, 5 — profiles/history/r1_gemm)."""
    import torch

    m, n, k, out = _nt_operands("gemm_nt", a, bt, out)
    s = stream if stream is not None else torch.cuda.current_stream(a.device)
    with torch.cuda.device(a.device):
        lib = _native.probe()
        ptrs = (a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k, C.c_void_p(s.cuda_stream))
        rc = (lib.gm_probe_gemm_nt(*ptrs) if variant is None
              else lib.gm_probe_gemm_nt_variant(variant, *ptrs))
        _check(rc, "gemm_nt")
    return out


def gemm_tflops(dev: int, m: int = 8192, n: int = 8192, k: int = 8192, iters: int = 10) -> float:
    """Dense bf16 TF/s of the 256²-tile GEMM on uniform [-1,1] operands (burn-in load)."""
    t = C.c_double(0)
    _check(_native.probe().gm_probe_gemm_nt_tflops(dev, m, n, k, iters, C.byref(t)),
           "gemm tflops")
    return t.value


def parse_burn_in_flip(text) -> Tuple[int, int]:
    """``"ELEM:MASK"`` (any Python integer literal, e.g. ``8:0x8000``) → (element, mask): a bf16
    element index of the burn-in's reference result and a nonzero 16-bit XOR mask."""
    try:
        elem, mask = str(text).split(":")
        elem, mask = int(elem, 0), int(mask, 0)
    except ValueError:
        raise ProbeError(f"burn-in: cannot read {text!r} as ELEM:MASK") from None
    if elem < 0 or not 0 < mask < 1 << 16:
        raise ProbeError(f"burn-in: flip {text!r} needs ELEM >= 0 and 0 < MASK < 0x10000")
    return elem, mask


def _burn_in_flips(_flips, n: int):
    """The burn-ins' flip control, checked: (element indices, the two native arrays)."""
    flips = list(_flips or ())
    elems = [e for e, _ in flips]
    for e, m in flips:
        if not (isinstance(e, int) and isinstance(m, int) and 0 <= e < n * n and 0 < m < 1 << 16):
            raise ProbeError(f"burn-in: flip ({e!r}, {m!r}) needs 0 <= elem < n*n and a nonzero "
                             f"16-bit mask")
    if len(set(elems)) != len(elems):
        raise ProbeError("burn-in: an element may be flipped only once")
    fe = (C.c_uint64 * max(1, len(flips)))(*elems)
    fm = (C.c_uint16 * max(1, len(flips)))(*[m for _, m in flips])
    return elems, fe, fm


def _burn_in_report(dev: int, n: int, seconds: float, elems, tf, bad, it) -> Dict:
    out = {"device": dev, "n": n, "seconds": seconds, "iterations": it.value,
           "tflops": tf.value, "mismatches": bad.value, "ok": bad.value == 0}
    if elems:
        out["flipped_words"] = len({e // 8 for e in elems})
    return out


BURN_IN_FIRST = "first"       # an injection into the CU that computed tile 0 in the warm-up
BURN_IN_TILE = 256


def _burn_in_id(v, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < _native.CUSCAN_IDS:
        raise ProbeError(f"burn-in: {what} {v!r} is not an integer in [0, "
                         f"{_native.CUSCAN_IDS})")
    return v


def parse_burn_in_inject(text) -> Tuple:
    """``"ID:MASK"`` or ``"first:MASK"`` (Python integer literals, e.g. ``0x123:0x1``) → (a
    12-bit CU id or ``"first"``, a nonzero 16-bit XOR mask): the attributed burn-in's injection."""
    try:
        cu_id, mask = (p.strip() for p in str(text).split(":"))
        cu_id = BURN_IN_FIRST if cu_id.lower() == BURN_IN_FIRST else int(cu_id, 0)
        mask = int(mask, 0)
    except ValueError:
        raise ProbeError(f"burn-in: cannot read {text!r} as ID|first:MASK") from None
    _burn_in_inject((cu_id, mask), True)
    return cu_id, mask


def _burn_in_inject(_inject, attribute: bool) -> Optional[_native.BurninInject]:
    """The attributed burn-ins' injection, checked: None, or the native struct."""
    if _inject is None:
        return None
    if not attribute:
        raise ProbeError("burn-in: an injection needs attribute=True (it is a statement about a "
                         "CU, and only the attributed burn-in knows the CUs)")
    try:
        cu_id, mask = _inject
    except (TypeError, ValueError):
        raise ProbeError(f"burn-in: injection {_inject!r} is not (id or 'first', mask)") from None
    if cu_id != BURN_IN_FIRST:
        _burn_in_id(cu_id, "injection id")
    if not isinstance(mask, int) or isinstance(mask, bool) or not 0 < mask < 1 << 16:
        raise ProbeError(f"burn-in: injection mask {mask!r} is not a nonzero 16-bit integer")
    first = cu_id == BURN_IN_FIRST
    return _native.BurninInject(0 if first else cu_id, mask, int(first))


def _blamed_units(blamed, n: int) -> List[Dict]:
    from gpumounter_amd.ops import cuframe

    return [{"id": b.id, **cuframe.decode_id(b.id), "events": b.events, "words": b.words,
             "as_worker": b.as_worker, "as_reference": b.as_reference}
            for b in blamed[:min(n, len(blamed))]]


def _first_events(attr) -> List[Dict]:
    return [{"iteration": e.iteration, "tile": e.tile, "worker": e.worker,
             "reference": e.reference, "words": e.words}
            for e in attr.records[:attr.records_filled]]


def _attribution(attr, blamed) -> Dict:
    """The ``attribution`` dict of an attributed burn-in from the C structures."""
    units = _blamed_units(blamed, attr.n_blamed)
    out = {"tiles": attr.tiles, "grid": attr.grid, "step": attr.step,
           "rotations": attr.rotations, "cus_seen": attr.cus_seen,
           "tiles_moved": attr.tiles_moved, "tiles_exonerated": attr.tiles_exonerated,
           "events": attr.events, "logged": attr.logged,
           "log_overflow": bool(attr.log_overflow), "first_id": attr.first_id,
           "blamed": units, "first_events": _first_events(attr)}
    if attr.inject_id != _native.CUSCAN_ANY:
        out["inject_id"] = attr.inject_id
    if attr.log_overflow:
        out["note"] = (f"{attr.events - attr.logged} of the {attr.events} events were counted "
                       f"but not logged: only the logged ones are blamed")
    return out


def _run_burn_in(what: str, stem: str, lead: tuple, dev: int, n: int, seconds: float, _flips,
                 attribute: bool, _inject) -> Dict:
    """One burn-in through the native entry point ``{stem}_flip`` or, attributed, ``{stem}_attr``
    (``lead``: what they take before ``n``): the controls checked, the call, the report."""
    elems, fe, fm = _burn_in_flips(_flips, n)
    inj = _burn_in_inject(_inject, attribute)
    tf, bad, it = C.c_double(0), C.c_uint64(0), C.c_int(0)
    args, outs = (*lead, n, seconds, len(elems), fe, fm), (C.byref(tf), C.byref(bad), C.byref(it))
    if attribute:
        attr = _native.BurninAttr()
        blamed = (_native.BurninBlamed * _native.BURNIN_LOG_CAP)()
        _check(getattr(_native.probe(), f"{stem}_attr")(
            *args, C.byref(inj) if inj else None, *outs, C.byref(attr), blamed, len(blamed)), what)
    else:
        _check(getattr(_native.probe(), f"{stem}_flip")(*args, *outs), what)
    out = _burn_in_report(dev, n, seconds, elems, tf, bad, it)
    if attribute:
        out["attribution"] = _attribution(attr, blamed)
    return out


def describe_blamed(result: Dict) -> str:
    """One line naming the units an attributed burn-in blames (the first four, then how many
    more), in the words the scans use, for ``doctor``."""
    blamed = result["attribution"]["blamed"]
    text = "; ".join(
        f"xcc {b['xcc']} se {b['se']} sh {b['sh']} cu {b['cu']} (id {b['id']:#05x}) "
        + " + ".join(f"{b[k]} as {k[3:]}" for k in ("as_worker", "as_reference") if b[k])
        for b in blamed[:4])
    return text + (f"; and {len(blamed) - 4} more" if len(blamed) > 4 else "")


def burn_in_tile_map(n: int, r: int = 0) -> Tuple[List[int], int]:
    """Host only: (the tile, row-major over the (n / 256)² tiles, that each block of the
    burn-in GEMM's grid computes at rotation ``r``; the rotation's step for that grid)."""
    if not isinstance(n, int) or isinstance(n, bool) or n <= 0 or n % BURN_IN_TILE:
        raise ProbeError(f"burn-in: n = {n!r} is not a positive multiple of {BURN_IN_TILE}")
    grid = (n // BURN_IN_TILE) ** 2
    if not isinstance(r, int) or isinstance(r, bool) or not 0 <= r < grid:
        raise ProbeError(f"burn-in: rotation {r!r} is not in [0, {grid})")
    tm, tn, step, tiles = C.c_int(0), C.c_int(0), C.c_int(0), []
    for b in range(grid):
        _check(_native.probe().gm_probe_burn_in_tile_map(n, n, b, r, C.byref(tm), C.byref(tn),
                                                         C.byref(step)), "burn-in tile map")
        tiles.append(tm.value * (n // BURN_IN_TILE) + tn.value)
    return tiles, step.value


def burn_in_blame(events: Sequence[Tuple[int, int, int, int, int]], exonerated: Sequence,
                  counted: Optional[int] = None) -> Dict:
    """Host only: the attributed burn-in's blame rule over a log of (iteration, tile, worker id,
    reference id, words) and one exonerated flag per tile. ``counted``: how many events the run
    counted, where that is more than the log holds."""
    tiles = len(exonerated)
    if tiles == 0:
        raise ProbeError("burn-in blame: no tiles")
    for e in events:
        if len(e) != 5 or not all(isinstance(v, int) and 0 <= v < 1 << 32 for v in e):
            raise ProbeError(f"burn-in blame: event {e!r} is not five 32-bit integers")
        if e[1] >= tiles:
            raise ProbeError(f"burn-in blame: event {e!r} at a tile outside the {tiles}")
        _burn_in_id(e[2], "worker id"), _burn_in_id(e[3], "reference id")
    counted = len(events) if counted is None else counted
    if not isinstance(counted, int) or counted < len(events):
        raise ProbeError(f"burn-in blame: counted = {counted!r} is below the log's length")
    if len(events) < min(counted, _native.BURNIN_LOG_CAP):
        raise ProbeError("burn-in blame: the log is shorter than what was counted and fits")
    ev = (_native.BurninEvent * max(1, len(events)))(*[_native.BurninEvent(*e) for e in events])
    ex = (C.c_uint8 * tiles)(*[1 if x else 0 for x in exonerated])
    attr = _native.BurninAttr()
    blamed = (_native.BurninBlamed * _native.BURNIN_LOG_CAP)()
    _check(_native.probe().gm_probe_burn_in_blame(ev, counted, ex, tiles, C.byref(attr), blamed,
                                                  len(blamed)), "burn-in blame")
    units = _blamed_units(blamed, attr.n_blamed)
    return {"events": attr.events, "logged": attr.logged,
            "log_overflow": bool(attr.log_overflow), "tiles_exonerated": attr.tiles_exonerated,
            "blamed": units, "first_events": _first_events(attr)}


def _traced_args(what: str, r, grid: int, _inject) -> Optional[_native.BurninInject]:
    """What one traced GEMM takes besides its operands, checked: the rotation, and the injection
    (returned as the native struct, or None)."""
    if not isinstance(r, int) or isinstance(r, bool) or not 0 <= r < grid:
        raise ProbeError(f"{what}: rotation {r!r} is not in [0, {grid})")
    inj = _burn_in_inject(_inject, True)
    if inj is not None and inj.first:
        raise ProbeError(f"{what}: one GEMM has no warm-up to take 'first' from")
    return inj


def gemm_nt_traced(a, bt, r: int = 0, out=None, _inject=None, stream=None):
    """:func:`gemm_nt` through the attributed burn-in's kernel at rotation ``r``: (C, cu_of_tile),
    ``cu_of_tile`` an int32 device tensor with the 12-bit id of the CU that computed each tile,
    row-major over the tiles. ``_inject=(id, mask)``: blocks on that CU flip element (0, 0) of
    their tile. Asynchronous."""
    import torch

    m, n, k, out = _nt_operands("gemm_nt_traced", a, bt, out)
    grid = (m // 256) * (n // 256)
    inj = _traced_args("gemm_nt_traced", r, grid, _inject)
    cus = torch.full((grid,), -1, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        _check(_native.probe().gm_probe_gemm_nt_traced(
            a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k, r, cus.data_ptr(),
            C.byref(inj) if inj else None, _stream_of(a, stream)), "gemm_nt_traced")
    return out, cus


def traced_kernel_info(fmt: str = "bf16") -> Dict[str, int]:
    """Registers and scratch bytes of a format's traced GEMM kernel: ``scratch_bytes`` must be
    0, as for the plain kernels."""
    from gpumounter_amd.ops import mxgemm

    regs, scratch = C.c_int(0), C.c_int(0)
    if fmt == "bf16":
        rc = _native.probe().gm_probe_gemm_nt_traced_info(C.byref(regs), C.byref(scratch))
    else:
        rc = _native.probe().gm_probe_mxgemm_nt_traced_info(mxgemm._fmt(fmt), C.byref(regs),
                                                            C.byref(scratch))
    _check(rc, "traced kernel info")
    return {"num_regs": regs.value, "scratch_bytes": scratch.value}


def burn_in(dev: int, seconds: float = 10.0, n: int = 8192,
            _flips: Optional[Sequence[Tuple[int, int]]] = None, attribute: bool = False,
            _inject=None) -> Dict:
    """Sustained-load check of an attached GPU: back-to-back n³ bf16 GEMMs for ``seconds``,
    each compared bit-for-bit with the first result (the kernel is deterministic). Any
    ``mismatches`` means silent data corruption. ``tflops`` is the sustained rate, so
    throttling shows up as a low number. ``_flips=[(elem, mask), ...]`` is the negative control:
    those bf16 elements of the reference result are XORed with ``mask`` before the loop, so
    every iteration must count each 16-byte word they touch.

    ``attribute=True`` rotates the block → tile map from one iteration to the next, so every
    tile is recomputed by other blocks, XCDs and CUs than the reference's, records the CU of
    every block and adds ``"attribution"``: what moved, and the units blamed for mismatches
    (native/include/gm_probe.h, "attributed burn-in"). ``_inject=(id or "first", mask)`` is its
    negative control: every block on that CU XORs ``mask`` into element (0, 0) of its tile, in
    the reference too; ``"first"`` is the CU that computed tile 0 in the warm-up."""
    return _run_burn_in("burn-in", "gm_probe_burn_in", (dev,), dev, n, seconds, _flips, attribute,
                        _inject)


def _dev_bytes(t, what: str, align: int = 16, multiple: int = 16) -> int:
    """Checks a tensor a stream kernel may walk as raw bytes; returns its size in bytes."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ProbeError(f"{what} expects a torch tensor")
    if t.device.type != "cuda":
        raise ProbeError(f"{what} expects a tensor on a HIP device, got {t.device}")
    if not t.is_contiguous():
        raise ProbeError(f"{what} expects a contiguous tensor")
    nbytes = t.numel() * t.element_size()
    if nbytes == 0 or nbytes % multiple:
        raise ProbeError(f"{what}: {nbytes} bytes is not a nonzero multiple of {multiple}")
    if t.data_ptr() % align:
        raise ProbeError(f"{what}: the tensor's storage is not {align}-byte aligned")
    return nbytes


def _stream_of(t, stream):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream(t.device)
    return C.c_void_p(s.cuda_stream)


def count_diff(a, b, stream=None) -> int:
    """Number of 16-byte words in which two device tensors of the same size differ: the
    burn-in's compare kernel (gm_probe_count_diff). Waits for the result."""
    import torch

    na, nb = _dev_bytes(a, "count_diff"), _dev_bytes(b, "count_diff")
    if na != nb or a.device != b.device:
        raise ProbeError(f"count_diff: {na} and {nb} bytes, or different devices")
    n = C.c_uint64(0)
    with torch.cuda.device(a.device):
        _check(_native.probe().gm_probe_count_diff(a.data_ptr(), b.data_ptr(), na,
                                                   _stream_of(a, stream), C.byref(n)),
               "count_diff")
    return n.value


BURN_IN_STATE_BYTES = C.sizeof(_native.BurninState)   # gm_probe_burn_in_state_bytes()


class CompareState(NamedTuple):
    """What :func:`count_diff_tiles` accumulates over its calls, device tensors: ``state`` is
    :data:`BURN_IN_STATE_BYTES` bytes (a ``gm_burnin_state_t``: total, cursor, the log),
    ``exonerated`` and ``moved`` one int32 per tile, ``seen`` one per CU id. Zeroed by whoever
    makes it."""
    state: object
    exonerated: object
    moved: object
    seen: object


def count_diff_tiles(a, b, cu, ref_cu, iteration: int, state: Optional[CompareState] = None,
                     read: bool = True, stream=None):
    """One per-tile compare of the attributed burn-in (gm_probe_count_diff_tiles, the launch the
    burn-in's loop uses) of two n × n bf16 device tensors, ``b`` the reference, n a multiple of
    256; ``cu`` and ``ref_cu`` are the CU maps of the two, int32 tensors with one id per tile
    (-1, i.e. 0xFFFFFFFF: none stored). Without a ``state`` a zeroed one is made; handing back
    the returned one accumulates as the iterations of a run do. Waits for the launch and
    returns ``{"total", "cursor", "events": [(iteration, tile, worker, reference, words), ...]
    in log order, "exonerated", "moved", "seen": lists of 0 / 1, "state"}``; with
    ``read=False`` it only launches (asynchronous) and returns ``{"state"}``."""
    import torch

    for t, what in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16 or t.dim() != 2:
            raise ProbeError(f"count_diff_tiles: {what} must be a 2-D bf16 torch tensor")
        if not t.is_contiguous():
            raise ProbeError(f"count_diff_tiles: {what} must be contiguous")
    n = int(a.shape[0])
    if a.shape != (n, n) or b.shape != (n, n) or n == 0 or n % BURN_IN_TILE:
        raise ProbeError(f"count_diff_tiles: a{tuple(a.shape)} and b{tuple(b.shape)} are not two "
                         f"n × n results with n a positive multiple of {BURN_IN_TILE}")
    tiles = (n // BURN_IN_TILE) ** 2
    if not isinstance(iteration, int) or isinstance(iteration, bool) or \
            not 0 <= iteration < 1 << 32:
        raise ProbeError(f"count_diff_tiles: iteration {iteration!r} is not a 32-bit integer")

    def words(t, what: str, count: int) -> None:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous():
            raise ProbeError(f"count_diff_tiles: {what} must be a contiguous int32 torch tensor")
        if t.numel() != count:
            raise ProbeError(f"count_diff_tiles: {what} has {t.numel()} entries, not {count}")

    words(cu, "cu", tiles)
    words(ref_cu, "ref_cu", tiles)
    if state is None:
        if a.device.type != "cuda":
            raise ProbeError(f"count_diff_tiles expects tensors on a HIP device, got {a.device}")
        state = CompareState(
            torch.zeros(BURN_IN_STATE_BYTES, dtype=torch.uint8, device=a.device),
            *(torch.zeros(k, dtype=torch.int32, device=a.device)
              for k in (tiles, tiles, _native.CUSCAN_IDS)))
    elif not isinstance(state, CompareState):
        raise ProbeError("count_diff_tiles: state must be a CompareState")
    st = state.state
    if not isinstance(st, torch.Tensor) or not st.is_contiguous() or \
            st.numel() * st.element_size() != BURN_IN_STATE_BYTES:
        raise ProbeError(f"count_diff_tiles: the state must be a contiguous tensor of exactly "
                         f"{BURN_IN_STATE_BYTES} bytes")
    words(state.exonerated, "exonerated", tiles)
    words(state.moved, "moved", tiles)
    words(state.seen, "seen", _native.CUSCAN_IDS)
    every = (a, b, cu, ref_cu) + tuple(state)
    if a.device.type != "cuda" or any(t.device != a.device for t in every):
        raise ProbeError(f"count_diff_tiles expects every tensor on one HIP device, got "
                         f"{sorted({str(t.device) for t in every})}")
    if a.data_ptr() % 16 or b.data_ptr() % 16 or st.data_ptr() % 8:
        raise ProbeError("count_diff_tiles: a and b must be 16-byte and the state 8-byte aligned")
    s = stream if stream is not None else torch.cuda.current_stream(a.device)
    with torch.cuda.device(a.device):
        _check(_native.probe().gm_probe_count_diff_tiles(
            a.data_ptr(), b.data_ptr(), n, cu.data_ptr(), ref_cu.data_ptr(), iteration,
            st.data_ptr(), state.exonerated.data_ptr(), state.moved.data_ptr(),
            state.seen.data_ptr(), C.c_void_p(s.cuda_stream)), "count_diff_tiles")
    if not read:
        return {"state": state}
    s.synchronize()
    return {**read_compare_state(state), "state": state}


def read_compare_state(state: CompareState) -> Dict:
    """The host's view of a :class:`CompareState` (copies it back; the caller has waited for
    the compares): total, cursor, the logged events and the three mark arrays."""
    import numpy as np

    raw = state.state.cpu().numpy().view(np.uint8).tobytes()
    st = _native.BurninState.from_buffer_copy(raw)
    events = [(e.iteration, e.tile, e.worker, e.reference, e.words)
              for e in st.log[:min(st.cursor, _native.BURNIN_LOG_CAP)]]
    return {"total": st.total, "cursor": st.cursor, "events": events,
            "exonerated": state.exonerated.cpu().tolist(), "moved": state.moved.cpu().tolist(),
            "seen": state.seen.cpu().tolist()}


def fill_bf16(t, seed: int, stream=None):
    """Fill a bf16 (or int16/uint16) device tensor with the burn-in's operand sequence for
    ``seed`` (gm_probe_fill_bf16; formula in native/include/gm_probe.h). Asynchronous."""
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bfloat16, torch.int16,
                                                          torch.uint16):
        raise ProbeError("fill_bf16 expects a bf16, int16 or uint16 torch tensor")
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 32:
        raise ProbeError("fill_bf16: seed must be an integer in [0, 2^32)")
    _dev_bytes(t, "fill_bf16", align=2, multiple=2)
    with torch.cuda.device(t.device):
        _check(_native.probe().gm_probe_fill_bf16(t.data_ptr(), t.numel(), seed,
                                                  _stream_of(t, stream)), "fill_bf16")
    return t


def copy(variant: int, src, dst, blocks_per_cu: int = 8, stream=None):
    """One launch of HBM copy variant ``variant`` (0..6, see gm_probe.h) from ``src`` to ``dst``,
    device tensors of the same size in bytes (gm_probe_copy). Asynchronous."""
    import torch

    ns, nd = _dev_bytes(src, "copy"), _dev_bytes(dst, "copy")
    if ns != nd or src.device != dst.device:
        raise ProbeError(f"copy: {ns} and {nd} bytes, or different devices")
    with torch.cuda.device(src.device):
        _check(_native.probe().gm_probe_copy(variant, src.data_ptr(), dst.data_ptr(), ns,
                                             blocks_per_cu, _stream_of(src, stream)), "copy")
    return dst


READ_SINK_WORDS = 1024
READ_MAGIC = 0x9E3779B9       # a thread stores only if the XOR of the words it read is this


def read(src, sink, blocks_per_cu: int = 2, stream=None):
    """One launch of the HBM read stream over ``src`` (gm_probe_read). ``sink`` is a device
    tensor of 1024 int32/uint32: a thread of block ``b`` writes ``sink[b & 1023] = READ_MAGIC``
    only if the XOR of the 32-bit words it read (elements 256 apart in the block's chunk) equals
    READ_MAGIC. Asynchronous."""
    import torch

    ns = _dev_bytes(src, "read")
    if not isinstance(sink, torch.Tensor) or sink.dtype not in (torch.int32, torch.uint32) \
            or sink.numel() != READ_SINK_WORDS or sink.device != src.device:
        raise ProbeError(f"read: sink must be {READ_SINK_WORDS} int32 on the source's device")
    _dev_bytes(sink, "read", align=4, multiple=4)
    with torch.cuda.device(src.device):
        _check(_native.probe().gm_probe_read(src.data_ptr(), sink.data_ptr(), ns, blocks_per_cu,
                                             _stream_of(src, stream)), "read")
    return sink


def p2p(dev_a: int, dev_b: int, nbytes: int = 256 << 20, iters: int = 10) -> Dict:
    can, g = C.c_int(0), C.c_double(0)
    _check(_native.probe().gm_probe_p2p(dev_a, dev_b, nbytes, iters, C.byref(can), C.byref(g)),
           "p2p")
    return {"src": dev_a, "dst": dev_b, "peer_access": bool(can.value), "gbps": g.value}


@dataclass
class VerifyResult:
    device: int
    bdf: str
    quick_us: float
    gcn_arch: str
    hbm_gbps: Optional[float] = None
    hbm_read_gbps: Optional[float] = None
    mfma_tflops: Optional[float] = None
    gemm_max_abs_err: Optional[float] = None
    gemm_tflops: Optional[float] = None

    def to_dict(self) -> Dict:
        return asdict(self)


def verify(bdfs: List[str], full: bool = False) -> List[VerifyResult]:
    """Run the validation on each attached GPU (by PCI address)."""
    out = []
    for bdf in bdfs:
        dev = find_device(bdf)
        if dev < 0:
            raise ProbeError(f"attached GPU {bdf} is not visible to HIP in this process")
        pr = props(dev)
        r = VerifyResult(dev, bdf, quick(dev), pr["gcn_arch"])
        if full:
            r.hbm_gbps = hbm_gbps(dev)
            r.hbm_read_gbps = hbm_read_gbps(dev)
            r.mfma_tflops = mfma_tflops(dev)
            r.gemm_max_abs_err = gemm_check(dev)["max_abs_err"]
            r.gemm_tflops = gemm_tflops(dev, 4096, 4096, 4096, 10)
        out.append(r)
    return out
