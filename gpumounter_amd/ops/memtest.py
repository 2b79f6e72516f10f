"""HBM pattern test of an attached GPU (native/hip/gm_memtest.hip): does the VRAM hold what is
written to it?

The other probes prove that a hot-mounted GPU executes kernels; this one fills most of its free
memory with patterns and reads them back. For every selected pattern and pass the region is
filled with ``P``, read and checked while ``~P`` is written over it, and read and checked again,
so every cell holds both polarities and is read once after each write. The expected value of a
word is a pure function of its byte offset in the region (formulas: native/include/gm_probe.h),
shared by the host and the kernels; :func:`expected` evaluates it without a GPU.

What it cannot tell: offsets are virtual offsets inside the test's own allocations, not physical
HBM addresses; memory that is in use when the test runs is not covered; and below 1 GiB the
256 MiB Infinity Cache and the L2s can serve most of the reads (``hbm_exercised`` is false then).
No silent fallback: a missing ``libgm_probe.so`` or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Sequence, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops.probe import ProbeError, _check

PATTERNS = {"addr": 1, "solid": 2, "checker": 4, "walk": 8, "random": 16}
PATTERN_NAMES = {v: k for k, v in PATTERNS.items()}
ALL_PATTERNS = tuple(PATTERNS)
DEFAULT_SEED = 0x243F6A8885A308D3
MIN_HBM_BYTES = 1 << 30       # below this the caches can serve most reads
_U64 = (1 << 64) - 1


def pattern_bit(pattern) -> int:
    """The bit of one pattern, given by name or by bit."""
    if isinstance(pattern, str) and pattern in PATTERNS:
        return PATTERNS[pattern]
    if isinstance(pattern, int) and not isinstance(pattern, bool) and pattern in PATTERN_NAMES:
        return pattern
    raise ProbeError(f"unknown memtest pattern {pattern!r} (one of {', '.join(PATTERNS)})")


def pattern_mask(patterns: Iterable) -> int:
    if isinstance(patterns, (str, int)):
        patterns = (patterns,)
    mask = 0
    for p in patterns:
        mask |= pattern_bit(p)
    if not mask:
        raise ProbeError("memtest needs at least one pattern")
    return mask


def _u64(v, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= _U64:
        raise ProbeError(f"memtest: {what} must be an integer in [0, 2^64)")
    return v


def _u32(v, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << 32:
        raise ProbeError(f"memtest: {what} must be an integer in [0, 2^32)")
    return v


def expected(pattern, seed: int, pass_: int, base_offset: int, n_words: int):
    """numpy uint64 array: the expected words of ``n_words`` consecutive 64-bit words starting
    at global byte offset ``base_offset`` (a multiple of 8). Host only, no GPU."""
    import numpy as np

    bit = pattern_bit(pattern)
    _u64(seed, "seed"), _u32(pass_, "pass"), _u64(base_offset, "base_offset")
    if base_offset % 8 or not isinstance(n_words, int) or n_words < 0:
        raise ProbeError("memtest.expected: base_offset must be a multiple of 8, n_words >= 0")
    out = np.empty(n_words, dtype=np.uint64)
    _check(_native.probe().gm_probe_memtest_expected(
        bit, seed, pass_, base_offset, n_words, out.ctypes.data_as(C.POINTER(C.c_uint64))),
        "memtest expected")
    return out


def plan_bytes(free_bytes: int, total_bytes: int, fraction: float = 0.9) -> int:
    """Default size of a test: ``fraction`` of the memory that is *free* now, rounded down to
    16 bytes. Memory other processes hold is theirs and is not tested."""
    if not 0 < fraction <= 1:
        raise ProbeError(f"memtest: fraction {fraction} not in (0, 1]")
    if free_bytes < 0 or total_bytes < free_bytes:
        raise ProbeError(f"memtest: free {free_bytes} / total {total_bytes} bytes make no sense")
    n = int(free_bytes * fraction) // 16 * 16
    if n < 16:
        raise ProbeError(f"memtest: only {free_bytes} bytes free, nothing to test")
    return n


def parse_size(text) -> int:
    """``"64M"``, ``"8G"``, ``"123456"`` → bytes (K, M, G, T are powers of 1024)."""
    s = str(text).strip()
    mult = 1
    units = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30, "T": 1 << 40}
    if s and s[-1].upper() in units:
        mult = units[s[-1].upper()]
        s = s[:-1]
    if not (s.isascii() and s.isdigit()):
        raise ProbeError(f"memtest: cannot read {text!r} as a size (digits, then K, M, G or T)")
    return int(s) * mult


def parse_flip(text) -> Tuple[int, int]:
    """``"OFFSET:MASK"`` (any Python integer literal, e.g. ``4096:0x10``) → (offset, mask)."""
    try:
        off, mask = str(text).split(":")
        return _u64(int(off, 0), "flip offset"), _u64(int(mask, 0), "flip mask")
    except ValueError:
        raise ProbeError(f"memtest: cannot read {text!r} as OFFSET:MASK") from None


def parse_patterns(text) -> Tuple[str, ...]:
    """``"addr,random"`` → ("addr", "random"); every name is checked."""
    names = tuple(t.strip() for t in str(text).split(",") if t.strip())
    pattern_mask(names)
    return names


def mem_info(dev: int) -> Dict[str, int]:
    f, t = C.c_uint64(0), C.c_uint64(0)
    _check(_native.probe().gm_probe_mem_info(dev, C.byref(f), C.byref(t)), "mem info")
    return {"free": f.value, "total": t.value}


def _buffer(t, what: str) -> int:
    """Checks a tensor the kernels may walk; returns its size in bytes."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ProbeError(f"{what} expects a torch tensor")
    if t.dtype not in (torch.uint8, torch.int64, torch.uint64):
        raise ProbeError(f"{what} expects a uint8, int64 or uint64 tensor, got {t.dtype}")
    if t.device.type != "cuda":
        raise ProbeError(f"{what} expects a tensor on a HIP device, got {t.device}")
    if not t.is_contiguous():
        raise ProbeError(f"{what} expects a contiguous tensor")
    nbytes = t.numel() * t.element_size()
    if nbytes == 0 or nbytes % 16:
        raise ProbeError(f"{what}: {nbytes} bytes is not a nonzero multiple of 16")
    if t.data_ptr() % 16:
        raise ProbeError(f"{what}: the tensor's storage is not 16-byte aligned")
    return nbytes


def _common(pattern, seed, pass_, base_offset) -> int:
    bit = pattern_bit(pattern)
    _u64(seed, "seed"), _u32(pass_, "pass"), _u64(base_offset, "base_offset")
    if base_offset % 8:
        raise ProbeError("memtest: base_offset must be a multiple of 8")
    return bit


def fill(tensor, pattern, invert: bool = False, seed: int = DEFAULT_SEED, pass_: int = 0,
         base_offset: int = 0, stream=None):
    """Fill a caller-owned device tensor with pattern ``P`` (``~P`` with ``invert``), as if its
    first byte were at ``base_offset`` of a test region. Asynchronous on the stream."""
    import torch

    bit = _common(pattern, seed, pass_, base_offset)
    nbytes = _buffer(tensor, "memtest.fill")
    s = stream if stream is not None else torch.cuda.current_stream(tensor.device)
    with torch.cuda.device(tensor.device):
        _check(_native.probe().gm_probe_memtest_fill(
            tensor.data_ptr(), nbytes, bit, int(bool(invert)), seed, pass_, base_offset,
            C.c_void_p(s.cuda_stream)), "memtest fill")
    return tensor


def _errors(r: _native.MemtestResult) -> Dict:
    recs = []
    for i in range(r.records_filled):
        x = r.records[i]
        recs.append({"offset": x.offset, "expected": f"{x.expected:#018x}",
                     "got": f"{x.got:#018x}", "xor": f"{x.expected ^ x.got:#018x}",
                     "pattern": PATTERN_NAMES.get(x.pattern, str(x.pattern)),
                     "pass": x.pass_})
    return {"errors": r.words_in_error, "bit_errors": r.bit_errors,
            "stuck_mask": f"{r.stuck_mask:#018x}", "first_errors": recs,
            "ok": r.words_in_error == 0}


def verify(tensor, pattern, invert: bool = False, write_inverse: bool = False,
           seed: int = DEFAULT_SEED, pass_: int = 0, base_offset: int = 0, stream=None) -> Dict:
    """Check a caller-owned device tensor against ``P`` (``~P`` with ``invert``). With
    ``write_inverse`` the same kernel writes the opposite polarity over every word it read.
    Returns ``errors`` (words), ``bit_errors``, ``stuck_mask``, ``first_errors`` (at most 16)."""
    import torch

    bit = _common(pattern, seed, pass_, base_offset)
    nbytes = _buffer(tensor, "memtest.verify")
    s = stream if stream is not None else torch.cuda.current_stream(tensor.device)
    res = _native.MemtestResult()
    with torch.cuda.device(tensor.device):
        _check(_native.probe().gm_probe_memtest_verify(
            tensor.data_ptr(), nbytes, bit, int(bool(invert)), int(bool(write_inverse)), seed,
            pass_, base_offset, C.c_void_p(s.cuda_stream), C.byref(res)), "memtest verify")
    out = _errors(res)
    out["bytes"] = res.bytes_tested
    return out


def memtest(dev: int, nbytes: Optional[int] = None, patterns: Sequence = ALL_PATTERNS,
            passes: int = 1, seed: int = DEFAULT_SEED, chunk_bytes: int = 0,
            _flip: Optional[Tuple[int, int]] = None) -> Dict:
    """The whole test on device ``dev``: ``nbytes`` (default :func:`plan_bytes` of the free
    memory) in allocations of at most ``chunk_bytes`` (0: 8 GiB). ``_flip=(offset, mask)`` is the
    negative control: the word at that global offset is corrupted after every fill, so the test
    must report it."""
    mask = pattern_mask(patterns)
    names = [n for n in PATTERNS if PATTERNS[n] & mask]
    if not isinstance(passes, int) or isinstance(passes, bool) or not 1 <= passes < 1 << 31:
        raise ProbeError(f"memtest: passes must be a positive integer, got {passes!r}")
    _u64(seed, "seed"), _u64(chunk_bytes, "chunk_bytes")
    if chunk_bytes % 16:
        raise ProbeError("memtest: chunk_bytes must be a multiple of 16")
    if nbytes is not None:
        _u64(nbytes, "nbytes")
        if nbytes == 0 or nbytes % 16:
            raise ProbeError(f"memtest: {nbytes} bytes is not a nonzero multiple of 16")
    flip_off = flip_mask = 0
    if _flip is not None:
        flip_off, flip_mask = _u64(_flip[0], "flip offset"), _u64(_flip[1], "flip mask")
        if flip_off % 8:
            raise ProbeError("memtest: the flip offset must be a multiple of 8")
    if nbytes is None:
        mi = mem_info(dev)
        nbytes = plan_bytes(mi["free"], mi["total"])
    if flip_mask and flip_off + 8 > nbytes:
        raise ProbeError(f"memtest: flip offset {flip_off} is outside the {nbytes} bytes tested")
    res = _native.MemtestResult()
    _check(_native.probe().gm_probe_memtest(dev, nbytes, chunk_bytes, mask, passes, seed,
                                            flip_off, flip_mask, C.byref(res)), "memtest")
    out = {"device": dev, "bytes": res.bytes_tested, "requested_bytes": nbytes,
           "allocations": res.allocations, "patterns": names, "passes": passes,
           "seconds": res.seconds, "write_gbps": res.write_gbps, "read_gbps": res.read_gbps,
           "rw_gbps": res.rw_gbps}
    out.update(_errors(res))
    out["hbm_exercised"] = res.bytes_tested >= MIN_HBM_BYTES
    return out
