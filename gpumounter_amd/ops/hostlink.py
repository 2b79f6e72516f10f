"""Host-link (PCIe) data and bandwidth test of an attached GPU (native/hip/gm_hostlink.hip): do
bytes arrive intact between pinned host memory and the GPU, and how fast?

The other probes stay inside the package or go to a peer GPU. This one pins host memory, which a
container may be refused, and moves checked bytes across the host link in six ways ("legs"): the
copy engines in each direction and in both at once, and kernels that read, write and copy pinned
host memory through its device mapping. Every expected value is the memtest pattern function
(:func:`gpumounter_amd.ops.memtest.expected`); before a leg its destination holds something that
fails the leg's check. The rates are measurements, never a verdict: ``ok`` says only whether a
wrong word was seen.

The link's trained speed and width are read from sysfs *while the transfers run* (AMD GPUs lower
the link speed at rest); ``link["degraded"]`` says that either stayed below its maximum, and a
leg's ``rate_above_link`` that its GB/s exceeds what that link can carry (GT/s x width x 128/130
/ 8), so not all of its bytes crossed the link. Neither changes ``ok``.

What it cannot tell: pageable copies, NUMA placement (the node is only reported), and which part
of the path (host DRAM, root complex, switch, HBM) damaged a word.
No silent fallback: a missing ``libgm_probe.so``, a refused pin or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Callable, Dict, Iterable, Optional, Sequence, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops import memtest
from gpumounter_amd.ops.probe import ProbeError, _check

LEGS = {"h2d": 1, "d2h": 2, "bidir": 4, "kread": 8, "kwrite": 16, "kduplex": 32}
LEG_NAMES = {v: k for k, v in LEGS.items()}
ALL_LEGS = tuple(LEGS)
TWO_WAY_LEGS = ("bidir", "kduplex")      # their bytes and GB/s count both directions
DEFAULT_BYTES = 256 << 20
DEFAULT_PATTERNS = ("addr", "random")
DEFAULT_SEED = memtest.DEFAULT_SEED
STEP_BYTES = 8 * 256 * 16     # the kernels' bytes per block per step (gm_probe_hostlink_geometry)
DEFAULT_BLOCKS = 16           # the driver's grid for blocks = 0 (gm_probe_hostlink_geometry)
MAX_BLOCKS = _native.HOSTLINK_MAX_BLOCKS
MAX_ITERS = 1024
LINK_FILES = ("current_link_speed", "max_link_speed", "current_link_width", "max_link_width",
              "numa_node")
SAMPLE_INTERVAL_S = 0.005


class HostlinkError(ProbeError):
    """A HIP failure of the driver; ``stage`` names what failed ("pin", "alloc", a leg, ...)."""

    def __init__(self, msg: str, stage: str, code: int):
        super().__init__(msg)
        self.stage = stage
        self.code = code


# ------------------------------------------------------------------------------------- parsers
def leg_bit(leg) -> int:
    """The bit of one leg, given by name or by bit."""
    if isinstance(leg, str) and leg in LEGS:
        return LEGS[leg]
    if isinstance(leg, int) and not isinstance(leg, bool) and leg in LEG_NAMES:
        return leg
    raise ProbeError(f"unknown host-link leg {leg!r} (one of {', '.join(LEGS)})")


def legs_mask(legs: Iterable) -> int:
    if isinstance(legs, (str, int)):
        legs = (legs,)
    mask = 0
    for leg in legs:
        mask |= leg_bit(leg)
    if not mask:
        raise ProbeError("host-link needs at least one leg")
    return mask


def parse_legs(text) -> Tuple[str, ...]:
    """``"h2d,kread"`` → ("h2d", "kread"); every name is checked."""
    names = tuple(t.strip() for t in str(text).split(",") if t.strip())
    legs_mask(names)
    return names


def parse_patterns(text) -> Tuple[str, ...]:
    return memtest.parse_patterns(text)


def parse_size(text) -> int:
    return memtest.parse_size(text)


def parse_blocks(text) -> int:
    try:
        return _int(int(str(text), 0), 1, MAX_BLOCKS, "blocks")
    except ValueError:
        raise ProbeError(f"host-link: cannot read {text!r} as a number of blocks") from None


def parse_flip(text) -> Tuple[str, int, int]:
    """``"LEG:OFFSET:MASK"`` (integers as Python literals, e.g. ``kread:4096:0x10``) →
    (leg name, offset, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    if len(parts) != 3:
        raise ProbeError(f"host-link: cannot read {text!r} as LEG:OFFSET:MASK")
    leg = LEG_NAMES[leg_bit(parts[0])]
    try:
        off, mask = int(parts[1], 0), int(parts[2], 0)
    except ValueError:
        raise ProbeError(f"host-link: cannot read {text!r} as LEG:OFFSET:MASK") from None
    return _flip_arg((leg, off, mask))


def _int(v, lo: int, hi: int, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ProbeError(f"host-link: {what} must be an integer in [{lo}, {hi}], got {v!r}")
    return v


def _flip_arg(flip) -> Tuple[str, int, int]:
    try:
        leg, off, mask = flip
    except (TypeError, ValueError):
        raise ProbeError(f"host-link: flip {flip!r} is not (leg, offset, mask)") from None
    leg = LEG_NAMES[leg_bit(leg)]
    _int(off, 0, (1 << 64) - 1, "flip offset")
    _int(mask, 1, (1 << 64) - 1, "flip mask")
    if off % 8:
        raise ProbeError("host-link: the flip offset must be a multiple of 8")
    return leg, off, mask


# ------------------------------------------------------------------------------ the link itself
def _read_link_file(path: str) -> Optional[str]:
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return None
    try:
        return os.read(fd, 128).decode("ascii", errors="replace").strip()
    except OSError:
        return None
    finally:
        os.close(fd)


def _speed_gts(text: Optional[str]) -> Optional[float]:
    """``"32.0 GT/s PCIe"`` → 32.0; anything that does not read so → None."""
    if not text:
        return None
    parts = text.split()
    if len(parts) < 2 or parts[1] != "GT/s":
        return None
    try:
        v = float(parts[0])
    except ValueError:
        return None
    return v if 0 < v < 1e4 else None


def _small_int(text: Optional[str], lo: int, hi: int) -> Optional[int]:
    try:
        v = int(text) if text is not None else None
    except ValueError:
        return None
    return v if v is not None and lo <= v <= hi else None


def link_state(bdf: str, sysfs: str = "/sys") -> Dict:
    """What ``bus/pci/devices/<bdf>`` under ``sysfs`` says about the device's link now. The files
    are opened read-only; a missing, unreadable or unparsable file gives ``None`` for its field,
    never an error."""
    base = os.path.join(sysfs, "bus", "pci", "devices", str(bdf).lower())
    raw = {n: _read_link_file(os.path.join(base, n)) for n in LINK_FILES}
    return {"bdf": str(bdf).lower(),
            "speed_gts": _speed_gts(raw["current_link_speed"]),
            "max_speed_gts": _speed_gts(raw["max_link_speed"]),
            "width": _small_int(raw["current_link_width"], 1, 64),
            "max_width": _small_int(raw["max_link_width"], 1, 64),
            "numa_node": _small_int(raw["numa_node"], -1, 1 << 16)}


def link_gbps(speed_gts: Optional[float], width: Optional[int]) -> Optional[float]:
    """GB/s one direction of a link can carry: GT/s x width x 128/130 / 8. A derived bound (the
    line code alone; packet headers take more), not a measured threshold."""
    if not speed_gts or not width:
        return None
    return speed_gts * width * 128.0 / 130.0 / 8.0


def _max_seen(a, b):
    return b if a is None else a if b is None else max(a, b)


class LinkSampler:
    """Reads :func:`link_state` from a helper thread until stopped and keeps the highest speed and
    width seen. One sample is taken before the thread starts (``rest``) and one when it is asked
    to stop."""

    def __init__(self, bdf: str, sysfs: str = "/sys", interval: float = SAMPLE_INTERVAL_S):
        self.bdf, self.sysfs, self.interval = bdf, sysfs, interval
        self.rest = link_state(bdf, sysfs)
        self.speed_gts = self.width = None
        self.last = self.rest
        self.samples = 0
        self.sampled = threading.Condition()
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, name="gm-link-sampler", daemon=True)

    def _sample(self) -> None:
        st = link_state(self.bdf, self.sysfs)
        with self.sampled:
            self.last = st
            self.speed_gts = _max_seen(self.speed_gts, st["speed_gts"])
            self.width = _max_seen(self.width, st["width"])
            self.samples += 1
            self.sampled.notify_all()

    def _run(self) -> None:
        while not self._stop.wait(self.interval):
            self._sample()
        self._sample()

    def wait_for_sample(self, timeout: float = 5.0) -> bool:
        """Blocks until one more sample has been taken (for tests that change the files)."""
        with self.sampled:
            n = self.samples
            return self.sampled.wait_for(lambda: self.samples > n, timeout)

    def __enter__(self):
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()

    def report(self) -> Dict:
        last = self.last
        max_speed = _max_seen(self.rest["max_speed_gts"], last["max_speed_gts"])
        max_width = _max_seen(self.rest["max_width"], last["max_width"])
        out = {"bdf": self.bdf, "rest": {"speed_gts": self.rest["speed_gts"],
                                         "width": self.rest["width"]},
               "speed_gts": self.speed_gts, "width": self.width,
               "max_speed_gts": max_speed, "max_width": max_width,
               "numa_node": _max_seen(self.rest["numa_node"], last["numa_node"]),
               "samples": self.samples}
        out["readable"] = self.speed_gts is not None and self.width is not None
        out["degraded"] = degraded(out)
        out["gbps_per_direction"] = link_gbps(self.speed_gts, self.width)
        return out


def degraded(link: Dict) -> bool:
    """True when the speed or the width seen under load stayed below its maximum. A field that
    could not be read decides nothing."""
    for got, top in (("speed_gts", "max_speed_gts"), ("width", "max_width")):
        if link.get(got) is not None and link.get(top) is not None and link[got] < link[top]:
            return True
    return False


def describe_link(link: Dict) -> str:
    """``"x8 of x16, 16.0 of 32.0 GT/s"``"""
    def f(v, fmt):
        return "?" if v is None else format(v, fmt)
    return (f"x{f(link.get('width'), 'd')} of x{f(link.get('max_width'), 'd')}, "
            f"{f(link.get('speed_gts'), '.1f')} of {f(link.get('max_speed_gts'), '.1f')} GT/s")


def sample_link_during(fn: Callable, bdf: Optional[str], sysfs: str = "/sys",
                       interval: float = SAMPLE_INTERVAL_S):
    """Runs ``fn(sampler)`` on this thread while a helper thread samples the link of ``bdf``;
    returns (what fn returned, the link report). Without a ``bdf`` nothing is sampled."""
    if not bdf:
        return fn(None), {"bdf": None, "rest": {"speed_gts": None, "width": None},
                          "speed_gts": None, "width": None, "max_speed_gts": None,
                          "max_width": None, "numa_node": None, "samples": 0,
                          "readable": False, "degraded": False, "gbps_per_direction": None}
    sampler = LinkSampler(bdf, sysfs, interval)
    with sampler:
        result = fn(sampler)
    return result, sampler.report()


def rate_above_link(gbps: float, link: Dict, directions: int = 1) -> bool:
    """True when ``gbps`` exceeds what ``directions`` directions of the sampled link can carry."""
    cap = link_gbps(link.get("speed_gts"), link.get("width"))
    return cap is not None and gbps > cap * directions


# --------------------------------------------------------------------------- caller-owned memory
def geometry() -> Dict[str, int]:
    """``step_bytes`` and ``default_blocks`` as the loaded library has them."""
    step, blocks = C.c_uint32(0), C.c_uint32(0)
    _check(_native.probe().gm_probe_hostlink_geometry(C.byref(step), C.byref(blocks)),
           "host-link geometry")
    return {"step_bytes": step.value, "default_blocks": blocks.value}


def _pinned(t, what: str) -> int:
    """Checks a tensor the kernels may walk over the link; returns its size in bytes."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ProbeError(f"{what} expects a torch tensor")
    if not t.is_pinned():
        raise ProbeError(f"{what} expects a tensor in pinned host memory "
                         f"(tensor.pin_memory()), got one on {t.device} that is not")
    if t.dtype not in (torch.uint8, torch.int64, torch.uint64):
        raise ProbeError(f"{what} expects a uint8, int64 or uint64 tensor, got {t.dtype}")
    if not t.is_contiguous():
        raise ProbeError(f"{what} expects a contiguous tensor")
    nbytes = t.numel() * t.element_size()
    if nbytes == 0 or nbytes % 16:
        raise ProbeError(f"{what}: {nbytes} bytes is not a nonzero multiple of 16")
    if t.data_ptr() % 16:
        raise ProbeError(f"{what}: the tensor's storage is not 16-byte aligned")
    return nbytes


def _blocks(blocks) -> int:
    return DEFAULT_BLOCKS if blocks is None else _int(blocks, 1, MAX_BLOCKS, "blocks")


def _launch_ctx(device, stream):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None \
        else torch.device(device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    return dev, C.c_void_p(s.cuda_stream)


def _kflip(flip) -> Tuple[int, int]:
    if flip is None:
        return 0, 0
    try:
        off, mask = flip
    except (TypeError, ValueError):
        raise ProbeError(f"host-link: flip {flip!r} is not (offset, mask)") from None
    _int(off, 0, (1 << 64) - 1, "flip offset"), _int(mask, 0, (1 << 64) - 1, "flip mask")
    if off % 8:
        raise ProbeError("host-link: the flip offset must be a multiple of 8")
    return off, mask


def kwrite(tensor, pattern, invert: bool = False, seed: int = DEFAULT_SEED, pass_: int = 0,
           base_offset: int = 0, blocks: Optional[int] = None, flip=None, device=None,
           stream=None):
    """One kernel on ``device`` (default: the current one) writes pattern ``P`` (``~P`` with
    ``invert``) into a pinned host tensor, as if its first byte were at ``base_offset`` of a test
    region. ``flip=(offset, mask)`` XORs the word written at that global offset. Asynchronous on
    the stream."""
    import torch

    nbytes = _pinned(tensor, "hostlink.kwrite")
    bit = memtest._common(pattern, seed, pass_, base_offset)
    off, mask = _kflip(flip)
    dev, s = _launch_ctx(device, stream)
    with torch.cuda.device(dev):
        _check(_native.probe().gm_probe_hostlink_kwrite(
            tensor.data_ptr(), nbytes, bit, int(bool(invert)), seed, pass_, base_offset,
            _blocks(blocks), off, mask, s), "host-link kwrite")
    return tensor


def kread(tensor, pattern, invert: bool = False, seed: int = DEFAULT_SEED, pass_: int = 0,
          base_offset: int = 0, blocks: Optional[int] = None, device=None, stream=None) -> Dict:
    """One kernel reads a pinned host tensor over the link and checks every word against ``P``.
    Returns ``errors`` (words), ``bit_errors``, ``stuck_mask``, ``first_errors`` (at most 16)."""
    import torch

    nbytes = _pinned(tensor, "hostlink.kread")
    bit = memtest._common(pattern, seed, pass_, base_offset)
    dev, s = _launch_ctx(device, stream)
    res = _native.MemtestResult()
    with torch.cuda.device(dev):
        _check(_native.probe().gm_probe_hostlink_kread(
            tensor.data_ptr(), nbytes, bit, int(bool(invert)), seed, pass_, base_offset,
            _blocks(blocks), s, C.byref(res)), "host-link kread")
    out = memtest._errors(res)
    out["bytes"] = res.bytes_tested
    return out


def kcopy(src, dst, pattern, invert: bool = False, seed: int = DEFAULT_SEED, pass_: int = 0,
          base_offset: int = 0, blocks: Optional[int] = None, flip=None, device=None,
          stream=None) -> Dict:
    """One kernel reads pinned ``src``, checks it against ``P`` and writes what it read to pinned
    ``dst`` (same size, disjoint). ``flip`` changes one written word, not the check. Returns what
    :func:`kread` returns, for the source."""
    import torch

    nbytes = _pinned(src, "hostlink.kcopy")
    if _pinned(dst, "hostlink.kcopy") != nbytes:
        raise ProbeError("hostlink.kcopy: src and dst differ in size")
    a, b = src.data_ptr(), dst.data_ptr()
    if a < b + nbytes and b < a + nbytes:
        raise ProbeError("hostlink.kcopy: src and dst overlap")
    bit = memtest._common(pattern, seed, pass_, base_offset)
    off, mask = _kflip(flip)
    dev, s = _launch_ctx(device, stream)
    res = _native.MemtestResult()
    with torch.cuda.device(dev):
        _check(_native.probe().gm_probe_hostlink_kcopy(
            a, b, nbytes, bit, int(bool(invert)), seed, pass_, base_offset, _blocks(blocks), off,
            mask, s, C.byref(res)), "host-link kcopy")
    out = memtest._errors(res)
    out["bytes"] = res.bytes_tested
    return out


# ------------------------------------------------------------------------------------ the driver
def _leg_entry(leg: _native.HostlinkLeg, link: Dict, directions: int) -> Dict:
    return {"bytes": leg.bytes, "ms": leg.ms, "gbps": leg.gbps, "errors": leg.words_in_error,
            "rate_above_link": rate_above_link(leg.gbps, link, directions)}


def _report(res: _native.HostlinkResult, names: Sequence[str], link: Dict) -> Dict:
    legs = {}
    for i, name in enumerate(LEGS):
        if name not in names:
            continue
        legs[name] = _leg_entry(res.legs[i], link, 2 if name in TWO_WAY_LEGS else 1)
        if name == "bidir":
            legs[name]["h2d"] = _leg_entry(res.bidir_h2d, link, 1)
            legs[name]["d2h"] = _leg_entry(res.bidir_d2h, link, 1)
    recs = []
    for i in range(res.records_filled):
        x = res.records[i]
        recs.append({"leg": LEG_NAMES.get(x.leg, str(x.leg)),
                     "pattern": memtest.PATTERN_NAMES.get(x.pattern, str(x.pattern)),
                     "pass": x.pass_, "offset": x.offset, "expected": f"{x.expected:#018x}",
                     "got": f"{x.got:#018x}", "xor": f"{x.expected ^ x.got:#018x}"})
    return {"bytes": res.bytes, "pinned_bytes": res.pinned_bytes, "legs": legs,
            "errors": res.words_in_error, "bit_errors": res.bit_errors,
            "stuck_mask": f"{res.stuck_mask:#018x}", "first_errors": recs,
            "ok": res.words_in_error == 0, "seconds": res.seconds,
            "host_seconds": res.host_seconds, "transfer_seconds": res.transfer_seconds,
            "setup_seconds": res.setup_seconds, "link": link}


def _raise_stage(rc: int, stage: str, nbytes: int) -> None:
    msg = _native.probe().gm_probe_strerror(rc).decode(errors="replace")
    if stage == "pin":
        text = (f"host-link: pinning {nbytes} bytes of host memory was refused: hip error {rc} "
                f"({msg}); check the container's memlock limit (ulimit -l) and IOMMU mapping")
    else:
        text = f"host-link {stage or 'call'}: hip error {rc} ({msg})"
    raise HostlinkError(text, stage, rc)


def hostlink(dev: int, nbytes: Optional[int] = None, legs: Sequence = ALL_LEGS,
             patterns: Sequence = DEFAULT_PATTERNS, passes: int = 1, iters: int = 4,
             blocks: Optional[int] = None, seed: int = DEFAULT_SEED,
             _flip: Optional[Tuple] = None, _sysfs: str = "/sys",
             _bdf: Optional[str] = None) -> Dict:
    """The whole test on device ``dev``: two pinned host buffers and two device buffers of
    ``nbytes`` (default 256 MiB), every leg of ``legs`` for every pattern and pass, each transfer
    timed over ``iters`` repeats after a warm-up. ``_flip=(leg, offset, mask)`` is the negative
    control: one word of that leg's data arrives wrong, so the leg must report it. The link of the
    device is sampled from sysfs while the native call runs."""
    lmask = legs_mask(legs)
    names = [n for n in LEGS if LEGS[n] & lmask]
    pmask = memtest.pattern_mask(patterns)
    pnames = [n for n in memtest.PATTERNS if memtest.PATTERNS[n] & pmask]
    _int(dev, 0, 1 << 16, "device")
    _int(passes, 1, (1 << 31) - 1, "passes")
    _int(iters, 1, MAX_ITERS, "iters")
    _int(seed, 0, (1 << 64) - 1, "seed")
    nb = 0 if blocks is None else _int(blocks, 1, MAX_BLOCKS, "blocks")
    nbytes = DEFAULT_BYTES if nbytes is None else _int(nbytes, 16, 1 << 62, "nbytes")
    if nbytes % 16:
        raise ProbeError(f"host-link: {nbytes} bytes is not a nonzero multiple of 16")
    flip_leg = flip_off = flip_mask = 0
    if _flip is not None:
        leg, flip_off, flip_mask = _flip_arg(_flip)
        flip_leg = LEGS[leg]
        if not flip_leg & lmask:
            raise ProbeError(f"host-link: flip into {leg!r}, which is not run")
        if flip_off + 8 > nbytes:
            raise ProbeError(f"host-link: flip offset {flip_off} is outside the {nbytes} bytes")
    lib = _native.probe()
    if _bdf is None:
        from gpumounter_amd.ops import probe
        _bdf = probe.props(dev)["pci_bus_id"]
    res = _native.HostlinkResult()

    def call(_sampler):
        return lib.gm_probe_hostlink(dev, nbytes, lmask, pmask, passes, iters, nb, seed,
                                     flip_leg, flip_off, flip_mask, C.byref(res))

    rc, link = sample_link_during(call, _bdf, _sysfs)
    if rc != 0:
        _raise_stage(rc, res.stage.decode(errors="replace"), nbytes)
    out = {"device": dev, "requested_bytes": nbytes, "patterns": pnames, "passes": passes,
           "iters": iters, "blocks": nb or DEFAULT_BLOCKS}
    out.update(_report(res, names, link))
    return out


def describe_errors(report: Dict) -> str:
    """One line for a report with wrong words: the legs and the first offset of each."""
    parts = []
    for name, leg in report["legs"].items():
        if not leg["errors"]:
            continue
        first = next((r for r in report["first_errors"] if r["leg"] == name), None)
        at = f" first at offset {first['offset']} xor {first['xor']}" if first else ""
        parts.append(f"{name}: {leg['errors']} wrong word(s){at}")
    return "; ".join(parts)
