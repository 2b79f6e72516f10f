"""What the per-CU scans share above their kernels (the device side of the frame is
native/hip/gm_cuscan_frame.h): one 256-thread block per CU, the CU id read from the hardware
registers, 4 signature words per thread and test compared bit for bit with a table computed on the
host, and one result shape.

A scan is a :class:`Scan` descriptor in its own module (``SCAN`` in :mod:`.cuscan`,
:mod:`.mfmascan`, :mod:`.lanescan`, :mod:`.cachescan`, :mod:`.ldsscan`, :mod:`.sparsescan`), next to its
tables and the functions only it has. The descriptor's methods are everything the scans do alike: the name and bit lookups, the
parsers, the argument checks, ``expected``, ``signature`` and ``scan``. The command line, ``doctor``
and ``validate`` walk :func:`all_scans` and know no scan by name. Adding a scan: its kernel and
host reference, a module with a ``SCAN`` and the public functions, its name in
:data:`LATER_MODULES` (:data:`MODULES` and :data:`MORE_MODULES` are closed), the three entry points in ``_native.py`` and its keyword parameters in ``doctor``.

Every refusal is made here, in Python, before the native library is reached.
"""
from __future__ import annotations

import ctypes as C
import importlib
from dataclasses import dataclass, field
from typing import Callable, Dict, Iterable, Optional, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops.probe import ProbeError, _check

THREADS, WORDS = 256, 4
MAX_ROUNDS = 1024
DEFAULT_SEED = 0x243F6A8885A308D3
ANY = "any"
MODULES = ("cuscan", "mfmascan", "lanescan", "cachescan")    # the order of every report
MORE_MODULES = ("ldsscan",)     # the scans added since: they run and report after MODULES'
LATER_MODULES = ("sparsescan",)     # and those added after that tier was pinned: after MORE_MODULES'


def registry() -> Tuple["Scan", ...]:
    """The scans' descriptors in the order of :data:`MODULES`. The CU scan is the first: it runs
    before the host-link and atomics tests, the later scans after them."""
    return tuple(importlib.import_module(f"{__package__}.{m}").SCAN for m in MODULES)


def scans() -> Tuple["Scan", ...]:
    """:func:`registry`'s four descriptors, then those of :data:`MORE_MODULES`."""
    return registry() + tuple(importlib.import_module(f"{__package__}.{m}").SCAN
                              for m in MORE_MODULES)


def all_scans() -> Tuple["Scan", ...]:
    """Every scan's descriptor: those of :func:`scans`, then those of :data:`LATER_MODULES`. This
    is what the command line, ``doctor`` and ``validate`` walk."""
    return scans() + tuple(importlib.import_module(f"{__package__}.{m}").SCAN
                           for m in LATER_MODULES)


def decode_id(cu_id: int) -> Dict[str, int]:
    """The fields of a 12-bit CU id: XCC_ID[3:0] << 8 | HW_ID[15:8] (SE 15:13, SH 12, CU 11:8)."""
    if not isinstance(cu_id, int) or isinstance(cu_id, bool) or not 0 <= cu_id < _native.CUSCAN_IDS:
        raise ProbeError(f"cu-scan: CU id {cu_id!r} is not an integer in [0, 4096)")
    return {"xcc": cu_id >> 8, "se": (cu_id >> 5) & 7, "sh": (cu_id >> 4) & 1, "cu": cu_id & 15}


def encode_id(xcc: int, se: int, sh: int, cu: int) -> int:
    if not (0 <= xcc < 16 and 0 <= se < 8 and 0 <= sh < 2 and 0 <= cu < 16):
        raise ProbeError(f"cu-scan: no CU id for xcc {xcc} se {se} sh {sh} cu {cu}")
    return xcc << 8 | se << 5 | sh << 4 | cu


def _simds(mask: int):
    return [i for i in range(4) if mask >> i & 1]


def _ref(arg):
    return C.byref(arg) if arg is not None else None


def decode_result(dev: int, mask: int, iters: int, res, cus, n: int, bits: Dict[str, int],
                  key: str) -> Dict:
    """The result dict of a scan from the C structures; ``bits`` names the test bits and ``key``
    is what the list of the tests that ran is called (``"tests"``, hence ``"test"`` in a record
    and ``"tests_failed"`` per CU; ``"formats"`` for the matrix-core format scan)."""
    names = {v: k for k, v in bits.items()}

    def named(m: int):
        return [k for k, v in bits.items() if v & m]

    per_cu = []
    for i in range(min(n, _native.CUSCAN_IDS)):
        c = cus[i]
        per_cu.append({"id": c.id, "xcc": c.xcc, "se": c.se, "sh": c.sh, "cu": c.cu,
                       "runs": c.runs, "failed_runs": c.failed_runs,
                       f"{key}_failed": named(c.tests_failed),
                       "simds_seen": _simds(c.simds_seen),
                       "simds_failed": _simds(c.simds_failed)})
    records = []
    for i in range(res.records_filled):
        r = res.records[i]
        records.append({"id": r.id, **decode_id(r.id & (_native.CUSCAN_IDS - 1)), "simd": r.simd,
                        key[:-1]: names.get(r.test, str(r.test)), "thread": r.thread,
                        "word": r.word, "expected": f"{r.expected:#010x}",
                        "got": f"{r.got:#010x}", "xor": f"{r.expected ^ r.got:#010x}"})
    return {"device": dev, key: named(mask), "iters": iters,
            "cus_expected": res.cus_expected, "cus_seen": res.cus_seen,
            "complete": bool(res.complete), "rounds": res.rounds, "blocks_run": res.blocks_run,
            "words_in_error": res.words_in_error, "failed_cus": res.failed_cus,
            "blocks_four_simds": res.blocks_four_simds,
            "xcc_cus": list(res.xcc_cus), "seconds": res.seconds, "kernel_ms": res.kernel_ms,
            "first_errors": records,
            "failed": [{k: c[k] for k in ("id", "xcc", "se", "sh", "cu", "runs", "failed_runs",
                                          f"{key}_failed", "simds_failed")}
                       for c in per_cu if c["failed_runs"]],
            "per_cu": per_cu, "ok": res.words_in_error == 0}


def describe_failed(result: Dict, key: str = "tests") -> str:
    """One line naming the failed units of a scan's result (the first four, then how many more),
    for ``doctor``; ``key`` as in :func:`decode_result`."""
    failed = result["failed"]
    text = "; ".join(f"xcc {c['xcc']} se {c['se']} sh {c['sh']} cu {c['cu']} (id {c['id']:#05x}) "
                     f"simd {','.join(map(str, c['simds_failed']))} "
                     f"{'+'.join(c[key + '_failed'])}" for c in failed[:4])
    return text + (f"; and {len(failed) - 4} more" if len(failed) > 4 else "")


@dataclass(frozen=True)
class Scan:
    """One scan in the frame. ``key`` names its module (``gpumounter_amd.ops.<key>``), its native
    entry points (``gm_probe_<key>``, ``_expected``, ``_signature``) and its place in the JSON
    reports; ``label`` its options (``--<label>``, ``--<label>-inject`` ...) and its messages."""
    label: str                    # "lane-scan"
    key: str                      # "lanescan"
    bits: Dict[str, int]          # test or format name → its bit
    selection: str                # what scan() calls the selection: "tests" or "formats"
    default_iters: int
    max_iters: int
    title: str                    # "per-CU cache scan"; the texts below are for the help
    does: str                     # what probe's help says the scan runs on every compute unit
    flips: str                    # what the injection flips
    covers: str = ""              # appended to the title where ``does`` is not shown
    iters_unit: Optional[str] = None      # what --<label>-iters counts; None: no such option
    # a refusal beyond 1 <= iters <= max_iters: called with (mask, iters), raises ProbeError
    iters_rule: Optional[Callable[[int, int], None]] = None
    # negative controls besides "inject": name → (metavar, help, what validate's help calls it).
    # Control NAME is parsed by the module's parse_NAME and handed to its scan as _NAME.
    more_controls: Dict[str, Tuple[str, str, str]] = field(default_factory=dict)
    # The CU scan's command line is older than the frame: --cu-scan-tests and --cu-scan-rounds
    # default to all tests and 1, not to None; doctor's line does not count the tests; and only
    # probe has the negative control, doctor's and validate's command lines do not.
    plain_cli: bool = False

    @property
    def stem(self) -> str:
        """Of the argparse attributes and doctor's keyword parameters: ``lane_scan``."""
        return self.label.replace("-", "_")

    @property
    def symbol(self) -> str:
        return f"gm_probe_{self.key}"

    @property
    def unit(self) -> str:
        """One of the selection: ``test`` or ``format``."""
        return self.selection[:-1]

    @property
    def all(self) -> Tuple[str, ...]:
        return tuple(self.bits)

    @property
    def module(self):
        return importlib.import_module(f"{__package__}.{self.key}")

    @property
    def controls(self) -> Dict[str, Tuple[str, str, str]]:
        return {"inject": (f"ID|any:{self.unit.upper()}:THREAD:WORD:MASK",
                           f"negative control: flip that {self.flips} on that CU; the scan must "
                           f"name it", "negative control"), **self.more_controls}

    def run(self, dev: int, **kw) -> Dict:
        """The module's ``scan``, looked up when called (a test may have replaced it)."""
        return self.module.scan(dev, **kw)

    # ------------------------------------------------------------ names, parsers and checks
    def bit_of(self, item) -> int:
        """The bit of one test (or format), given by name or by bit."""
        if isinstance(item, str) and item in self.bits:
            return self.bits[item]
        if isinstance(item, int) and not isinstance(item, bool) and item in self.bits.values():
            return item
        raise ProbeError(f"unknown {self.label} {self.unit} {item!r} (one of "
                         f"{', '.join(self.bits)})")

    def name_of(self, item) -> str:
        bit = self.bit_of(item)
        return next(k for k, v in self.bits.items() if v == bit)

    def mask_of(self, items: Iterable) -> int:
        if isinstance(items, (str, int)):
            items = (items,)
        mask = 0
        for t in items:
            mask |= self.bit_of(t)
        if not mask:
            raise ProbeError(f"{self.label} needs at least one {self.unit}")
        return mask

    def parse_list(self, text) -> Tuple[str, ...]:
        """``"a, b"`` → ("a", "b"); every name is checked."""
        names = tuple(t.strip() for t in str(text).split(",") if t.strip())
        self.mask_of(names)
        return names

    def check_int(self, v, lo: int, hi: int, what: str) -> int:
        if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
            raise ProbeError(f"{self.label}: {what} must be an integer in [{lo}, {hi}], got {v!r}")
        return v

    def check_iters(self, mask: int, iters) -> int:
        self.check_int(iters, 1, self.max_iters, "iters")
        if self.iters_rule is not None:
            self.iters_rule(mask, iters)
        return iters

    def inject_arg(self, inject, mask: int) -> Optional[_native.CuscanInject]:
        """(id or "any", test, thread, word, xor mask) → the C struct; None stays None.
        ``mask``: what runs."""
        if inject is None:
            return None
        try:
            cu_id, item, thread, word, xor = inject
        except (TypeError, ValueError):
            raise ProbeError(f"{self.label}: injection {inject!r} is not (id, {self.unit}, "
                             f"thread, word, mask)") from None
        bit = self.bit_of(item)
        if not bit & mask:
            raise ProbeError(f"{self.label}: injection into {self.name_of(bit)!r}, which is not "
                             f"run")
        if cu_id != ANY:
            decode_id(cu_id)
        self.check_int(thread, 0, THREADS - 1, "injection thread")
        self.check_int(word, 0, WORDS - 1, "injection word")
        self.check_int(xor, 1, 0xFFFFFFFF, "injection mask")
        return _native.CuscanInject(_native.CUSCAN_ANY if cu_id == ANY else cu_id, bit, thread,
                                    word, xor)

    def parse_inject(self, text):
        """``"ID|any:TEST:THREAD:WORD:MASK"`` (integers as Python literals, e.g.
        ``0x123:mfma:130:2:0x10000``; FORMAT for TEST in the matrix-core format scan) → (id or
        "any", name, thread, word, mask)."""
        parts = [p.strip() for p in str(text).split(":")]
        if len(parts) != 5:
            raise ProbeError(f"{self.label}: cannot read {text!r} as {self.controls['inject'][0]}")
        try:
            cu_id = ANY if parts[0].lower() == ANY else int(parts[0], 0)
            thread, word, xor = (int(p, 0) for p in parts[2:])
        except ValueError:
            raise ProbeError(f"{self.label}: {text!r} holds something that is not an "
                             f"integer") from None
        inj = (cu_id, self.name_of(parts[1]), thread, word, xor)
        self.inject_arg(inj, self.bits[inj[1]])
        return inj

    # ------------------------------------------------------------ the three entry points
    # ``more(bit or mask)``, where a scan has it, checks that scan's further inputs once the
    # common ones are good and returns them as the arguments its entry point takes after them.
    def _one(self, item, seed, iters, more) -> Tuple[int, tuple]:
        bit = self.bit_of(item)
        self.check_int(seed, 0, (1 << 64) - 1, "seed"), self.check_iters(bit, iters)
        return bit, (more(bit) if more is not None else ())

    def expected(self, item, seed: int, iters: int, more=None):
        """numpy uint32[256, 4]: word i of thread t of ``item``'s signature. Host only, no GPU."""
        import numpy as np

        bit, ins = self._one(item, seed, iters, more)
        out = np.empty(THREADS * WORDS, dtype=np.uint32)
        _check(getattr(_native.probe(), self.symbol + "_expected")(
            bit, seed, iters, *ins, out.ctypes.data_as(C.POINTER(C.c_uint32))),
            f"{self.label} expected")
        return out.reshape(THREADS, WORDS)

    def signature(self, item, seed: int, iters: int, stream=None, more=None):
        """One block of the scan's device code on the current device: (uint32[256, 4] raw
        signature, where), ``where`` = the decoded CU id the block ran on plus ``id`` and
        ``simds``, the SIMD of each of its four waves."""
        bit, ins = self._one(item, seed, iters, more)
        import numpy as np
        import torch

        out = torch.zeros(THREADS * WORDS, dtype=torch.int32, device="cuda")
        where = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        s = stream if stream is not None else torch.cuda.current_stream(out.device)
        if stream is not None:
            s.wait_stream(torch.cuda.current_stream(out.device))   # out and where are filled there
        with torch.cuda.device(out.device):
            _check(getattr(_native.probe(), self.symbol + "_signature")(
                bit, seed, iters, *ins, out.data_ptr(), where.data_ptr(),
                C.c_void_p(s.cuda_stream)), f"{self.label} signature")
        s.synchronize()
        w = [int(v) & 0xFFFFFFFF for v in where.cpu().tolist()]
        sig = out.cpu().numpy().view(np.uint32).reshape(THREADS, WORDS)
        return sig, {"id": w[0], **decode_id(w[0] & (_native.CUSCAN_IDS - 1)), "simds": w[1:]}

    def scan(self, dev: int, items, iters: int, seed: int, min_rounds: int, max_rounds: int,
             inject, more=None, outs: tuple = ()) -> Dict:
        """The scan of device ``dev``: the checks, the native call and the one decoder. ``outs``:
        what the entry point takes after the frame's outputs."""
        mask = self.mask_of(items)
        self.check_iters(mask, iters)
        self.check_int(dev, 0, (1 << 31) - 1, "device")
        self.check_int(seed, 0, (1 << 64) - 1, "seed")
        self.check_int(min_rounds, 1, MAX_ROUNDS, "min_rounds")
        self.check_int(max_rounds, min_rounds, MAX_ROUNDS, "max_rounds (at least min_rounds)")
        inj = self.inject_arg(inject, mask)
        ins = more(mask) if more is not None else ()
        res = _native.CuscanResult()
        cus = (_native.CuscanCu * _native.CUSCAN_IDS)()
        n = C.c_int(0)
        _check(getattr(_native.probe(), self.symbol)(
            dev, mask, iters, seed, min_rounds, max_rounds, _ref(inj), *ins, C.byref(res), cus,
            _native.CUSCAN_IDS, C.byref(n), *outs), self.label)
        return decode_result(dev, mask, iters, res, cus, n.value, self.bits, self.selection)

    def describe_failed(self, result: Dict) -> str:
        """One line naming the failed units of a :meth:`scan` result, with what failed there."""
        return describe_failed(result, self.selection)
