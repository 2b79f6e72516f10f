"""Per-compute-unit self-test of an attached GPU (native/hip/gm_cuscan.hip): which CU computes a
wrong word?

The liveness kernel looks at one CU and the burn-in can only say that some word of a large result
differed. The scan runs four short known-answer tests (integer VALU, fp32 FMA, bf16 MFMA, a march
over the whole 160 KiB of LDS) in blocks that each fill a CU, compares every thread's four
signature words per test with a table computed on the host, and books each outcome under the CU
id the block read from the hardware registers. The signature is a pure function of (test, seed,
iters, thread) (formulas: native/include/gm_probe.h); :func:`expected` evaluates it without a GPU
and :func:`signature` returns what one block computed.

What it cannot tell: clocks and thermals are not covered (transcendental units, register-file
addressing, the scalar unit and the cross-lane network are in :mod:`gpumounter_amd.ops.lanescan`,
the vector L1, L2, scalar and instruction caches in :mod:`gpumounter_amd.ops.cachescan`); a CU id is a label from the hardware registers, not a verified die position; and where
blocks run is up to the dispatcher, so on a GPU that is in use some CUs may not be reached
(``complete`` is false then, which is not an error: ``ok`` says whether a wrong word was seen).
No silent fallback: a missing ``libgm_probe.so`` or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Tuple

from gpumounter_amd import _native
from gpumounter_amd.ops.probe import ProbeError, _check

TESTS = {"int": 1, "f32": 2, "mfma": 4, "lds": 8}
TEST_NAMES = {v: k for k, v in TESTS.items()}
ALL_TESTS = tuple(TESTS)
DEFAULT_ITERS = 16            # native/include/gm_cuscan_sig.h GM_CUSCAN_DEFAULT_ITERS
MAX_ITERS = 65535             # GM_CUSCAN_MAX_ITERS
MFMA_MAX_ITERS = 8191         # GM_CUSCAN_MFMA_MAX_ITERS: 32 * 16 * (4 * iters) < 2^24
MAX_ROUNDS = 1024
DEFAULT_SEED = 0x243F6A8885A308D3
THREADS, WORDS = 256, 4
ANY = "any"


def bit_of(test) -> int:
    """The bit of one test, given by name or by bit."""
    if isinstance(test, str) and test in TESTS:
        return TESTS[test]
    if isinstance(test, int) and not isinstance(test, bool) and test in TEST_NAMES:
        return test
    raise ProbeError(f"unknown cu-scan test {test!r} (one of {', '.join(TESTS)})")


def mask_of(tests: Iterable) -> int:
    if isinstance(tests, (str, int)):
        tests = (tests,)
    mask = 0
    for t in tests:
        mask |= bit_of(t)
    if not mask:
        raise ProbeError("cu-scan needs at least one test")
    return mask


def parse_tests(text) -> Tuple[str, ...]:
    """``"int,f32,mfma,lds"`` → ("int", "f32", "mfma", "lds"); every name is checked."""
    names = tuple(t.strip() for t in str(text).split(",") if t.strip())
    mask_of(names)
    return names


def decode_id(cu_id: int) -> Dict[str, int]:
    """The fields of a 12-bit CU id: XCC_ID[3:0] << 8 | HW_ID[15:8] (SE 15:13, SH 12, CU 11:8)."""
    if not isinstance(cu_id, int) or isinstance(cu_id, bool) or not 0 <= cu_id < _native.CUSCAN_IDS:
        raise ProbeError(f"cu-scan: CU id {cu_id!r} is not an integer in [0, 4096)")
    return {"xcc": cu_id >> 8, "se": (cu_id >> 5) & 7, "sh": (cu_id >> 4) & 1, "cu": cu_id & 15}


def encode_id(xcc: int, se: int, sh: int, cu: int) -> int:
    if not (0 <= xcc < 16 and 0 <= se < 8 and 0 <= sh < 2 and 0 <= cu < 16):
        raise ProbeError(f"cu-scan: no CU id for xcc {xcc} se {se} sh {sh} cu {cu}")
    return xcc << 8 | se << 5 | sh << 4 | cu


def _int(v, lo: int, hi: int, what: str) -> int:
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise ProbeError(f"cu-scan: {what} must be an integer in [{lo}, {hi}], got {v!r}")
    return v


def _iters(mask: int, iters) -> int:
    _int(iters, 1, MAX_ITERS, "iters")
    if mask & TESTS["mfma"] and iters > MFMA_MAX_ITERS:
        raise ProbeError(f"cu-scan: the mfma test is exact only up to iters {MFMA_MAX_ITERS} "
                         f"(32 * 16 * 4 * iters < 2^24), got {iters}")
    return iters


def _inject_arg(inject, mask: int) -> Optional[_native.CuscanInject]:
    """(id or "any", test, thread, word, xor mask) → the C struct; None stays None."""
    if inject is None:
        return None
    try:
        cu_id, test, thread, word, xor = inject
    except (TypeError, ValueError):
        raise ProbeError(f"cu-scan: injection {inject!r} is not (id, test, thread, word, "
                         f"mask)") from None
    bit = bit_of(test)
    if not bit & mask:
        raise ProbeError(f"cu-scan: injection into {TEST_NAMES[bit]!r}, which is not run")
    if cu_id != ANY:
        decode_id(cu_id)
    _int(thread, 0, THREADS - 1, "injection thread")
    _int(word, 0, WORDS - 1, "injection word")
    _int(xor, 1, 0xFFFFFFFF, "injection mask")
    return _native.CuscanInject(_native.CUSCAN_ANY if cu_id == ANY else cu_id, bit, thread, word,
                                xor)


def parse_inject(text):
    """``"ID|any:TEST:THREAD:WORD:MASK"`` (integers as Python literals, e.g.
    ``0x123:mfma:130:2:0x10000``) → (id or "any", test name, thread, word, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    if len(parts) != 5:
        raise ProbeError(f"cu-scan: cannot read {text!r} as ID|any:TEST:THREAD:WORD:MASK")
    try:
        cu_id = ANY if parts[0].lower() == ANY else int(parts[0], 0)
        thread, word, xor = (int(p, 0) for p in parts[2:])
    except ValueError:
        raise ProbeError(f"cu-scan: {text!r} holds something that is not an integer") from None
    inj = (cu_id, TEST_NAMES[bit_of(parts[1])], thread, word, xor)
    _inject_arg(inj, TESTS[inj[1]])
    return inj


def expected(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS):
    """numpy uint32[256, 4]: word i of thread t of ``test``'s signature. Host only, no GPU."""
    import numpy as np

    bit = bit_of(test)
    _int(seed, 0, (1 << 64) - 1, "seed"), _iters(bit, iters)
    out = np.empty(THREADS * WORDS, dtype=np.uint32)
    _check(_native.probe().gm_probe_cuscan_expected(
        bit, seed, iters, out.ctypes.data_as(C.POINTER(C.c_uint32))), "cu-scan expected")
    return out.reshape(THREADS, WORDS)


def signature(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None):
    """One block of the scan's device code on the current device: (uint32[256, 4] raw signature,
    where), ``where`` = the decoded CU id the block ran on plus ``id`` and ``simds``, the SIMD of
    each of its four waves."""
    import numpy as np
    import torch

    bit = bit_of(test)
    _int(seed, 0, (1 << 64) - 1, "seed"), _iters(bit, iters)
    out = torch.zeros(THREADS * WORDS, dtype=torch.int32, device="cuda")
    where = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream(out.device)
    with torch.cuda.device(out.device):
        _check(_native.probe().gm_probe_cuscan_signature(
            bit, seed, iters, out.data_ptr(), where.data_ptr(), C.c_void_p(s.cuda_stream)),
            "cu-scan signature")
    s.synchronize()
    w = [int(v) & 0xFFFFFFFF for v in where.cpu().tolist()]
    sig = out.cpu().numpy().view(np.uint32).reshape(THREADS, WORDS)
    return sig, {"id": w[0], **decode_id(w[0] & (_native.CUSCAN_IDS - 1)), "simds": w[1:]}


def _simds(mask: int):
    return [i for i in range(4) if mask >> i & 1]


def scan(dev: int, tests=ALL_TESTS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None) -> Dict:
    """The scan of device ``dev``. A round is one launch of as many blocks as the device has CUs;
    the scan stops after ``min_rounds`` once every CU has been seen, or at ``max_rounds``.
    ``_inject=(id or "any", test, thread, word, mask)`` is the negative control: that signature
    word is flipped in every block that runs on that CU, so the scan must name it.

    ``ok`` is true when no wrong word was seen; ``complete`` says separately whether every CU was
    reached (a GPU a tenant is using may legitimately not be)."""
    mask = mask_of(tests)
    _iters(mask, iters)
    _int(dev, 0, (1 << 31) - 1, "device")
    _int(seed, 0, (1 << 64) - 1, "seed")
    _int(min_rounds, 1, MAX_ROUNDS, "min_rounds")
    _int(max_rounds, min_rounds, MAX_ROUNDS, "max_rounds (at least min_rounds)")
    inj = _inject_arg(_inject, mask)
    res = _native.CuscanResult()
    cus = (_native.CuscanCu * _native.CUSCAN_IDS)()
    n = C.c_int(0)
    _check(_native.probe().gm_probe_cuscan(
        dev, mask, iters, seed, min_rounds, max_rounds,
        C.byref(inj) if inj is not None else None, C.byref(res), cus,
        _native.CUSCAN_IDS, C.byref(n)), "cu-scan")
    return decode_result(dev, mask, iters, res, cus, n.value, TESTS, "tests")


def decode_result(dev: int, mask: int, iters: int, res, cus, n: int, bits: Dict[str, int],
                  key: str) -> Dict:
    """The result dict of a scan in the CU scan's frame (this one and
    :mod:`gpumounter_amd.ops.mfmascan`) from the C structures; ``bits`` names the test bits and
    ``key`` is what the list of the tests that ran is called (``"tests"`` here, hence ``"test"`` in
    a record and ``"tests_failed"`` per CU)."""
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
    """One line naming the failed units of a :func:`scan` result (the first four, then how many
    more), for ``doctor``; ``key`` as in :func:`decode_result`."""
    failed = result["failed"]
    text = "; ".join(f"xcc {c['xcc']} se {c['se']} sh {c['sh']} cu {c['cu']} (id {c['id']:#05x}) "
                     f"simd {','.join(map(str, c['simds_failed']))} "
                     f"{'+'.join(c[key + '_failed'])}" for c in failed[:4])
    return text + (f"; and {len(failed) - 4} more" if len(failed) > 4 else "")
