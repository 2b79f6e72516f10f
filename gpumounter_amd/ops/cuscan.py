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

from typing import Dict

from gpumounter_amd.ops import cuframe
from gpumounter_amd.ops.cuframe import (ANY, DEFAULT_SEED, MAX_ROUNDS, THREADS, WORDS,  # noqa: F401
                                        decode_id, decode_result, describe_failed, encode_id)
from gpumounter_amd.ops.probe import ProbeError

TESTS = {"int": 1, "f32": 2, "mfma": 4, "lds": 8}
TEST_NAMES = {v: k for k, v in TESTS.items()}
ALL_TESTS = tuple(TESTS)
DEFAULT_ITERS = 16            # native/include/gm_cuscan_sig.h GM_CUSCAN_DEFAULT_ITERS
MAX_ITERS = 65535             # GM_CUSCAN_MAX_ITERS
MFMA_MAX_ITERS = 8191         # GM_CUSCAN_MFMA_MAX_ITERS: 32 * 16 * (4 * iters) < 2^24


def _mfma_is_exact(mask: int, iters: int) -> None:
    if mask & TESTS["mfma"] and iters > MFMA_MAX_ITERS:
        raise ProbeError(f"cu-scan: the mfma test is exact only up to iters {MFMA_MAX_ITERS} "
                         f"(32 * 16 * 4 * iters < 2^24), got {iters}")


SCAN = cuframe.Scan(
    label="cu-scan", key="cuscan", bits=TESTS, selection="tests", default_iters=DEFAULT_ITERS,
    max_iters=MAX_ITERS, iters_rule=_mfma_is_exact, plain_cli=True, title="per-CU self-test",
    does="integer, fp32, MFMA and LDS known-answer tests", flips="signature word")
bit_of, mask_of, parse_tests, parse_inject = (SCAN.bit_of, SCAN.mask_of, SCAN.parse_list,
                                              SCAN.parse_inject)


def expected(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS):
    """numpy uint32[256, 4]: word i of thread t of ``test``'s signature. Host only, no GPU."""
    return SCAN.expected(test, seed, iters)


def signature(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None):
    """One block of the scan's device code on the current device: (uint32[256, 4] raw signature,
    where), ``where`` = the decoded CU id the block ran on plus ``id`` and ``simds``, the SIMD of
    each of its four waves."""
    return SCAN.signature(test, seed, iters, stream)


def scan(dev: int, tests=ALL_TESTS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None) -> Dict:
    """The scan of device ``dev``. A round is one launch of as many blocks as the device has CUs;
    the scan stops after ``min_rounds`` once every CU has been seen, or at ``max_rounds``.
    ``_inject=(id or "any", test, thread, word, mask)`` is the negative control: that signature
    word is flipped in every block that runs on that CU, so the scan must name it.

    ``ok`` is true when no wrong word was seen; ``complete`` says separately whether every CU was
    reached (a GPU a tenant is using may legitimately not be)."""
    return SCAN.scan(dev, tests, iters, seed, min_rounds, max_rounds, _inject)
