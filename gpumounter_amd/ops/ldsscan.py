"""Per-CU LDS scan of an attached GPU (native/hip/gm_ldsscan.hip): which CU's LDS hands a lane
a wrong word on the way between the lane and the cells?

The fifth scan in the CU scan's frame (one 256-thread block per CU that declares all 160 KiB of
LDS, the CU id read from the hardware registers, a table computed on the host and compared bit for
bit). The CU scan's ``lds`` march proves that each of the 40960 words holds a value, with 32- and
128-bit plain accesses; this scan checks what sits in front of the cells. Five known-answer tests
of 4 signature words per thread:

``width``   8-bit stores read back as 16-bit (unsigned, signed) and 32-bit, 16-bit stores read back
            as bytes and 64-bit, 64- and 96-bit stores read back by the paired forms
            (``ds_read2_b32``, ``ds_read2st64_b32``; ``ds_write2_b32`` fills), and a byte and a
            halfword stored into a filled word whose other bytes must stay; every pass an
            odd-stride permutation that reads what another wave wrote
``atomic``  the LDS atomic units on a table in the LDS: thirteen 32-bit kinds, four 64-bit kinds
            and f32 add, private (returned old values folded), contended by all 256 threads and by
            the 64 lanes of one instruction (only final values folded, after a barrier), and
            tickets from one counter marked in a bitmap. No signature word depends on the order in
            which lanes or waves reach a word
``bank``    the crossbar: 32-bit writes, 32- and 64-bit reads at lane strides of 1 to 64 words
            with rotating offsets, so that every lane reads from every bank at every conflict
            degree 1 to 32, and broadcast reads (all lanes, each half, pairs ``l`` and ``l+16``)
``tr16``    gfx950's transposing read ``ds_read_b64_tr_b16`` of 4 x 16 blocks at row strides of
            32, 72 and 264 bytes, the origins sweeping the whole LDS
``dma``     direct global -> LDS loads (``global_load_lds_dword`` and ``_dwordx4``, alternating by
            chunk, the destination chunk a permutation of the source chunk) from one read-only
            160 KiB arena, read back with plain loads

The formulas are written out in native/include/gm_probe.h and implemented once for the host and
the kernel (native/include/gm_ldsscan_ref.h). :func:`expected` evaluates them without a GPU, with
or without a poked word, and :func:`signature` returns what one block computed.

Two negative controls: ``_inject`` flips a word of a computed signature as in the other scans, and
``_poke=(test, word offset, mask)`` flips a word of the data itself (of the LDS image after the
test's first fill; for ``dma`` of the arena), so that the real detection path finds it. ``atomic``
has no data to poke.

What it cannot tell: the 4-, 6- and 8-bit transposing reads are not covered (their lane maps are
not documented); cross-lane permutes through the LDS crossbar are the lane scan's; nothing judges
speed or conflict cycles; a CU id is a label. No silent fallback: a missing ``libgm_probe.so`` or
a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

from gpumounter_amd import _native
from gpumounter_amd.ops import cuframe
from gpumounter_amd.ops.cuframe import ANY, DEFAULT_SEED, _ref
from gpumounter_amd.ops.probe import ProbeError, _check

TESTS = {"width": 1, "atomic": 2, "bank": 4, "tr16": 8, "dma": 16}
TEST_NAMES = {v: k for k, v in TESTS.items()}
ALL_TESTS = tuple(TESTS)
DEFAULT_ITERS = 2             # native/include/gm_ldsscan_ref.h GM_LDSSCAN_DEFAULT_ITERS
MAX_ITERS = 63                # GM_LDSSCAN_MAX_ITERS
LDS_WORDS = 40960             # GM_LDSSCAN_WORDS, also the arena's

__all__ = ["TESTS", "ALL_TESTS", "DEFAULT_ITERS", "MAX_ITERS", "ANY", "ProbeError", "parse_tests",
           "parse_inject", "parse_poke", "expected", "signature", "scan", "kernel_info",
           "geometry", "describe_failed"]


SCAN = cuframe.Scan(
    label="lds-scan", key="ldsscan", bits=TESTS, selection="tests",
    default_iters=DEFAULT_ITERS, max_iters=MAX_ITERS, title="per-CU LDS scan",
    covers=" (access widths, LDS atomics, bank crossbar, transposing read, global-to-LDS loads)",
    does="sub-dword, wide and paired LDS accesses, the LDS atomics, the bank crossbar at every "
         "conflict degree, the transposing read and direct global-to-LDS loads",
    flips="signature word of that test", iters_unit="rounds of each test's passes",
    more_controls={"poke": (
        "TEST:WORD_OFFSET:MASK",
        "negative control: flip that word of the test's data (width, bank, tr16: of every "
        "block's LDS image after the first fill; dma: of the arena); the test must find it",
        "data poke")})
bit_of, mask_of, parse_tests, parse_inject = (SCAN.bit_of, SCAN.mask_of, SCAN.parse_list,
                                              SCAN.parse_inject)
describe_failed = SCAN.describe_failed
_int = SCAN.check_int


def _poke_arg(poke, mask: int):
    """(test, word offset, xor mask) → the C struct; None stays None. ``mask``: the tests that
    run."""
    if poke is None:
        return None
    try:
        test, offset, xor = poke
    except (TypeError, ValueError):
        raise ProbeError(f"lds-scan: poke {poke!r} is not (test, word offset, mask)") from None
    bit = bit_of(test)
    if bit == TESTS["atomic"]:
        raise ProbeError("lds-scan: atomic has no data to poke")
    if not bit & mask:
        raise ProbeError(f"lds-scan: poke of {TEST_NAMES[bit]!r}, which is not run")
    _int(offset, 0, LDS_WORDS - 1, f"poke word offset of {TEST_NAMES[bit]}")
    _int(xor, 1, 0xFFFFFFFF, "poke mask")
    return _native.LdsscanPoke(bit, offset, xor)


def parse_poke(text):
    """``"TEST:WORD_OFFSET:MASK"`` (integers as Python literals, e.g. ``tr16:4099:0x10``) →
    (test name, word offset, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    if len(parts) != 3:
        raise ProbeError(f"lds-scan: cannot read {text!r} as TEST:WORD_OFFSET:MASK")
    try:
        offset, xor = (int(p, 0) for p in parts[1:])
    except ValueError:
        raise ProbeError(f"lds-scan: {text!r} holds something that is not an integer") from None
    poke = (TEST_NAMES[bit_of(parts[0])], offset, xor)
    _poke_arg(poke, TESTS[poke[0]])
    return poke


def expected(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, poke=None):
    """numpy uint32[256, 4]: word i of thread t of ``test``'s signature, in a run with ``poke``
    (a poke of another test leaves it alone). Host only, no GPU."""
    return SCAN.expected(test, seed, iters,
                         lambda bit: (_ref(_poke_arg(poke, mask_of(ALL_TESTS))),))


def signature(test, seed: int = DEFAULT_SEED, iters: int = DEFAULT_ITERS, stream=None, poke=None):
    """One block of the scan's device code on the current device, with an arena of its own:
    (uint32[256, 4] raw signature, where), ``where`` as
    :func:`gpumounter_amd.ops.cuscan.signature` gives it. ``poke`` must name ``test``."""
    return SCAN.signature(test, seed, iters, stream, lambda bit: (_ref(_poke_arg(poke, bit)),))


def scan(dev: int, tests=ALL_TESTS, iters: int = DEFAULT_ITERS, seed: int = DEFAULT_SEED,
         min_rounds: int = 1, max_rounds: int = 16, _inject=None, _poke=None) -> Dict:
    """The scan of device ``dev``; rounds, ``ok``, ``complete`` and the result shape as in
    :func:`gpumounter_amd.ops.cuscan.scan` (``tests``, ``tests_failed`` per CU by name, ``test``
    in a record). ``_inject=(id or "any", test, thread, word, mask)`` and ``_poke=(test, word
    offset, mask)`` are the negative controls."""
    return SCAN.scan(dev, tests, iters, seed, min_rounds, max_rounds, _inject,
                     lambda mask: (_ref(_poke_arg(_poke, mask)),))


def kernel_info() -> Dict[str, int]:
    """``num_regs`` and ``scratch_bytes`` of the scan kernel as the HIP runtime reports them on
    the current device."""
    regs, scratch = C.c_int(0), C.c_int(0)
    _check(_native.probe().gm_probe_ldsscan_kernel_info(C.byref(regs), C.byref(scratch)),
           "lds-scan kernel info")
    return {"num_regs": regs.value, "scratch_bytes": scratch.value}


def geometry() -> Dict:
    """The build's constants: ``lds_bytes``, ``arena_bytes``, ``atomic_table_words`` and
    ``tr16_strides`` (bytes). Host only, no GPU."""
    v = [C.c_uint32(0) for _ in range(3)]
    strides = (C.c_uint32 * 3)()
    _check(_native.probe().gm_probe_ldsscan_geometry(*(C.byref(x) for x in v), strides),
           "lds-scan geometry")
    return {"lds_bytes": v[0].value, "arena_bytes": v[1].value,
            "atomic_table_words": v[2].value, "tr16_strides": list(strides)}
