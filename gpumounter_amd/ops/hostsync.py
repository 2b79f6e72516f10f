"""Host-GPU atomics and hand-off test of an attached GPU (native/hip/gm_hostsync.hip): can a
tenant's host code and its kernels synchronise over the link?

RCCL's proxy threads, host-polled completion flags and GPU-polled doorbells all rest on two
things: system-scope atomics on pinned host memory, which travel as PCIe AtomicOps, and
release/acquire hand-offs through flags in host memory while a kernel runs. Five tests, one bit
each (formulas: native/include/gm_probe.h; value functions and audits:
native/include/gm_hostsync_ref.h; the host threads: native/include/gm_hostsync_host.h):

``add``      no-return fetch-add, u32 and u64, by the kernel and by host threads into one table
``ticket``   returning fetch-add: GPU and host draw from the same counters, no ticket twice
``swap``     exchange chains: every value handed on exactly once
``cas``      add u64 through a compare-exchange loop, GPU and host contending
``handoff``  a ping-pong per block through flags in host memory, every payload word compared by
             the consumer, in both directions

In the atomic tests the host plays blocks ``blocks .. blocks + host_threads - 1`` with the same
value functions, so the expected tables are the atomics test's over ``blocks + host_threads``
blocks. Every wait is bounded (a count, ``budget_us`` on the GPU, ``host_budget_us`` on the host,
2 s for a host thread's start), so a call ends on any device or host state; a hand-off whose flag
was not seen in time is counted (``unseen``) and is not an error. Where the device reports no
native host atomics (``atomics_supported``) the four atomic tests are skipped and the hand-off
alone decides.

What it cannot tell: which part of the path lost a word; anything about the kinds PCIe lacks
(min, max, and, or, xor, float adds), about pageable or non-coherent host memory, about a hand-off
under a tenant's load or several GPUs behind one switch.
No silent fallback: a missing ``libgm_probe.so`` or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

from gpumounter_amd import _native
from gpumounter_amd.ops._testargs import Checks
from gpumounter_amd.ops.probe import ProbeError, _check

TESTS = {"add": 1, "ticket": 2, "swap": 4, "cas": 8, "handoff": 16}
TEST_NAMES = {v: k for k, v in TESTS.items()}
ALL_TESTS = tuple(TESTS)
ATOMIC_TESTS = ALL_TESTS[:4]
ADD_KINDS = ("add_u32", "add_u64")
# kinds of expected(): the atomics test's indices, and the swap's token list
KINDS = {"add_u32": 0, "add_u64": 1, "ticket": 10, "cas": 11, "count": 13, "swap": 14}
WIDE = frozenset(("add_u64", "cas", "swap"))      # 8-byte words
DIRECTIONS = ("h2d", "d2h")
THREADS = 256
MAX_BLOCKS = 4096             # native/include/gm_hostsync_ref.h GM_HOSTSYNC_MAX_BLOCKS
DEFAULT_BLOCKS = 16           # GM_HOSTSYNC_DEFAULT_BLOCKS: blocks=0 means min(16, CUs)
MAX_HOST_THREADS = 8
DEFAULT_HOST_THREADS = 2
MAX_ITERS = 1024
DEFAULT_ITERS = 4
MAX_OPS = 1 << 20             # (blocks + host_threads) * 256 * iters
MAX_SPREAD = 65536
DEFAULT_SPREAD = 4096
MAX_WIDTH = 1 << 21           # a widened CAS table
MAX_ROUNDS = 64
DEFAULT_ROUNDS = 8
DEFAULT_LINES = 16
MAX_BUDGET_US = 20000
DEFAULT_BUDGET_US = 2251      # the larger of 1000 and 8 x the longest poll measured, 281.36 us
#                               
MAX_HOST_BUDGET_US = 100000
DEFAULT_HOST_BUDGET_US = 5000  # the larger of 5000 and 8 x the longest poll measured, 0.13 us
MAX_MAILBOX_BYTES = 1 << 28
DEFAULT_SEED = 0x243F6A8885A308D3
ERROR_COUNTERS = ("words_in_error", "holes", "duplicates", "counter_errors", "out_of_range",
                  "swap_missing", "swap_duplicates", "swap_foreign", "cas_giveups",
                  "stale_words_h2d", "stale_words_d2h", "lost_words")
NO_ATOMICS = "the device reports no native host atomics over this link"


_checks = Checks("host-sync", TESTS)
_int, _pow2 = _checks.int_in, _checks.pow2
bit_of, mask_of, parse_tests = _checks.bit_of, _checks.mask_of, _checks.parse_tests


def _direction(d) -> int:
    if d in DIRECTIONS:
        return DIRECTIONS.index(d)
    if isinstance(d, int) and not isinstance(d, bool) and d in (0, 1):
        return d
    raise ProbeError(f"host-sync: direction {d!r} is neither h2d (0) nor d2h (1)")


def parse_inject(text):
    """The negative controls, integers as Python literals:
    ``add:KIND:G:S:MASK`` → ("add", kind name, g, s, mask); ``cas:G:S:MASK`` → ("cas", g, s,
    mask); ``ticket:G:S`` → ("ticket", g, s); ``swap:G:S:MASK`` → ("swap", g, s, mask);
    ``handoff:DIR:BLOCK:ROUND:WORD:MASK`` → ("handoff", "h2d" or "d2h", block, round, word,
    mask). ``G`` may name a host-played thread (G >= 256 * blocks)."""
    parts = [p.strip() for p in str(text).split(":")]
    forms = {"add": 5, "cas": 4, "ticket": 3, "swap": 4, "handoff": 6}
    if parts[0] not in forms or len(parts) != forms[parts[0]]:
        raise ProbeError(f"host-sync: cannot read {text!r} as add:KIND:G:S:MASK, cas:G:S:MASK, "
                         f"ticket:G:S, swap:G:S:MASK or handoff:DIR:BLOCK:ROUND:WORD:MASK")
    try:
        if parts[0] == "add":
            kind = parts[1] if parts[1] in ADD_KINDS else ADD_KINDS[int(parts[1], 0)] \
                if parts[1] in ("0", "1") else None
            if kind is None:
                raise ProbeError(f"host-sync: {parts[1]!r} is not a kind of the add test "
                                 f"({', '.join(ADD_KINDS)})")
            inj = ("add", kind) + tuple(int(p, 0) for p in parts[2:])
        elif parts[0] == "handoff":
            d = parts[1] if parts[1] in DIRECTIONS else int(parts[1], 0)
            inj = ("handoff", DIRECTIONS[_direction(d)]) + tuple(int(p, 0) for p in parts[2:])
        else:
            inj = (parts[0],) + tuple(int(p, 0) for p in parts[1:])
    except ValueError:
        raise ProbeError(f"host-sync: {text!r} holds something that is not an integer") from None
    _inject_arg(inj)
    return inj


def _inject_arg(inject, mask: Optional[int] = None, blocks: int = 0, host_threads: int = 0,
                iters: int = 0, rounds: int = 0, lines: int = 0
                ) -> Optional[_native.HostsyncInject]:
    """A parse_inject tuple → the C struct; None stays None. With a geometry (blocks != 0) the
    place is checked against it; the native call checks it again once the block count is known."""
    if inject is None:
        return None
    try:
        bit = bit_of(inject[0])
        name = TEST_NAMES[bit]
        if name == "add":
            _, kind, a, b, xor = inject
            if kind not in ADD_KINDS:
                raise ProbeError(f"host-sync: {kind!r} is not a kind of the add test")
            k, word = ADD_KINDS.index(kind), 0
        elif name in ("cas", "swap"):
            (_, a, b, xor), k, word = inject, 0, 0
        elif name == "ticket":
            (_, a, b), k, word, xor = inject, 0, 0, 0
        else:
            _, d, a, b, word, xor = inject
            k = _direction(d)
    except (TypeError, ValueError, IndexError):
        raise ProbeError(f"host-sync: injection {inject!r} is not one of parse_inject's "
                         f"forms") from None
    if mask is not None and not bit & mask:
        raise ProbeError(f"host-sync: injection into {name!r}, which is not run")
    if name == "handoff":
        _int(a, 0, (blocks or MAX_BLOCKS) - 1, "injection block")
        _int(b, 0, (rounds or MAX_ROUNDS) - 1, "injection round")
        _int(word, 0, (lines or 16) * 1024 - 1, "injection word")
    else:
        top = (blocks + host_threads if blocks else MAX_BLOCKS + MAX_HOST_THREADS) * THREADS
        _int(a, 0, top - 1, "injection thread g")
        _int(b, 0, (iters or MAX_ITERS) - 1, "injection step s")
    if name != "ticket":
        _int(xor, 1, 0xFFFFFFFF, "injection mask")
    return _native.HostsyncInject(bit, k, a, b, word, xor)


def _geometry(blocks, host_threads, iters, lo_blocks: int = 1) -> None:
    _int(blocks, lo_blocks, MAX_BLOCKS, "blocks")
    _int(host_threads, 0, MAX_HOST_THREADS, "host_threads")
    _int(iters, 1, MAX_ITERS, "iters")
    if (max(blocks, 1) + host_threads) * THREADS * iters > MAX_OPS:
        raise ProbeError(f"host-sync: (blocks + host_threads) * 256 * iters must not exceed "
                         f"{MAX_OPS}, got ({blocks} + {host_threads}) * 256 * {iters}")


def _handoff_args(blocks, host_threads, rounds, lines, budget_us, host_budget_us,
                  lo_blocks: int = 1, run_it: bool = True) -> None:
    _int(blocks, lo_blocks, MAX_BLOCKS, "blocks")
    _int(host_threads, 0, MAX_HOST_THREADS, "host_threads")
    if run_it and host_threads < 1:
        raise ProbeError("host-sync: the hand-off needs at least one host thread")
    _int(rounds, 1, MAX_ROUNDS, "rounds")
    if lines not in (1, 16) or isinstance(lines, bool):
        raise ProbeError(f"host-sync: lines must be 1 or 16, got {lines!r}")
    _int(budget_us, 1, MAX_BUDGET_US, "budget_us")
    _int(host_budget_us, 1, MAX_HOST_BUDGET_US, "host_budget_us")
    if 2 * max(blocks, 1) * rounds * (lines * 4096 + 128) > MAX_MAILBOX_BYTES:
        raise ProbeError(f"host-sync: {blocks} blocks x {rounds} rounds x {lines} lines need more "
                         f"than 256 MiB of pinned mailboxes")


def cas_width(blocks: int, host_threads: int = DEFAULT_HOST_THREADS, iters: int = DEFAULT_ITERS,
              spread: int = DEFAULT_SPREAD) -> int:
    """The CAS table's words for a requested ``spread``: the atomics test's width rule over
    ``blocks + host_threads`` blocks. Host only."""
    _geometry(blocks, host_threads, iters), _pow2(spread, MAX_SPREAD, "spread")
    w = C.c_uint32(0)
    _check(_native.probe().gm_probe_hostsync_cas_width(blocks, host_threads, iters, spread,
                                                       C.byref(w)), "host-sync cas width")
    return w.value


def expected(kind, blocks: int, host_threads: int = DEFAULT_HOST_THREADS,
             iters: int = DEFAULT_ITERS, spread: int = DEFAULT_SPREAD, seed: int = DEFAULT_SEED,
             width: Optional[int] = None):
    """What the host expects for ``blocks`` GPU blocks and ``host_threads`` host-played ones.
    ``"add_u32"``, ``"add_u64"``, ``"cas"``: the final table (numpy uint32[W] or uint64[W]);
    ``"ticket"``: the counters' final values; ``"count"``: the operations per word; ``"swap"``:
    uint64[(blocks + host_threads) * 256 * iters], ``word << 32 | token`` of operation
    ``g * iters + s``. W is ``width`` if given, else ``spread`` (for ``"cas"``: :func:`cas_width`).
    Host only, no GPU."""
    import numpy as np

    if kind not in KINDS:
        raise ProbeError(f"unknown host-sync kind {kind!r} (one of {', '.join(KINDS)})")
    _geometry(blocks, host_threads, iters), _int(seed, 0, (1 << 64) - 1, "seed")
    if width is None:
        _pow2(spread, MAX_SPREAD, "spread")
        width = cas_width(blocks, host_threads, iters, spread) if kind == "cas" else spread
    _pow2(width, MAX_WIDTH, "width")
    n = (blocks + host_threads) * THREADS * iters if kind == "swap" else width
    out = np.empty(n, dtype=np.uint64 if kind in WIDE else np.uint32)
    rc = _native.probe().gm_probe_hostsync_expected(KINDS[kind], blocks, host_threads, iters,
                                                    width, seed, out.ctypes.data_as(C.c_void_p),
                                                    out.nbytes)
    if rc == 1:
        raise ProbeError(f"host-sync: {kind} is refused at width {width} for {blocks} + "
                         f"{host_threads} blocks x {iters} iters (too many operations into one "
                         f"word)")
    _check(rc, "host-sync expected")
    return out


def payload(direction, block: int, round_: int, word: int, seed: int = DEFAULT_SEED) -> int:
    """E(dir, block, round, word): what the hand-off stores there. Host only."""
    d = _direction(direction)
    _int(block, 0, MAX_BLOCKS - 1, "block"), _int(round_, 0, MAX_ROUNDS - 1, "round")
    _int(word, 0, 16 * 1024 - 1, "word")
    return int(_native.probe().gm_probe_hostsync_payload(seed, d, block, round_, word))


def atomics_supported(dev: int = 0) -> bool:
    """hipDeviceAttributeHostNativeAtomicSupported of device ``dev``."""
    _int(dev, 0, (1 << 31) - 1, "device")
    v = C.c_int(0)
    _check(_native.probe().gm_probe_hostsync_supported(dev, C.byref(v)), "host-sync supported")
    return bool(v.value)


# ------------------------------------------------- per-test calls on the current device
def _stream_arg(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def _byref(inj):
    return C.byref(inj) if inj is not None else None


def _records(res):
    out = []
    for i in range(res.records_filled):
        r = res.records[i]
        name = TEST_NAMES.get(r.test, str(r.test))
        rec = {"test": name, "index": r.index, "expected": f"{r.expected:#x}",
               "got": f"{r.got:#x}", "xor": f"{r.expected ^ r.got:#x}"}
        if name == "add":
            rec["kind"] = ADD_KINDS[r.kind] if r.kind < len(ADD_KINDS) else str(r.kind)
        if name == "handoff":
            rec["direction"] = DIRECTIONS[r.kind & 1]
            rec["found"] = "audit" if r.where == _native.HOSTSYNC_WHERE_LOST else "consumer"
            if r.index >> 40:
                rec.update(block=(r.index >> 6) & 0xFFF, round=r.index & 63, flag=True)
            else:
                rec.update(block=r.index >> 20, round=(r.index >> 14) & 63,
                           word=r.index & 0x3FFF)
        out.append(rec)
    return out


def _dir_fields(d) -> Dict:
    return {"handoffs": d.handoffs, "observed": d.observed, "unseen": d.unseen,
            "stale_words": d.stale_words, "poll_max_us": d.poll_max_us}


def _handoff_fields(res) -> Dict:
    return {"h2d": _dir_fields(res.dir[0]), "d2h": _dir_fields(res.dir[1]),
            "stale_words_h2d": res.dir[0].stale_words, "stale_words_d2h": res.dir[1].stale_words,
            "lost_words": res.lost_words, "rtt_median_us": res.rtt_median_us,
            "rtt_max_us": res.rtt_max_us}


def add(kind, blocks: int, host_threads: int = DEFAULT_HOST_THREADS, iters: int = DEFAULT_ITERS,
        width: int = DEFAULT_SPREAD, seed: int = DEFAULT_SEED, stream=None, _inject=None):
    """One launch of one kind of the add test, with its host threads, on a fresh table on the
    current device: numpy uint32[width] or uint64[width], to be compared with :func:`expected`."""
    import numpy as np

    if kind not in ADD_KINDS:
        raise ProbeError(f"host-sync: {kind!r} is not a kind of the add test")
    _geometry(blocks, host_threads, iters), _pow2(width, MAX_SPREAD, "width")
    inj = _inject_arg(_inject, TESTS["add"], blocks, host_threads, iters)
    table = np.empty(width, dtype=np.uint64 if kind in WIDE else np.uint32)
    res = _native.HostsyncResult()
    _check(_native.probe().gm_probe_hostsync_add(
        ADD_KINDS.index(kind), blocks, host_threads, iters, width, seed, _byref(inj),
        _stream_arg(stream), table.ctypes.data_as(C.c_void_p), C.byref(res)), "host-sync add")
    return table


def cas(blocks: int, host_threads: int = DEFAULT_HOST_THREADS, iters: int = DEFAULT_ITERS,
        width: int = DEFAULT_SPREAD, seed: int = DEFAULT_SEED, stream=None, _inject=None):
    """The CAS test on a fresh table of ``width`` words (see :func:`cas_width`): (numpy
    uint64[width], {"cas_giveups": n, "host_ops_in_flight": n})."""
    import numpy as np

    _geometry(blocks, host_threads, iters), _pow2(width, MAX_WIDTH, "width")
    inj = _inject_arg(_inject, TESTS["cas"], blocks, host_threads, iters)
    table = np.empty(width, dtype=np.uint64)
    res = _native.HostsyncResult()
    _check(_native.probe().gm_probe_hostsync_cas(
        blocks, host_threads, iters, width, seed, _byref(inj), _stream_arg(stream),
        table.ctypes.data_as(C.c_void_p), C.byref(res)), "host-sync cas")
    return table, {"cas_giveups": res.cas_giveups, "host_ops_in_flight": res.host_ops_in_flight}


def ticket(blocks: int, host_threads: int = DEFAULT_HOST_THREADS, iters: int = DEFAULT_ITERS,
           counters: int = DEFAULT_SPREAD, seed: int = DEFAULT_SEED, stream=None,
           _inject=None) -> Dict:
    """The ticket test on fresh counters and marks: its counters of the result."""
    _geometry(blocks, host_threads, iters), _pow2(counters, MAX_SPREAD, "counters")
    inj = _inject_arg(_inject, TESTS["ticket"], blocks, host_threads, iters)
    res = _native.HostsyncResult()
    _check(_native.probe().gm_probe_hostsync_ticket(
        blocks, host_threads, iters, counters, seed, _byref(inj), _stream_arg(stream),
        C.byref(res)), "host-sync ticket")
    return {"tickets": res.tickets, "holes": res.holes, "duplicates": res.duplicates,
            "counter_errors": res.counter_errors, "out_of_range": res.out_of_range,
            "host_ops_in_flight": res.host_ops_in_flight, "first_errors": _records(res)}


def swap(blocks: int, host_threads: int = DEFAULT_HOST_THREADS, iters: int = DEFAULT_ITERS,
         width: int = DEFAULT_SPREAD, seed: int = DEFAULT_SEED, stream=None,
         _inject=None) -> Dict:
    """The swap test on fresh words: its counters of the result."""
    _geometry(blocks, host_threads, iters), _pow2(width, MAX_SPREAD, "width")
    inj = _inject_arg(_inject, TESTS["swap"], blocks, host_threads, iters)
    res = _native.HostsyncResult()
    _check(_native.probe().gm_probe_hostsync_swap(
        blocks, host_threads, iters, width, seed, _byref(inj), _stream_arg(stream),
        C.byref(res)), "host-sync swap")
    return {"swaps": res.swaps, "swap_missing": res.swap_missing,
            "swap_duplicates": res.swap_duplicates, "swap_foreign": res.swap_foreign,
            "host_ops_in_flight": res.host_ops_in_flight, "first_errors": _records(res)}


def handoff(blocks: int, host_threads: int = DEFAULT_HOST_THREADS, rounds: int = DEFAULT_ROUNDS,
            lines: int = DEFAULT_LINES, budget_us: int = DEFAULT_BUDGET_US,
            host_budget_us: int = DEFAULT_HOST_BUDGET_US, seed: int = DEFAULT_SEED, stream=None,
            _inject=None) -> Dict:
    """The hand-off test on fresh mailboxes: its counters of the result."""
    _handoff_args(blocks, host_threads, rounds, lines, budget_us, host_budget_us)
    inj = _inject_arg(_inject, TESTS["handoff"], blocks, host_threads, 0, rounds, lines)
    res = _native.HostsyncResult()
    _check(_native.probe().gm_probe_hostsync_handoff(
        blocks, host_threads, rounds, lines, budget_us, host_budget_us, seed, _byref(inj),
        _stream_arg(stream), C.byref(res)), "host-sync handoff")
    out = _handoff_fields(res)
    out["first_errors"] = _records(res)
    return out


def _test_names(mask: int):
    return [n for n in TESTS if TESTS[n] & mask]


def run(dev: int, tests=ALL_TESTS, blocks: int = 0, host_threads: int = DEFAULT_HOST_THREADS,
        iters: int = DEFAULT_ITERS, spread: int = DEFAULT_SPREAD, rounds: int = DEFAULT_ROUNDS,
        lines: int = DEFAULT_LINES, budget_us: int = DEFAULT_BUDGET_US,
        host_budget_us: int = DEFAULT_HOST_BUDGET_US, seed: int = DEFAULT_SEED,
        _inject=None) -> Dict:
    """The tests of ``tests`` on device ``dev``; ``blocks`` 0 means min(16, CUs), so that every
    block is resident. ``_inject`` is a negative control in one of :func:`parse_inject`'s forms.

    ``ok`` is about data only: every error counter is 0. ``unseen`` hand-offs and skipped tests
    never change it. ``tests_skipped`` maps each atomic test that was asked for and not launched
    to the reason (``atomics_supported`` is false). ``handoff_vacuous`` says that the hand-off ran
    and one direction observed not one flag in time, so that it proved nothing there.
    ``host_ops_in_flight`` is informational: the host operations made while the kernels ran."""
    mask = mask_of(tests)
    _int(dev, 0, (1 << 31) - 1, "device"), _int(seed, 0, (1 << 64) - 1, "seed")
    _geometry(blocks, host_threads, iters, 0), _pow2(spread, MAX_SPREAD, "spread")
    _handoff_args(blocks, host_threads, rounds, lines, budget_us, host_budget_us, 0,
                  bool(mask & TESTS["handoff"]))
    inj = _inject_arg(_inject, mask, blocks, host_threads, iters, rounds, lines)
    res = _native.HostsyncResult()
    _check(_native.probe().gm_probe_hostsync(
        dev, mask, blocks, host_threads, iters, spread, rounds, lines, budget_us, host_budget_us,
        seed, _byref(inj), C.byref(res)), "host-sync")
    ran = _test_names(res.tests_run)
    out = {"device": dev, "tests": ran,
           "tests_skipped": {n: NO_ATOMICS for n in _test_names(res.tests_skipped)},
           "atomics_supported": bool(res.atomics_supported), "blocks": res.blocks,
           "host_threads": res.host_threads, "iters": res.iters, "spread": res.spread,
           "rounds": res.rounds, "lines": res.lines, "budget_us": res.budget_us,
           "host_budget_us": res.host_budget_us, "cas_width": res.cas_width,
           "words_in_error": res.words_in_error, "add_u32_errors": res.add_u32_errors,
           "add_u64_errors": res.add_u64_errors, "cas_errors": res.cas_errors,
           "tickets": res.tickets, "holes": res.holes, "duplicates": res.duplicates,
           "counter_errors": res.counter_errors, "out_of_range": res.out_of_range,
           "swaps": res.swaps, "swap_missing": res.swap_missing,
           "swap_duplicates": res.swap_duplicates, "swap_foreign": res.swap_foreign,
           "cas_giveups": res.cas_giveups, "host_ops_in_flight": res.host_ops_in_flight,
           "ms": {n: res.ms[i] for i, n in enumerate(ALL_TESTS) if n in ran},
           "seconds": res.seconds}
    out.update(_handoff_fields(res))
    out["first_errors"] = _records(res)
    out["handoff_vacuous"] = "handoff" in ran and (res.dir[0].observed == 0
                                                   or res.dir[1].observed == 0)
    out["ok"] = all(out[c] == 0 for c in ERROR_COUNTERS)
    return out


def describe_failed(result: Dict) -> str:
    """One line naming what a :func:`run` result found wrong: the nonzero error counters and the
    first record with its test, its direction and its place, for ``doctor``."""
    parts = [f"{c} {result[c]}" for c in ERROR_COUNTERS if result[c]]
    if result["first_errors"]:
        r = result["first_errors"][0]
        if r["test"] == "handoff":
            where = (f"handoff {r['direction']} block {r['block']} round {r['round']} "
                     + ("flag" if r.get("flag") else f"word {r['word']}")
                     + f" (by the {r['found']})")
        else:
            where = f"{r.get('kind', r['test'])} index {r['index']}"
        parts.append(f"first: {where} expected {r['expected']} got {r['got']}")
    return "; ".join(parts)
