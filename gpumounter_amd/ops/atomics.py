"""Cross-XCC atomics and coherence test of an attached GPU (native/hip/gm_atomics.hip): does what
connects the eight XCCs work?

An MI355X has eight XCCs, each with a private L2 that is not coherent with the others, and
memory-side atomic units behind them. Four tests, one bit each (formulas:
native/include/gm_probe.h; value functions and host reference: native/include/gm_atomics_ref.h):

``add``      no-return atomics of ten kinds (integer add/xor/max/min/and/or, f32, f64 and packed
             bf16 add) whose operations commute, so the host gives the exact final table
``ticket``   returning fetch-add: no ticket may be handed out twice or left out
``cas``      add u64 through a compare-exchange loop with a host-counted retry bound
``handoff``  in-launch message passing between blocks with the documented agent-scope release
             and acquire, every word checked by an L1-warm consumer

No kernel waits without a bound on another block, so a call ends on any device state; a hand-off
whose flag was not seen within the budget is counted (``unseen``) and is not an error. XCC ids are
labels read from the hardware registers; no result depends on where a block ran.

What it cannot tell: system-scope or host memory (``ops.hostsync`` has those), LDS atomics,
several GPUs, a hand-off under a tenant's load. The counter a ticket is drawn from is computed at run time, so the compiler
does not fold a wave's draws into one add: per-lane returning atomics reach the hardware at every
``spread`` (checked in the assembly, profiles/atomics/README.md).
No silent fallback: a missing ``libgm_probe.so`` or a HIP failure raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

from gpumounter_amd import _native
from gpumounter_amd.ops._testargs import Checks
from gpumounter_amd.ops.probe import ProbeError, _check

TESTS = {"add": 1, "ticket": 2, "cas": 4, "handoff": 8}
TEST_NAMES = {v: k for k, v in TESTS.items()}
ALL_TESTS = tuple(TESTS)
KINDS = ("add_u32", "add_u64", "xor_u64", "umax_u32", "umin_u32", "and_u32", "or_u32",
         "add_f32", "add_f64", "pk_add_bf16", "ticket", "cas", "handoff")
ADD_KINDS = KINDS[:10]
COUNT = "count"               # pseudo-kind of expected(): operations per word
WIDE = frozenset(("add_u64", "xor_u64", "add_f64", "cas"))   # 8-byte words
THREADS = 256
MAX_BLOCKS = 4096             # native/include/gm_atomics_ref.h GM_ATOMICS_MAX_BLOCKS
MAX_ITERS = 1024              # GM_ATOMICS_MAX_ITERS
MAX_OPS = 1 << 26             # GM_ATOMICS_MAX_OPS
MAX_SPREAD = 65536            # GM_ATOMICS_MAX_SPREAD
MAX_WIDTH = 1 << 21           # GM_ATOMICS_MAX_WIDTH
MAX_ROUNDS = 64
MAX_BUDGET_US = 1000
MAX_MAILBOX_BYTES = 1 << 30
DEFAULT_ITERS = 8
DEFAULT_SPREAD = 4096
DEFAULT_ROUNDS = 8
DEFAULT_LINES = 16
DEFAULT_BUDGET_US = 200       # the larger of 200 and 8 x the longest poll measured
DEFAULT_SEED = 0x243F6A8885A308D3
ERROR_COUNTERS = ("words_in_error", "holes", "duplicates", "counter_errors", "order_violations",
                  "out_of_range", "cas_giveups", "stale_words", "lost_words")


_checks = Checks("atomics", TESTS)
_int, _pow2 = _checks.int_in, _checks.pow2
bit_of, mask_of, parse_tests = _checks.bit_of, _checks.mask_of, _checks.parse_tests


def kind_of(kind) -> int:
    """The index of a kind, given by name or by index; ``"count"`` is 13."""
    if kind == COUNT:
        return len(KINDS)
    if isinstance(kind, str) and kind in KINDS:
        return KINDS.index(kind)
    if isinstance(kind, int) and not isinstance(kind, bool) and 0 <= kind < len(KINDS):
        return kind
    raise ProbeError(f"unknown atomics kind {kind!r} (one of {', '.join(KINDS)})")


def parse_spread(text) -> int:
    try:
        return _pow2(int(str(text), 0), MAX_SPREAD, "spread")
    except ValueError:
        raise ProbeError(f"atomics: spread {text!r} is not an integer") from None


def parse_inject(text):
    """The negative controls, integers as Python literals:
    ``add:KIND:G:S:MASK`` → ("add", kind name, g, s, mask); ``cas:G:S:MASK`` → ("cas", g, s,
    mask); ``ticket:G:S`` → ("ticket", g, s); ``handoff:BLOCK:ROUND:WORD:MASK`` → ("handoff",
    block, round, word, mask)."""
    parts = [p.strip() for p in str(text).split(":")]
    forms = {"add": 5, "cas": 4, "ticket": 3, "handoff": 5}
    if parts[0] not in forms or len(parts) != forms[parts[0]]:
        raise ProbeError(f"atomics: cannot read {text!r} as add:KIND:G:S:MASK, cas:G:S:MASK, "
                         f"ticket:G:S or handoff:BLOCK:ROUND:WORD:MASK")
    try:
        if parts[0] == "add":
            inj = ("add", KINDS[kind_of(parts[1])]) + tuple(int(p, 0) for p in parts[2:])
        else:
            inj = (parts[0],) + tuple(int(p, 0) for p in parts[1:])
    except ValueError:
        raise ProbeError(f"atomics: {text!r} holds something that is not an integer") from None
    _inject_arg(inj)
    return inj


def _inject_arg(inject, mask: Optional[int] = None) -> Optional[_native.AtomicsInject]:
    """A parse_inject tuple → the C struct; None stays None. What depends on the run's geometry
    is checked by the native call."""
    if inject is None:
        return None
    try:
        test = inject[0]
        bit = bit_of(test)
        name = TEST_NAMES[bit]
        if name == "add":
            _, kind, a, b, xor = inject
            k, word = kind_of(kind), 0
            if k >= len(ADD_KINDS):
                raise ProbeError(f"atomics: {kind!r} is not a kind of the add test")
        elif name == "cas":
            (_, a, b, xor), k, word = inject, KINDS.index("cas"), 0
        elif name == "ticket":
            (_, a, b), k, word, xor = inject, KINDS.index("ticket"), 0, 0
        else:
            (_, a, b, word, xor), k = inject, KINDS.index("handoff")
    except (TypeError, ValueError, IndexError):
        raise ProbeError(f"atomics: injection {inject!r} is not one of parse_inject's "
                         f"forms") from None
    if mask is not None and not bit & mask:
        raise ProbeError(f"atomics: injection into {name!r}, which is not run")
    if name == "handoff":
        _int(a, 0, MAX_BLOCKS - 1, "injection block")
        _int(b, 0, MAX_ROUNDS - 1, "injection round")
        _int(word, 0, 16 * 1024 - 1, "injection word")
    else:
        _int(a, 0, MAX_BLOCKS * THREADS - 1, "injection thread g")
        _int(b, 0, MAX_ITERS - 1, "injection step s")
    if name != "ticket":
        _int(xor, 1, 0xFFFFFFFF, "injection mask")
    return _native.AtomicsInject(bit, k, a, b, word, xor)


def _geometry(blocks, iters, lo_blocks: int = 1) -> None:
    _int(blocks, lo_blocks, MAX_BLOCKS, "blocks")
    _int(iters, 1, MAX_ITERS, "iters")
    if max(blocks, 1) * THREADS * iters > MAX_OPS:
        raise ProbeError(f"atomics: blocks * 256 * iters must not exceed {MAX_OPS}, got "
                         f"{blocks} * 256 * {iters}")


def _handoff_args(blocks, rounds, lines, budget_us, lo_blocks: int = 1) -> None:
    _int(blocks, lo_blocks, MAX_BLOCKS, "blocks")
    _int(rounds, 1, MAX_ROUNDS, "rounds")
    if lines not in (1, 16) or isinstance(lines, bool):
        raise ProbeError(f"atomics: lines must be 1 or 16, got {lines!r}")
    _int(budget_us, 1, MAX_BUDGET_US, "budget_us")
    if max(blocks, 1) * rounds * (lines * 4096 + 128) > MAX_MAILBOX_BYTES:
        raise ProbeError(f"atomics: {blocks} blocks x {rounds} rounds x {lines} lines need more "
                         f"than 1 GiB of mailboxes")


def widths(blocks: int, iters: int = DEFAULT_ITERS, spread: int = DEFAULT_SPREAD) -> Dict:
    """{kind: {"width", "cap", "max_adds"}}: the table width each kind uses for a requested
    ``spread`` (the smallest power of two >= spread that keeps the float kinds exact and the CAS
    loop's retries few), its cap on the operations into one word (0: none) and the operations
    into its busiest word. Host only."""
    _geometry(blocks, iters), _pow2(spread, MAX_SPREAD, "spread")
    n = len(KINDS)
    w, cap, adds = (C.c_uint32 * n)(), (C.c_uint64 * n)(), (C.c_uint64 * n)()
    _check(_native.probe().gm_probe_atomics_widths(blocks, iters, spread, w, cap, adds),
           "atomics widths")
    return {KINDS[i]: {"width": w[i], "cap": cap[i], "max_adds": adds[i]} for i in range(n)}


def expected(kind, blocks: int, iters: int = DEFAULT_ITERS, spread: int = DEFAULT_SPREAD,
             seed: int = DEFAULT_SEED, width: Optional[int] = None):
    """numpy uint32[W] (uint64[W] for the 8-byte kinds): the final table of ``kind`` as the host
    folds it; ``"ticket"``: the counters' final values N_k; ``"count"``: the operations per word.
    W is ``width`` if given, else the width rule's for ``spread``. A width at which the kind is
    no longer exact in any order is refused. Host only, no GPU."""
    import numpy as np

    k = kind_of(kind)
    if k == KINDS.index("handoff"):
        raise ProbeError("atomics: the hand-off has no table; see payload()")
    _geometry(blocks, iters), _int(seed, 0, (1 << 64) - 1, "seed")
    if width is None:
        _pow2(spread, MAX_SPREAD, "spread")
        width = spread if k >= len(KINDS) else widths(blocks, iters, spread)[KINDS[k]]["width"]
    _pow2(width, MAX_WIDTH, "width")
    out = np.empty(width, dtype=np.uint64 if k < len(KINDS) and KINDS[k] in WIDE else np.uint32)
    rc = _native.probe().gm_probe_atomics_expected(k, blocks, iters, width, seed,
                                                   out.ctypes.data_as(C.c_void_p), out.nbytes)
    if rc == 1:
        cap = widths(blocks, iters, 1)[KINDS[k]]["cap"] if k < len(KINDS) else 0
        raise ProbeError(f"atomics: {kind} is refused at width {width} for {blocks} blocks x "
                         f"{iters} iters (more than {cap} operations into one word)")
    _check(rc, "atomics expected")
    return out


def payload(block: int, round_: int, word: int, seed: int = DEFAULT_SEED) -> int:
    """E(block, round, word): what the hand-off stores there. Host only."""
    _int(block, 0, MAX_BLOCKS - 1, "block"), _int(round_, 0, MAX_ROUNDS - 1, "round")
    _int(word, 0, 16 * 1024 - 1, "word")
    return int(_native.probe().gm_probe_atomics_payload(seed, block, round_, word))


# ------------------------------------------------------------------ per-test calls on tensors
def _stream(stream, device):
    import torch

    return stream if stream is not None else torch.cuda.current_stream(device)


def add(kind, blocks: int, iters: int = DEFAULT_ITERS, width: int = DEFAULT_SPREAD,
        seed: int = DEFAULT_SEED, stream=None, _inject=None):
    """One launch of one kind of the add test on a fresh table on the current device: numpy
    uint32[width] or uint64[width], to be compared with :func:`expected`."""
    import numpy as np
    import torch

    k = kind_of(kind)
    if k >= len(ADD_KINDS):
        raise ProbeError(f"atomics: {kind!r} is not a kind of the add test")
    _geometry(blocks, iters), _pow2(width, MAX_WIDTH, "width")
    wide = KINDS[k] in WIDE
    table = torch.empty(width, dtype=torch.int64 if wide else torch.int32, device="cuda")
    s = _stream(stream, table.device)
    inj = _inject_arg(_inject)
    with torch.cuda.device(table.device):
        _check(_native.probe().gm_probe_atomics_add(
            k, table.data_ptr(), width, blocks, iters, seed,
            C.byref(inj) if inj is not None else None, C.c_void_p(s.cuda_stream)), "atomics add")
    s.synchronize()
    return table.cpu().numpy().view(np.uint64 if wide else np.uint32)


def cas(blocks: int, iters: int = DEFAULT_ITERS, width: int = DEFAULT_SPREAD,
        seed: int = DEFAULT_SEED, stream=None, _inject=None):
    """The CAS test on a fresh table: (numpy uint64[width], {"cas_giveups": n})."""
    import numpy as np
    import torch

    _geometry(blocks, iters), _pow2(width, MAX_WIDTH, "width")
    bounds = torch.from_numpy(expected(COUNT, blocks, iters, width=width).view(np.int32)).cuda()
    table = torch.empty(width, dtype=torch.int64, device="cuda")
    s = _stream(stream, table.device)
    s.wait_stream(torch.cuda.current_stream(table.device))
    inj, res = _inject_arg(_inject), _native.AtomicsResult()
    with torch.cuda.device(table.device):
        _check(_native.probe().gm_probe_atomics_cas(
            table.data_ptr(), bounds.data_ptr(), width, blocks, iters, seed,
            C.byref(inj) if inj is not None else None, C.c_void_p(s.cuda_stream), C.byref(res)),
            "atomics cas")
    return table.cpu().numpy().view(np.uint64), {"cas_giveups": res.cas_giveups}


def ticket(blocks: int, iters: int = DEFAULT_ITERS, counters: int = DEFAULT_SPREAD,
           seed: int = DEFAULT_SEED, stream=None, _inject=None) -> Dict:
    """The ticket test on fresh counters and marks: its counters of the result."""
    import numpy as np
    import torch

    _geometry(blocks, iters), _pow2(counters, MAX_SPREAD, "counters")
    n = expected("ticket", blocks, iters, width=counters, seed=seed)
    off = np.zeros(counters + 1, dtype=np.int64)
    np.cumsum(n, out=off[1:])
    marks = int(off[-1])
    d_off = torch.from_numpy(off).cuda()
    d_ctr = torch.empty(counters, dtype=torch.int32, device="cuda")
    d_marks = torch.empty(marks, dtype=torch.int32, device="cuda")
    s = _stream(stream, d_ctr.device)
    s.wait_stream(torch.cuda.current_stream(d_ctr.device))
    inj, res = _inject_arg(_inject), _native.AtomicsResult()
    with torch.cuda.device(d_ctr.device):
        _check(_native.probe().gm_probe_atomics_ticket(
            d_ctr.data_ptr(), d_off.data_ptr(), d_marks.data_ptr(), marks, counters, blocks,
            iters, seed, C.byref(inj) if inj is not None else None, C.c_void_p(s.cuda_stream),
            C.byref(res)), "atomics ticket")
    return {"tickets": res.tickets, "marks": marks, "holes": res.holes,
            "duplicates": res.duplicates, "counter_errors": res.counter_errors,
            "order_violations": res.order_violations, "out_of_range": res.out_of_range,
            "first_errors": _records(res)}


def handoff(blocks: int, rounds: int = DEFAULT_ROUNDS, lines: int = DEFAULT_LINES,
            budget_us: int = DEFAULT_BUDGET_US, seed: int = DEFAULT_SEED, stream=None,
            _inject=None) -> Dict:
    """The hand-off test on fresh mailboxes: its counters of the result."""
    import torch

    _handoff_args(blocks, rounds, lines, budget_us)
    boxes = blocks * rounds
    d_payload = torch.empty(boxes * lines * 1024, dtype=torch.int32, device="cuda")
    d_flags = torch.empty(boxes * 32, dtype=torch.int32, device="cuda")
    s = _stream(stream, d_payload.device)
    inj, res = _inject_arg(_inject), _native.AtomicsResult()
    with torch.cuda.device(d_payload.device):
        _check(_native.probe().gm_probe_atomics_handoff(
            d_payload.data_ptr(), d_flags.data_ptr(), blocks, rounds, lines, budget_us, seed,
            C.byref(inj) if inj is not None else None, C.c_void_p(s.cuda_stream), C.byref(res)),
            "atomics handoff")
    return _handoff_fields(res)


def _handoff_fields(res) -> Dict:
    return {"handoffs": res.handoffs, "observed": res.observed,
            "observed_cross_xcc": res.observed_cross_xcc, "unseen": res.unseen,
            "stale_words": res.stale_words, "lost_words": res.lost_words,
            "poll_max_us": res.poll_max_us, "poll_mean_us": res.poll_mean_us,
            "pairs_observed": [list(row) for row in res.pairs_observed],
            "pairs_stale": [list(row) for row in res.pairs_stale],
            "first_errors": _records(res)}


def _records(res):
    out = []
    for i in range(res.records_filled):
        r = res.records[i]
        rec = {"test": TEST_NAMES.get(r.test, str(r.test)),
               "kind": KINDS[r.kind] if r.kind < len(KINDS) else str(r.kind),
               "index": r.index, "expected": f"{r.expected:#x}", "got": f"{r.got:#x}",
               "xor": f"{r.expected ^ r.got:#x}"}
        if r.test == TESTS["handoff"]:
            if r.index >> 40:
                rec.update(mailbox=r.index & 0xFFFFFFFF, flag=True)
            else:
                rec.update(mailbox=r.index >> 14, word=r.index & 0x3FFF)
        for name, v in (("xcc_producer", r.xcc_producer), ("xcc_consumer", r.xcc_consumer)):
            if v != _native.ATOMICS_XCC_UNKNOWN:
                rec[name] = v
        out.append(rec)
    return out


def _test_names(mask: int):
    return [n for n in TESTS if TESTS[n] & mask]


def run(dev: int, tests=ALL_TESTS, blocks: int = 0, iters: int = DEFAULT_ITERS,
        spread: int = DEFAULT_SPREAD, rounds: int = DEFAULT_ROUNDS, lines: int = DEFAULT_LINES,
        budget_us: int = DEFAULT_BUDGET_US, seed: int = DEFAULT_SEED, _inject=None) -> Dict:
    """The tests of ``tests`` on device ``dev``; ``blocks`` 0 means one block per CU.
    ``_inject`` is a negative control in one of :func:`parse_inject`'s forms.

    ``ok`` is about data only: every error counter is 0. ``unseen`` hand-offs never change it;
    ``handoff_vacuous`` says that the hand-off ran and not one flag was seen in time, so that it
    proved nothing."""
    mask = mask_of(tests)
    _int(dev, 0, (1 << 31) - 1, "device"), _int(seed, 0, (1 << 64) - 1, "seed")
    _geometry(blocks, iters, 0), _pow2(spread, MAX_SPREAD, "spread")
    _handoff_args(blocks, rounds, lines, budget_us, 0)
    inj = _inject_arg(_inject, mask)
    res = _native.AtomicsResult()
    _check(_native.probe().gm_probe_atomics(
        dev, mask, blocks, iters, spread, rounds, lines, budget_us, seed,
        C.byref(inj) if inj is not None else None, C.byref(res)), "atomics")
    kinds = {}
    for i, name in enumerate(KINDS):
        k = res.kinds[i]
        if k.ops:
            kinds[name] = {"ops": k.ops, "ms": k.ms, "gops": k.gops, "width": k.width,
                           "words_in_error": k.words_in_error}
    out = {"device": dev, "tests": _test_names(res.tests_run), "blocks": res.blocks,
           "iters": res.iters, "spread": res.spread, "rounds": res.rounds, "lines": res.lines,
           "budget_us": res.budget_us, "xccs_seen": res.xccs_seen,
           "xcc_blocks": list(res.xcc_blocks), "kinds": kinds,
           "words_in_error": res.words_in_error, "tickets": res.tickets, "holes": res.holes,
           "duplicates": res.duplicates, "counter_errors": res.counter_errors,
           "order_violations": res.order_violations, "out_of_range": res.out_of_range,
           "cas_giveups": res.cas_giveups, "seconds": res.seconds}
    out.update(_handoff_fields(res))
    out["handoff_vacuous"] = bool(res.tests_run & TESTS["handoff"]) and res.observed == 0
    out["ok"] = all(out[c] == 0 for c in ERROR_COUNTERS)
    return out


def describe_failed(result: Dict) -> str:
    """One line naming what a :func:`run` result found wrong: the nonzero error counters, the
    kinds with wrong words and the first record, for ``doctor``."""
    parts = [f"{c} {result[c]}" for c in ERROR_COUNTERS if result[c]]
    bad = [n for n, k in result["kinds"].items() if k["words_in_error"]]
    if bad:
        parts.append("kinds " + "+".join(bad))
    if result["first_errors"]:
        r = result["first_errors"][0]
        where = (f"mailbox {r['mailbox']} " + ("flag" if r.get("flag") else f"word {r['word']}")
                 if "mailbox" in r else f"index {r['index']}")
        xcc = "".join(f" {n[4:]} xcc {r[n]}" for n in ("xcc_producer", "xcc_consumer") if n in r)
        parts.append(f"first: {r['kind']} {where} expected {r['expected']} got {r['got']}{xcc}")
    return "; ".join(parts)
