"""Cross-XCC atomics and coherence test on the GPU (native/hip/gm_atomics.hip): the ADD and CAS
tables against the host's bit for bit, the ticket audit, the hand-off's bookkeeping, every
negative control with its exact counts, and the command lines. Every call is milliseconds: the
shapes are the smallest that can go wrong (1, 2 and 9 blocks, 9 being no multiple of the 8 XCCs;
one block per CU; once more than one block per CU)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpumounter_amd.ops import atomics, probe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
G, S = 300, 2                       # the injected operation: thread 44 of block 1, its third step


@functools.lru_cache(maxsize=None)
def cu_count():
    return probe.props(0)["cu_count"]


def shapes():
    """(blocks, iters, spread); blocks 0 stands for one block per CU (resolved in the test)."""
    return ((1, 1, 1), (2, 3, 64), (9, 3, 1), (9, 2, 4096), (0, atomics.DEFAULT_ITERS, 4096),
            (0, 3, 64))


@functools.lru_cache(maxsize=None)
def host(kind, blocks, iters, spread):
    """The host's table, computed once per shape and never written to."""
    t = atomics.expected(kind, blocks, iters, spread, SEED)
    t.setflags(write=False)
    return t


def _blocks(blocks):
    return blocks or cu_count()


@pytest.mark.parametrize("blocks,iters,spread", shapes())
@pytest.mark.parametrize("kind", atomics.ADD_KINDS)
def test_add_table_equals_the_host_table(kind, blocks, iters, spread):
    blocks = _blocks(blocks)
    want = host(kind, blocks, iters, spread)
    got = atomics.add(kind, blocks, iters, len(want), SEED)
    assert got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("blocks,iters,spread", shapes())
def test_cas_table_equals_the_host_table(blocks, iters, spread):
    blocks = _blocks(blocks)
    want = host("cas", blocks, iters, spread)          # widened where spread breaks the CAS cap
    got, c = atomics.cas(blocks, iters, len(want), SEED)
    np.testing.assert_array_equal(got, want)
    assert c["cas_giveups"] == 0


def test_add_and_cas_on_a_side_stream():
    s = torch.cuda.Stream()
    for kind in ("add_f32", "xor_u64", "pk_add_bf16"):
        want = host(kind, 9, 3, 64)
        np.testing.assert_array_equal(atomics.add(kind, 9, 3, len(want), SEED, stream=s), want)
    got, c = atomics.cas(9, 3, 64, SEED, stream=s)
    np.testing.assert_array_equal(got, host("cas", 9, 3, 64))
    assert c["cas_giveups"] == 0


@pytest.mark.parametrize("blocks,iters,spread", shapes())
def test_ticket_counters_are_zero_except_tickets(blocks, iters, spread):
    blocks = _blocks(blocks)
    r = atomics.ticket(blocks, iters, spread, SEED)
    print(r)
    assert r["tickets"] == blocks * 256 * iters
    assert r["marks"] == int(host("ticket", blocks, iters, spread).sum(dtype=np.uint64))
    assert r["tickets"] <= r["marks"] <= 4 * r["tickets"]
    for c in ("holes", "duplicates", "counter_errors", "order_violations", "out_of_range"):
        assert r[c] == 0, r
    assert r["first_errors"] == []


def test_ticket_on_a_side_stream_and_its_negative_control():
    s = torch.cuda.Stream()
    r = atomics.ticket(9, 3, 64, SEED, stream=s, _inject=("ticket", G, S))
    assert r["duplicates"] == 1 and r["holes"] == 0 and r["counter_errors"] == 0, r
    (rec,) = r["first_errors"]
    # the mark lies among counter k's: off[k] <= index < off[k + 1], k = a(G, S) mod 64
    off = np.concatenate(([0], np.cumsum(host("ticket", 9, 3, 64), dtype=np.uint64)))
    k = (G + 97 * S) % 64
    assert rec["test"] == "ticket" and int(rec["got"], 16) == 2 and int(rec["expected"], 16) == 1
    assert off[k] <= rec["index"] < off[k + 1], (rec, k)


@pytest.mark.parametrize("kind", ("add_u32", "add_u64", "xor_u64"))
def test_add_negative_control_changes_exactly_one_word(kind):
    want = host(kind, 9, 3, 64)
    got = atomics.add(kind, 9, 3, 64, SEED, _inject=("add", kind, G, S, 0x10000))
    (wrong,) = np.flatnonzero(got != want)
    assert wrong == (G + 97 * S) % 64
    if kind == "xor_u64":
        assert int(got[wrong]) ^ int(want[wrong]) == 0x10000


def test_cas_negative_control_changes_exactly_one_word():
    got, c = atomics.cas(9, 3, 64, SEED, _inject=("cas", G, S, 0x10000))
    (wrong,) = np.flatnonzero(got != host("cas", 9, 3, 64))
    assert wrong == (G + 97 * S) % 64 and c["cas_giveups"] == 0


def _check_handoff(r, handoffs, resident=True):
    """`resident`: the grid is no larger than the CU count, so on the idle test GPU all its blocks
    run at once (a 256-thread block with 8 bytes of LDS per CU), the grid starts within a
    microsecond and a flag stored at agent scope is seen in tens of microseconds at most
    (BASELINE.md), far inside the budget: nothing may be unseen. A flag that only becomes visible
    when its L2 line happens to be written back (a plain store) fails this at the small grids."""
    print({k: r[k] for k in ("handoffs", "observed", "observed_cross_xcc", "unseen",
                             "poll_max_us", "poll_mean_us")})
    assert r["handoffs"] == handoffs and r["observed"] + r["unseen"] == r["handoffs"], r
    if resident:
        assert r["unseen"] == 0, r
    assert r["stale_words"] == 0 and r["lost_words"] == 0 and r["first_errors"] == [], r
    assert sum(map(sum, r["pairs_observed"])) == r["observed"]
    assert sum(map(sum, r["pairs_stale"])) == 0
    assert sum(r["pairs_observed"][i][i] for i in range(16)) == \
        r["observed"] - r["observed_cross_xcc"]
    assert all(v == 0 for row in r["pairs_observed"][8:] for v in row), "an XCC id above 7"
    # an observed poll ended at most one poll step (a sleep and a load) after the budget
    assert 0 <= r["poll_mean_us"] <= r["poll_max_us"] <= atomics.DEFAULT_BUDGET_US + 50


@pytest.mark.parametrize("blocks,rounds,lines", (
    (1, 1, 1), (1, 8, 16), (2, 1, 16), (2, 8, 1), (9, 8, 1), (9, 1, 16), (9, 8, 16), (0, 1, 1)))
def test_handoff_small_grids(blocks, rounds, lines):
    blocks = _blocks(blocks)
    _check_handoff(atomics.handoff(blocks, rounds, lines, seed=SEED), blocks * rounds)


def test_handoff_on_a_side_stream():
    _check_handoff(atomics.handoff(9, 8, 16, seed=SEED, stream=torch.cuda.Stream()), 72)


@pytest.fixture(scope="module")
def clean():
    """One clean default call (one block per CU, 8 rounds, 16 lines), shared by its readers."""
    return atomics.run(0, seed=SEED)


def test_default_call_is_clean_and_its_counters_add_up(clean):
    r = clean
    print({k: r[k] for k in ("blocks", "xccs_seen", "xcc_blocks", "seconds", "poll_max_us")})
    print({n: (k["width"], round(k["gops"], 1)) for n, k in r["kinds"].items()})
    assert r["ok"] and not r["handoff_vacuous"] and r["tests"] == list(atomics.ALL_TESTS), r
    for c in atomics.ERROR_COUNTERS:
        assert r[c] == 0, (c, r[c])
    assert r["blocks"] == cu_count() and sum(r["xcc_blocks"]) == r["blocks"]
    assert r["xccs_seen"] == sum(1 for v in r["xcc_blocks"] if v) >= 1
    assert list(r["kinds"]) == list(atomics.KINDS)
    ops = r["blocks"] * 256 * r["iters"]
    w = atomics.widths(r["blocks"], r["iters"], r["spread"])
    for name, k in r["kinds"].items():
        assert k["words_in_error"] == 0 and k["ms"] > 0 and k["gops"] > 0, (name, k)
        if name == "handoff":
            assert k["ops"] == k["width"] == r["blocks"] * r["rounds"]
        else:
            assert k["ops"] == ops and k["width"] == w[name]["width"], (name, k)
    assert r["tickets"] == ops
    _check_handoff(r, r["blocks"] * r["rounds"])
    if r["xccs_seen"] >= 2:
        assert r["observed_cross_xcc"] >= 1


def test_one_block_per_cu_sees_every_handoff_on_an_idle_gpu(clean):
    """blocks = cu_count, rounds 8: every block is resident, so every flag is seen well within
    the budget (the longest poll of 20 default calls was under 20 us of 200)."""
    assert clean["unseen"] == 0 and clean["observed"] == clean["handoffs"], clean["poll_max_us"]


def test_more_than_one_block_per_cu_ends_and_adds_up():
    blocks = 2 * cu_count() + 3
    r = atomics.run(0, blocks=blocks, iters=3, spread=64, rounds=8, lines=1, seed=SEED)
    assert r["ok"] and r["blocks"] == blocks and sum(r["xcc_blocks"]) == blocks, r
    _check_handoff(r, blocks * 8, resident=False)
    assert r["cas_giveups"] == 0 and r["tickets"] == blocks * 256 * 3


@pytest.mark.parametrize("spread", (1, 64))
def test_hot_words(spread):
    """One word for the whole chip, and one wave-instruction's worth."""
    r = atomics.run(0, tests=("add", "ticket", "cas"), iters=3, spread=spread, seed=SEED)
    assert r["ok"] and r["cas_giveups"] == 0 and r["tests"] == ["add", "ticket", "cas"], r
    w = atomics.widths(r["blocks"], 3, spread)
    assert r["kinds"]["pk_add_bf16"]["width"] == w["pk_add_bf16"]["width"] > spread
    assert r["kinds"]["add_f32"]["width"] == spread < r["kinds"]["cas"]["width"]


def _only(r, **nonzero):
    for c in atomics.ERROR_COUNTERS:
        assert r[c] == nonzero.get(c, 0), (c, r[c], r["first_errors"])
    assert not r["ok"]


@pytest.mark.parametrize("kind", ("add_u32", "add_u64", "xor_u64"))
def test_run_add_injection_is_one_wrong_word_of_that_kind(kind):
    r = atomics.run(0, tests=("add",), seed=SEED, _inject=("add", kind, G, S, 0x10000))
    _only(r, words_in_error=1)
    assert [n for n, k in r["kinds"].items() if k["words_in_error"]] == [kind]
    (rec,) = r["first_errors"]
    assert rec["test"] == "add" and rec["kind"] == kind
    assert rec["index"] == (G + 97 * S) % r["kinds"][kind]["width"]
    assert int(rec["expected"], 16) == int(host(kind, r["blocks"], r["iters"],
                                                r["spread"])[rec["index"]])
    assert kind in atomics.describe_failed(r)


def test_run_cas_injection():
    r = atomics.run(0, tests=("cas",), seed=SEED, _inject=("cas", G, S, 0x10000))
    _only(r, words_in_error=1)
    (rec,) = r["first_errors"]
    assert rec["kind"] == "cas" and rec["index"] == (G + 97 * S) % r["kinds"]["cas"]["width"]
    assert r["kinds"]["cas"]["words_in_error"] == 1


def test_run_ticket_injection():
    r = atomics.run(0, tests=("ticket",), seed=SEED, _inject=("ticket", G, S))
    _only(r, duplicates=1)
    (rec,) = r["first_errors"]
    assert rec["kind"] == "ticket" and int(rec["got"], 16) == 2


def test_run_handoff_injection(clean):
    block, rnd, word, mask = 3, 2, 1500, 0x100
    r = atomics.run(0, tests=("handoff",), seed=SEED, _inject=("handoff", block, rnd, word, mask))
    # this grid is fully resident (the clean call saw every hand-off), so this one was observed
    assert r["observed"] == r["handoffs"]
    _only(r, lost_words=1, stale_words=1)
    assert sum(map(sum, r["pairs_stale"])) == 1
    assert len(r["first_errors"]) == 2
    e = atomics.payload(block, rnd, word, SEED)
    for rec in r["first_errors"]:
        assert rec["mailbox"] == block * r["rounds"] + rnd and rec["word"] == word
        assert int(rec["expected"], 16) == e and int(rec["got"], 16) == e ^ mask
        assert rec["xcc_producer"] < 8
    (seen,) = [rec for rec in r["first_errors"] if "xcc_consumer" in rec]
    assert r["pairs_stale"][seen["xcc_producer"]][seen["xcc_consumer"]] == 1
    assert "mailbox 26 word 1500" in atomics.describe_failed(r)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=120)


def test_probe_cli_atomics():
    res = _cli("probe", "--atomics")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["atomics"]["ok"] and r["atomics"]["blocks"] == cu_count() for r in out)


@pytest.mark.parametrize("inject,counter", (
    ("add:add_f64:300:2:0x3", "words_in_error"), ("cas:300:2:0x10", "words_in_error"),
    ("ticket:300:2", "duplicates"), ("handoff:3:2:1500:0x100", "lost_words")))
def test_probe_cli_atomics_inject_fails(inject, counter):
    res = _cli("probe", "--atomics", "--atomics-tests", inject.split(":")[0], "--atomics-spread",
               "64", "--atomics-rounds", "3", "--atomics-inject", inject)
    assert res.returncode == 1, (res.stdout[-2000:], res.stderr[-2000:])
    for r in json.loads(res.stdout):
        assert not r["atomics"]["ok"] and r["atomics"][counter] == 1, r["atomics"]


def test_doctor_reports_clean_and_injected():
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    # the real amdsmi, as tests/test_gpu.py uses it: the mock's symbols, once loaded into this
    # process, would serve every later inventory of the session
    cfg = Config.load(env={})
    clean = [c for c in doctor.check_gpus(cfg, atomics=True) if c.name != "gpu"]
    assert clean and all(c.status in ("ok", "warn") and " 0 wrong words" in c.detail
                         and "proved nothing" not in c.detail for c in clean), clean
    bad = [c for c in doctor.check_gpus(cfg, atomics=True, atomics_inject=("ticket", G, S))
           if c.name != "gpu"]
    assert bad and all(c.status == "fail" and "failed: duplicates 1" in c.detail
                       for c in bad), bad


def test_validate_reports_clean_and_injected(monkeypatch, capsys):
    """validate's atomics step on the GPU; the all-reduce before it, which starts a process per
    GPU, is not what this test is about and is stubbed."""
    from gpumounter_amd.parallel import validate

    monkeypatch.setattr(validate, "run_allreduce", lambda world, cpu, numel: [
        {"ok": True, "ms": 1.0, "busbw_gbps": 1.0, "bytes": 2 * numel}])
    assert validate.main(["--no-p2p", "--atomics"]) == 0
    rep = json.loads(capsys.readouterr().out)
    assert rep["ok"] and all(a["ok"] and a["observed"] for a in rep["atomics"])
    assert validate.main(["--no-p2p", "--atomics", "--atomics-inject", "cas:300:2:0x10"]) == 1
    rep = json.loads(capsys.readouterr().out)
    assert not rep["ok"] and all(a["words_in_error"] == 1 for a in rep["atomics"])
