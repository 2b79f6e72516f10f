"""Host-GPU atomics and hand-off test on the GPU (native/hip/gm_hostsync.hip): the ADD and CAS
tables against the host's bit for bit with host threads contending, the ticket and swap audits,
the hand-off's bookkeeping in both directions, every negative control with its exact counts, and
the command lines. Every call is milliseconds: the shapes are the smallest that can go wrong (the
GPU alone on one hot word; one block against one host thread on one word; 9 blocks, which is no
multiple of the 8 XCCs nor of 2 or 3 threads). No test asserts a time.

Where the device reports no native host atomics over its link (``atomics_supported`` false) the
table, ticket, swap and cas tests skip with that reason, and one test asserts that the driver
skipped the four and still ran the hand-off."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpumounter_amd.ops import hostsync, probe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
G, S = 300, 2                       # the injected operation: thread 44 of block 1, its third step
# (blocks, host_threads, iters, spread)
SHAPES = ((1, 0, 1, 1), (1, 1, 1, 1), (2, 1, 3, 64), (9, 3, 3, 1), (9, 2, 2, 4096))
# (blocks, host_threads, rounds, lines)
HANDOFFS = ((1, 1, 1, 1), (2, 1, 3, 16), (9, 2, 3, 1))


@functools.lru_cache(maxsize=None)
def supported():
    return hostsync.atomics_supported(0)


def needs_atomics():
    if not supported():
        pytest.skip(hostsync.NO_ATOMICS)


@functools.lru_cache(maxsize=None)
def host(kind, blocks, threads, iters, spread):
    """The host's table, computed once per shape and never written to."""
    t = hostsync.expected(kind, blocks, threads, iters, spread, SEED)
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("blocks,threads,iters,spread", SHAPES)
@pytest.mark.parametrize("kind", hostsync.ADD_KINDS)
def test_add_table_equals_the_host_table(kind, blocks, threads, iters, spread):
    needs_atomics()
    want = host(kind, blocks, threads, iters, spread)
    got = hostsync.add(kind, blocks, threads, iters, spread, SEED)
    assert got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("blocks,threads,iters,spread", SHAPES)
def test_cas_table_equals_the_host_table(blocks, threads, iters, spread):
    needs_atomics()
    want = host("cas", blocks, threads, iters, spread)
    assert len(want) == hostsync.cas_width(blocks, threads, iters, spread) >= spread
    got, c = hostsync.cas(blocks, threads, iters, len(want), SEED)
    np.testing.assert_array_equal(got, want)
    assert c["cas_giveups"] == 0


@pytest.mark.parametrize("blocks,threads,iters,spread", SHAPES)
def test_ticket_and_swap_audits_are_clean(blocks, threads, iters, spread):
    needs_atomics()
    ops = (blocks + threads) * 256 * iters
    t = hostsync.ticket(blocks, threads, iters, spread, SEED)
    print("ticket", t)
    assert t["tickets"] == ops
    assert (t["holes"], t["duplicates"], t["counter_errors"], t["out_of_range"]) == (0, 0, 0, 0)
    assert t["first_errors"] == []
    s = hostsync.swap(blocks, threads, iters, spread, SEED)
    print("swap", s)
    assert s["swaps"] == ops
    assert (s["swap_missing"], s["swap_duplicates"], s["swap_foreign"]) == (0, 0, 0)
    assert s["first_errors"] == []


def _check_handoff(r, handoffs, budget_us=hostsync.DEFAULT_BUDGET_US,
                   host_budget_us=hostsync.DEFAULT_HOST_BUDGET_US):
    print({k: r[k] for k in ("h2d", "d2h", "rtt_median_us", "rtt_max_us", "lost_words")})
    for d, budget in (("h2d", budget_us), ("d2h", host_budget_us)):
        assert r[d]["handoffs"] == handoffs
        assert r[d]["observed"] + r[d]["unseen"] == handoffs
        assert r[d]["stale_words"] == 0
        assert 0 <= r[d]["poll_max_us"] <= budget
    assert r["stale_words_h2d"] == r["stale_words_d2h"] == r["lost_words"] == 0
    assert r["first_errors"] == []


@pytest.mark.parametrize("blocks,threads,rounds,lines", HANDOFFS)
def test_handoff_small_grids(blocks, threads, rounds, lines):
    _check_handoff(hostsync.handoff(blocks, threads, rounds, lines, seed=SEED), blocks * rounds)


@pytest.fixture(scope="module")
def clean():
    """One clean default call (min(16, CUs) blocks, 2 host threads), shared by its readers."""
    return hostsync.run(0, seed=SEED)


def test_default_call_is_clean_and_its_counters_add_up(clean):
    r = clean
    print(json.dumps({k: v for k, v in r.items() if k != "first_errors"}))
    assert r["ok"], r
    for c in hostsync.ERROR_COUNTERS:
        assert r[c] == 0, (c, r[c])
    assert r["blocks"] == min(16, probe.props(0)["cu_count"]) and r["host_threads"] == 2
    assert sorted(r["tests"] + list(r["tests_skipped"])) == sorted(hostsync.ALL_TESTS)
    assert "handoff" in r["tests"]
    _check_handoff(r, r["blocks"] * hostsync.DEFAULT_ROUNDS)
    if r["atomics_supported"]:
        ops = (r["blocks"] + 2) * 256 * hostsync.DEFAULT_ITERS
        assert r["tests"] == list(hostsync.ALL_TESTS) and r["tests_skipped"] == {}
        assert r["tickets"] == r["swaps"] == ops
        assert r["cas_width"] == hostsync.cas_width(r["blocks"], 2)
        assert 0 <= r["host_ops_in_flight"] <= 5 * 2 * 256 * hostsync.DEFAULT_ITERS


def test_default_call_observes_a_handoff_in_each_direction(clean):
    """On an idle GPU the default budgets must let both sides see flags: otherwise the hand-off
    proved nothing, and that is a finding."""
    assert not clean["handoff_vacuous"], (clean["h2d"], clean["d2h"])
    assert clean["h2d"]["observed"] >= 1 and clean["d2h"]["observed"] >= 1


def test_without_native_atomics_the_four_are_skipped_and_the_handoff_runs(clean):
    if clean["atomics_supported"]:
        assert supported() and clean["tests_skipped"] == {}
        return
    assert not supported()
    assert list(clean["tests_skipped"]) == list(hostsync.ATOMIC_TESTS)
    assert set(clean["tests_skipped"].values()) == {hostsync.NO_ATOMICS}
    assert clean["tests"] == ["handoff"] and clean["ok"]
    assert clean["tickets"] == clean["swaps"] == 0


# ---- negative controls, each once, on a side stream, with exact counts
@pytest.mark.parametrize("kind,g", (("add_u32", G), ("add_u64", 9 * 256 + G)))
def test_add_negative_control_changes_exactly_one_word(kind, g):
    """The second aims at a host-played thread: g >= 256 * blocks."""
    needs_atomics()
    want = host(kind, 9, 3, 3, 64)
    got = hostsync.add(kind, 9, 3, 3, 64, SEED, stream=torch.cuda.Stream(),
                       _inject=("add", kind, g, S, 0x10000))
    (wrong,) = np.flatnonzero(got != want)
    assert wrong == (g + 97 * S) % 64
    assert (int(got[wrong]) - int(want[wrong])) % (1 << 32) in (0x10000, (1 << 32) - 0x10000)


def test_cas_negative_control_changes_exactly_one_word():
    needs_atomics()
    want = host("cas", 9, 3, 3, 64)
    got, c = hostsync.cas(9, 3, 3, len(want), SEED, stream=torch.cuda.Stream(),
                          _inject=("cas", G, S, 0x10000))
    (wrong,) = np.flatnonzero(got != want)
    assert wrong == (G + 97 * S) % len(want) and c["cas_giveups"] == 0


def test_ticket_negative_control_is_one_duplicate():
    needs_atomics()
    r = hostsync.ticket(9, 3, 3, 64, SEED, stream=torch.cuda.Stream(), _inject=("ticket", G, S))
    assert (r["duplicates"], r["holes"], r["counter_errors"], r["out_of_range"]) == (1, 0, 0, 0), r
    (rec,) = r["first_errors"]
    off = np.concatenate(([0], np.cumsum(host("ticket", 9, 3, 3, 64), dtype=np.uint64)))
    k = (G + 97 * S) % 64
    assert off[k] <= rec["index"] < off[k + 1] and rec["got"] == "0x2"


@pytest.mark.parametrize("g", (G, 9 * 256 + 7))
def test_swap_negative_control_is_one_missing_and_one_foreign(g):
    """0x10 turns s = 2 into s = 18 >= iters: no token of any word. Once on the GPU, once on a
    host-played thread."""
    needs_atomics()
    r = hostsync.swap(9, 3, 3, 64, SEED, stream=torch.cuda.Stream(),
                      _inject=("swap", g, S, 0x10))
    assert (r["swap_missing"], r["swap_foreign"], r["swap_duplicates"]) == (1, 1, 0), r
    (rec,) = r["first_errors"]
    assert rec["index"] == (g + 97 * S) % 64
    assert int(rec["got"], 16) == (1 + 1024 * g + S) ^ 0x10


@pytest.mark.parametrize("direction", hostsync.DIRECTIONS)
def test_handoff_negative_control_is_one_stale_word_in_that_direction(direction):
    r = hostsync.handoff(2, 1, 3, 16, seed=SEED, stream=torch.cuda.Stream(),
                         _inject=("handoff", direction, 1, 2, 1500, 0x100))
    print(r)
    other = "d2h" if direction == "h2d" else "h2d"
    assert r["lost_words"] == 1 and r[f"stale_words_{other}"] == 0
    # the consumer sees it unless it missed that very flag, which an idle GPU does not
    assert r[f"stale_words_{direction}"] == 1
    recs = [x for x in r["first_errors"] if x["direction"] == direction]
    assert len(recs) == len(r["first_errors"]) == 2
    assert sorted(x["found"] for x in recs) == ["audit", "consumer"]
    for x in recs:
        assert (x["block"], x["round"], x["word"], x["xor"]) == (1, 2, 1500, "0x100")
        d = hostsync.DIRECTIONS.index(direction)
        assert int(x["expected"], 16) == hostsync.payload(d, 1, 2, 1500, SEED)


def test_run_injection_names_the_test_and_fails(clean):
    inj = ("swap", G, S, 0x10) if clean["atomics_supported"] else \
        ("handoff", "d2h", 1, 2, 1500, 0x100)
    r = hostsync.run(0, seed=SEED, _inject=inj)
    assert not r["ok"]
    bad = {c: r[c] for c in hostsync.ERROR_COUNTERS if r[c]}
    if inj[0] == "swap":
        assert bad == {"swap_missing": 1, "swap_foreign": 1}
        assert "first: swap index" in hostsync.describe_failed(r)
    else:
        assert bad == {"stale_words_d2h": 1, "lost_words": 1}
        assert "first: handoff d2h block 1 round 2 word 1500" in hostsync.describe_failed(r)


# ---- the command lines
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=120)


def test_probe_cli_host_sync():
    res = _cli("probe", "--host-sync")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["hostsync"]["ok"] and r["hostsync"]["host_threads"] == 2 for r in out)


def test_probe_cli_negative_control_exits_1():
    inject = "swap:300:2:0x10" if supported() else "handoff:d2h:1:2:1500:0x100"
    res = _cli("probe", "--host-sync", "--host-sync-inject", inject)
    assert res.returncode == 1, (res.returncode, res.stderr[-2000:])
    out = json.loads(res.stdout)
    assert not out[0]["hostsync"]["ok"]
