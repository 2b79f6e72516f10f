"""Coverage, time and residency evidence of the cache scan, in one process on one GPU (BASELINE.md
"Cache scan"; raw runs in profiles/cachescan/README.md). A measuring aid: no test depends on these
numbers and none of them is a threshold.

    python bench/cachescan_rates.py [--runs 7] [--device 0] [--out rates.json]

First, per test and iters 1 / 2 / 63, how many of one block's 1024 signature words differ from the
host table, and the kernel's register, scratch and icache-body figures. Then, after one warm-up
scan: ``--runs`` scans at the default iters (rounds needed for full coverage, kernel ms per round,
wall seconds of the call and what of it is not kernel: the host tables), the same at iters 1 and
63 and per test, the timing table (shader-clock counts of each test's first and last pass, with the
counts per load they imply), and the two negative controls. Numbers from different processes are
not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpumounter_amd.ops import cachescan, probe  # noqa: E402

KEYS = ("cus_expected", "cus_seen", "complete", "rounds", "blocks_run", "blocks_four_simds",
        "xcc_cus", "kernel_ms", "seconds", "words_in_error", "ok", "timing")
# what a thread issues in one timed pass: (load instructions, what they are)
PASS_LOADS = {"l2": (80, "64 32-bit sc1 + 16 128-bit nt loads of a round, independent"),
              "l1": (16, "16 plain loads of a hit pass, independent"),
              "scalar": (64, "64 dependent scalar loads"),
              "icache": (0, "no data loads: 3072 steps of straight-line code")}


def brief(r):
    out = {k: r[k] for k in KEYS}
    out["ms_per_round"] = r["kernel_ms"] / r["rounds"]
    out["host_ms"] = r["seconds"] * 1e3 - r["kernel_ms"]
    return out


def spread(xs):
    xs = sorted(xs)
    return {"median": statistics.median(xs), "min": xs[0], "max": xs[-1]}


def timing_rows(timing):
    rows = []
    for test in cachescan.ALL_TESTS:
        if test not in timing:
            continue
        loads, what = PASS_LOADS[test]
        for which in ("first", "last"):
            c = timing[test][which]
            per = round(c["median"] / loads, 1) if loads else None
            rows.append((test, which, c["min"], c["median"], c["max"], per, what))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev, runs = args.device, args.runs
    out = {"runs": runs, "props": probe.props(dev), "default_iters": cachescan.DEFAULT_ITERS,
           "geometry": cachescan.geometry()}

    def dump():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    print(out["props"], flush=True)
    out["kernel_info"] = cachescan.kernel_info()
    print("kernel", out["kernel_info"], "geometry", out["geometry"], flush=True)
    out["signature_words_differing"] = {}
    for test in cachescan.ALL_TESTS:
        row = {}
        for it in (1, 2, cachescan.MAX_ITERS):
            sig, _ = cachescan.signature(test, iters=it)
            row[it] = int((sig != cachescan.expected(test, iters=it)).sum())
        out["signature_words_differing"][test] = row
        print("signature", test, row, flush=True)
    dump()

    cachescan.scan(dev)                                # warm-up: clocks and the code object
    out["by_iters"] = {}
    for it in (cachescan.DEFAULT_ITERS, 1, cachescan.MAX_ITERS):
        rs = [brief(cachescan.scan(dev, iters=it)) for _ in range(runs)]
        out["by_iters"][it] = rs
        print("iters", it, "ms per round", [round(r["ms_per_round"], 4) for r in rs],
              "seconds", [round(r["seconds"], 5) for r in rs],
              "rounds", [r["rounds"] for r in rs], "complete", [r["complete"] for r in rs],
              flush=True)
    dump()
    out["per_test"] = {}
    for test in cachescan.ALL_TESTS:
        out["per_test"][test] = {}
        for it in (1, cachescan.DEFAULT_ITERS, cachescan.MAX_ITERS):
            rs = [brief(cachescan.scan(dev, tests=(test,), iters=it)) for _ in range(runs)]
            out["per_test"][test][it] = rs
            print(test, "iters", it, "ms per round", [round(r["ms_per_round"], 4) for r in rs],
                  flush=True)
    mid = cachescan.scan(dev)["per_cu"]
    target = mid[len(mid) // 2]["id"]
    flip = cachescan.scan(dev, _inject=(target, "l2", 130, 2, 0x10000))
    out["flip"] = {"target": target, "failed": flip["failed"], "first_errors": flip["first_errors"],
                   "words_in_error": flip["words_in_error"], "ok": flip["ok"]}
    print("flip", out["flip"], flush=True)
    poke = cachescan.scan(dev, _poke=("l1", 4099, 0x10))
    out["poke"] = {"failed_cus": poke["failed_cus"], "cus_seen": poke["cus_seen"],
                   "tests_failed": sorted({t for f in poke["failed"] for t in f["tests_failed"]}),
                   "first_errors": poke["first_errors"][:4],
                   "words_in_error": poke["words_in_error"], "ok": poke["ok"]}
    print("poke", out["poke"], flush=True)
    dump()
    clean = all(r["ok"] for rs in out["by_iters"].values() for r in rs)
    if not clean or flip["ok"] or poke["ok"]:
        print("a clean scan failed or a negative control passed")
        return 1

    print("SUMMARY")
    for it, rs in out["by_iters"].items():
        print("iters", it, "ms per round", {k: round(v, 4) for k, v in
                                            spread(r["ms_per_round"] for r in rs).items()},
              "call ms", {k: round(v * 1e3, 3) for k, v in spread(r["seconds"] for r in rs).items()},
              "host ms", {k: round(v, 3) for k, v in spread(r["host_ms"] for r in rs).items()},
              "one round reached all CUs", all(r["rounds"] == 1 and r["complete"] for r in rs))
    for test, by in out["per_test"].items():
        print(test, "ms per round at iters", {it: round(spread(r["ms_per_round"] for r in rs)["median"], 4)
                                              for it, rs in by.items()})
    print("TIMING: shader-clock counts over the blocks of the last round (min, median, max), and the "
          "median per load instruction of the pass")
    for label, r in (("all tests, default iters", out["by_iters"][cachescan.DEFAULT_ITERS][-1]),
                     ("all tests, iters 63", out["by_iters"][cachescan.MAX_ITERS][-1])):
        print(label)
        for row in timing_rows(r["timing"]):
            print("  %-7s %-5s %8d %8d %8d  per load %-8s %s" % row)
    print("each test alone, iters 63")
    for test in cachescan.ALL_TESTS:
        for row in timing_rows(out["per_test"][test][cachescan.MAX_ITERS][-1]["timing"]):
            print("  %-7s %-5s %8d %8d %8d  per load %-8s %s" % row)
    d = out["by_iters"][cachescan.DEFAULT_ITERS]
    print("per-XCC CU counts", d[0]["xcc_cus"])
    print("blocks with four distinct SIMDs", [(r["blocks_four_simds"], r["blocks_run"]) for r in d])
    return 0


if __name__ == "__main__":
    sys.exit(main())
