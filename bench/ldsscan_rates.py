"""Coverage and time of the LDS scan, in one process on one GPU (raw runs in
profiles/ldsscan/README.md). A measuring aid: no test depends on these numbers and none of them
is a threshold.

    python bench/ldsscan_rates.py [--runs 7] [--device 0] [--out rates.json]

First, per test and iters 1 / 2 / 63, how many of one block's 1024 signature words differ from the
host table, and the kernel's register and scratch figures. Then, after one warm-up scan: ``--runs``
scans at iters 1, 2, 4, 8 and 63 (rounds needed for full coverage, kernel ms per round, wall
seconds of the call and what of it is not kernel: the host tables), the same per test at iters 1
and the default, and the two negative controls. The default iters is the largest power of two at
which a round takes no longer than the slowest other scan's default round. Numbers from different
processes are not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpumounter_amd.ops import ldsscan, probe  # noqa: E402

KEYS = ("cus_expected", "cus_seen", "complete", "rounds", "blocks_run", "blocks_four_simds",
        "xcc_cus", "kernel_ms", "seconds", "words_in_error", "ok")
ITERS = (1, 2, 4, 8, ldsscan.MAX_ITERS)


def brief(r):
    out = {k: r[k] for k in KEYS}
    out["ms_per_round"] = r["kernel_ms"] / r["rounds"]
    out["host_ms"] = r["seconds"] * 1e3 - r["kernel_ms"]
    return out


def spread(xs):
    xs = sorted(xs)
    return {"median": statistics.median(xs), "min": xs[0], "max": xs[-1]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev, runs = args.device, args.runs
    out = {"runs": runs, "props": probe.props(dev), "default_iters": ldsscan.DEFAULT_ITERS,
           "geometry": ldsscan.geometry()}

    def dump():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    print(out["props"], flush=True)
    out["kernel_info"] = ldsscan.kernel_info()
    print("kernel", out["kernel_info"], "geometry", out["geometry"], flush=True)
    out["signature_words_differing"] = {}
    for test in ldsscan.ALL_TESTS:
        row = {}
        for it in (1, 2, ldsscan.MAX_ITERS):
            sig, _ = ldsscan.signature(test, iters=it)
            row[it] = int((sig != ldsscan.expected(test, iters=it)).sum())
        out["signature_words_differing"][test] = row
        print("signature", test, row, flush=True)
    dump()

    ldsscan.scan(dev)                                  # warm-up: clocks and the code object
    out["by_iters"] = {}
    for it in ITERS:
        rs = [brief(ldsscan.scan(dev, iters=it)) for _ in range(runs)]
        out["by_iters"][it] = rs
        print("iters", it, "ms per round", [round(r["ms_per_round"], 4) for r in rs],
              "seconds", [round(r["seconds"], 5) for r in rs],
              "rounds", [r["rounds"] for r in rs], "complete", [r["complete"] for r in rs],
              flush=True)
    dump()
    out["per_test"] = {}
    for test in ldsscan.ALL_TESTS:
        out["per_test"][test] = {}
        for it in sorted({1, ldsscan.DEFAULT_ITERS}):
            rs = [brief(ldsscan.scan(dev, tests=(test,), iters=it)) for _ in range(runs)]
            out["per_test"][test][it] = rs
            print(test, "iters", it, "ms per round", [round(r["ms_per_round"], 4) for r in rs],
                  flush=True)
    mid = ldsscan.scan(dev)["per_cu"]
    target = mid[len(mid) // 2]["id"]
    flip = ldsscan.scan(dev, _inject=(target, "atomic", 130, 2, 0x10000))
    out["flip"] = {"target": target, "failed": flip["failed"], "first_errors": flip["first_errors"],
                   "words_in_error": flip["words_in_error"], "ok": flip["ok"]}
    print("flip", out["flip"], flush=True)
    poke = ldsscan.scan(dev, _poke=("tr16", 4099, 0x10))
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
    d = out["by_iters"][ldsscan.DEFAULT_ITERS]
    print("per-XCC CU counts", d[0]["xcc_cus"])
    print("blocks with four distinct SIMDs", [(r["blocks_four_simds"], r["blocks_run"]) for r in d])
    return 0


if __name__ == "__main__":
    sys.exit(main())
