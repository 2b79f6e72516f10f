"""Coverage and time of the CU scan, in one process on one GPU (BASELINE.md "CU scan"; raw runs
in profiles/cuscan/README.md). A measuring aid: no test depends on these numbers.

    python bench/cuscan_rates.py [--runs 5] [--device 0] [--out rates.json]

After one warm-up scan: ``--runs`` scans at the default iters (rounds needed for full coverage,
time per round, per-XCC CU counts, blocks whose four waves reported four distinct SIMDs), the
same per test and at iters 1, 4 and 64, a ``min_rounds=8`` scan for the spread of runs per CU,
and the negative control. Numbers from different processes are not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpumounter_amd.ops import cuscan, probe  # noqa: E402

KEYS = ("cus_expected", "cus_seen", "complete", "rounds", "blocks_run", "blocks_four_simds",
        "xcc_cus", "kernel_ms", "seconds", "words_in_error", "ok")


def brief(r):
    out = {k: r[k] for k in KEYS}
    out["ms_per_round"] = r["kernel_ms"] / r["rounds"]
    runs = [c["runs"] for c in r["per_cu"]]
    out["runs_per_cu"] = [min(runs), max(runs)] if runs else []
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev, runs = args.device, args.runs
    out = {"runs": runs, "props": probe.props(dev), "default_iters": cuscan.DEFAULT_ITERS}

    def dump():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    print(out["props"], flush=True)
    cuscan.scan(dev)                                   # warm-up: clocks and the code object
    out["default"] = [brief(cuscan.scan(dev)) for _ in range(runs)]
    for r in out["default"]:
        print("default", r, flush=True)
    dump()
    out["per_test"] = {}
    for t in cuscan.ALL_TESTS:
        out["per_test"][t] = [brief(cuscan.scan(dev, tests=(t,))) for _ in range(runs)]
        print(t, [round(r["ms_per_round"], 4) for r in out["per_test"][t]], flush=True)
    out["by_iters"] = {}
    for it in (1, 4, 64):
        out["by_iters"][it] = [brief(cuscan.scan(dev, iters=it)) for _ in range(runs)]
        print("iters", it, [round(r["ms_per_round"], 4) for r in out["by_iters"][it]], flush=True)
    out["eight_rounds"] = brief(cuscan.scan(dev, min_rounds=8))
    print("min_rounds=8", out["eight_rounds"], flush=True)
    mid = cuscan.scan(dev)["per_cu"]
    target = mid[len(mid) // 2]["id"]
    flip = cuscan.scan(dev, _inject=(target, "mfma", 130, 2, 0x10000))
    out["flip"] = {"target": target, "failed": flip["failed"], "first_errors": flip["first_errors"],
                   "words_in_error": flip["words_in_error"], "ok": flip["ok"]}
    print("flip", out["flip"], flush=True)
    dump()
    if not all(r["ok"] for r in out["default"]) or flip["ok"]:
        print("a clean scan failed or the negative control passed")
        return 1

    print("SUMMARY")
    d = out["default"]
    print("rounds for full coverage", [r["rounds"] for r in d], "complete",
          [r["complete"] for r in d])
    print("ms per round, median", round(statistics.median(r["ms_per_round"] for r in d), 4),
          "min", round(min(r["ms_per_round"] for r in d), 4),
          "max", round(max(r["ms_per_round"] for r in d), 4))
    print("scan seconds, median", round(statistics.median(r["seconds"] for r in d), 5))
    print("per-XCC CU counts", d[0]["xcc_cus"])
    print("blocks with four distinct SIMDs", [(r["blocks_four_simds"], r["blocks_run"]) for r in d])
    return 0


if __name__ == "__main__":
    sys.exit(main())
