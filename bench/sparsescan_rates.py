"""Coverage and time of the sparse and 32x32 matrix-core scan, in one process on one GPU (raw runs
in profiles/sparsescan/README.md). A measuring aid: no test depends on these numbers and none of
them is a threshold.

    python bench/sparsescan_rates.py [--runs 7] [--device 0] [--out rates.json]

First, per format and iters 1 / 3 / 63, how many of one block's 1024 signature words differ from
the host table. Then, after one warm-up scan: ``--runs`` scans at iters 1, 16 and 63 (rounds needed
for full coverage, kernel ms per round, wall seconds of the call and what of it is not kernel: the
host tables), the same per format at the default iters, and the negative control. Numbers from
different processes are not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpumounter_amd.ops import probe, sparsescan  # noqa: E402

KEYS = ("cus_expected", "cus_seen", "complete", "rounds", "blocks_run", "blocks_four_simds",
        "xcc_cus", "kernel_ms", "seconds", "words_in_error", "ok")
ITERS = (1, sparsescan.DEFAULT_ITERS, sparsescan.MAX_ITERS)


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
    out = {"runs": runs, "props": probe.props(dev), "default_iters": sparsescan.DEFAULT_ITERS}

    def dump():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    print(out["props"], flush=True)
    out["signature_words_differing"] = {}
    for fmt in sparsescan.ALL_FORMATS:
        row = {}
        for it in (1, 3, sparsescan.MAX_ITERS):
            sig, _ = sparsescan.signature(fmt, iters=it)
            row[it] = int((sig != sparsescan.expected(fmt, iters=it)).sum())
        out["signature_words_differing"][fmt] = row
        print("signature", fmt, row, flush=True)
    dump()

    sparsescan.scan(dev)                               # warm-up: clocks and the code object
    out["by_iters"] = {}
    for it in ITERS:
        rs = [brief(sparsescan.scan(dev, iters=it)) for _ in range(runs)]
        out["by_iters"][it] = rs
        print("iters", it, "ms per round", [round(r["ms_per_round"], 4) for r in rs],
              "seconds", [round(r["seconds"], 5) for r in rs],
              "rounds", [r["rounds"] for r in rs], "complete", [r["complete"] for r in rs],
              flush=True)
    dump()
    out["per_format"] = {}
    for fmt in sparsescan.ALL_FORMATS:
        rs = [brief(sparsescan.scan(dev, formats=(fmt,))) for _ in range(runs)]
        out["per_format"][fmt] = rs
        print(fmt, "ms per round", [round(r["ms_per_round"], 4) for r in rs], flush=True)
    mid = sparsescan.scan(dev)["per_cu"]
    target = mid[len(mid) // 2]["id"]
    flip = sparsescan.scan(dev, _inject=(target, "bf16-32x32", 130, 2, 0x10000))
    out["flip"] = {"target": target, "failed": flip["failed"], "first_errors": flip["first_errors"],
                   "words_in_error": flip["words_in_error"], "ok": flip["ok"]}
    print("flip", out["flip"], flush=True)
    dump()
    clean = all(r["ok"] for rs in out["by_iters"].values() for r in rs)
    if not clean or flip["ok"]:
        print("a clean scan failed or the negative control passed")
        return 1

    print("SUMMARY")
    for it, rs in out["by_iters"].items():
        print("iters", it, "ms per round", {k: round(v, 4) for k, v in
                                            spread(r["ms_per_round"] for r in rs).items()},
              "call ms", {k: round(v * 1e3, 3) for k, v in spread(r["seconds"] for r in rs).items()},
              "host ms", {k: round(v, 3) for k, v in spread(r["host_ms"] for r in rs).items()},
              "one round reached all CUs", all(r["rounds"] == 1 and r["complete"] for r in rs))
    print("ms per round at the default iters", {
        fmt: round(spread(r["ms_per_round"] for r in rs)["median"], 4)
        for fmt, rs in out["per_format"].items()})
    d = out["by_iters"][sparsescan.DEFAULT_ITERS]
    print("per-XCC CU counts", d[0]["xcc_cus"])
    print("blocks with four distinct SIMDs", [(r["blocks_four_simds"], r["blocks_run"]) for r in d])
    return 0


if __name__ == "__main__":
    sys.exit(main())
