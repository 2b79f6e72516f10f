"""What the attributed burn-in costs and what it reaches: plain and attributed burn-ins of the
three formats (bf16, mxfp8, mxfp4) in one process on one GPU at 8192³, alternating, and the
placement the attributed ones observed (``cus_seen``, ``tiles_moved``). A measuring aid: no test
depends on these numbers (profiles/burnin_attr/README.md).

    python bench/burnin_attr_rates.py [--seconds 4] [--runs 3] [--device 0]
                                      [--out-dir profiles/burnin_attr]

After one warm-up burn-in per format and mode: ``--runs`` rounds of plain, attributed, plain,
attributed ... for ``--seconds`` each (compare kernels included in the rate, as the burn-in
reports it). The mode costs the id store, the per-tile compare and the L2 locality a rotation
gives up. Writes ``rates.json``. Exit 1 only if a burn-in found a mismatch. Numbers from
different processes are not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpumounter_amd.ops import mxgemm, probe  # noqa: E402

N = 8192
MODES = ("plain", "attributed")
PLACEMENT = ("tiles", "grid", "step", "rotations", "cus_seen", "tiles_moved", "tiles_exonerated",
             "events")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out-dir", default=os.path.join("profiles", "burnin_attr"))
    args = ap.parse_args()
    dev = args.device
    os.makedirs(args.out_dir, exist_ok=True)
    out = {"n": N, "seconds": args.seconds, "runs": args.runs, "props": probe.props(dev),
           "traced_kernel_info": {f: probe.traced_kernel_info(f) for f in mxgemm.BURN_IN_FORMATS},
           "burn_in": {f: {m: [] for m in MODES} for f in mxgemm.BURN_IN_FORMATS}}
    print(out["props"], flush=True)

    def dump():
        with open(os.path.join(args.out_dir, "rates.json"), "w") as fh:
            json.dump(out, fh, indent=1)

    def run(fmt, mode, seconds):
        return mxgemm.run_burn_in(dev, seconds, fmt, attribute=mode == "attributed")

    for fmt in mxgemm.BURN_IN_FORMATS:                 # warm-up: clocks and the code objects
        for mode in MODES:
            run(fmt, mode, 1.0)
    for _ in range(args.runs):
        for fmt in mxgemm.BURN_IN_FORMATS:
            for mode in MODES:
                r = run(fmt, mode, args.seconds)
                rec = {k: r[k] for k in ("iterations", "tflops", "mismatches", "ok")}
                if mode == "attributed":
                    rec.update({k: r["attribution"][k] for k in PLACEMENT})
                out["burn_in"][fmt][mode].append(rec)
                print("burn-in", fmt, mode, rec, flush=True)
        dump()
    med = {f: {m: statistics.median(r["tflops"] for r in out["burn_in"][f][m]) for m in MODES}
           for f in mxgemm.BURN_IN_FORMATS}
    out["median_tflops"] = med
    out["attributed_over_plain"] = {f: med[f]["attributed"] / med[f]["plain"] for f in med}
    out["placement"] = {f: {k: [r[k] for r in out["burn_in"][f]["attributed"]]
                            for k in ("cus_seen", "tiles_moved", "tiles_exonerated")}
                        for f in mxgemm.BURN_IN_FORMATS}
    dump()

    print("SUMMARY")
    print("burn-in TF/s, median", {f: {m: round(v, 1) for m, v in ms.items()}
                                   for f, ms in med.items()})
    print("attributed / plain", {f: round(v, 3) for f, v in out["attributed_over_plain"].items()})
    print("placement", out["placement"])
    clean = all(r["ok"] for modes in out["burn_in"].values() for runs in modes.values()
                for r in runs)
    if not clean:
        print("a burn-in found mismatches")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
