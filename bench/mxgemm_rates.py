"""Sustained rates of the three burn-ins (bf16, mxfp8, mxfp4) and of their GEMMs alone, in one
process on one GPU at 8192³, next to the register-resident ceilings on record
(profiles/r3_mx/sweep.json); and the MX GEMM's error on random operands against its bound. A
measuring aid: no test depends on these numbers (profiles/mxgemm/README.md).

    python bench/mxgemm_rates.py [--seconds 4] [--runs 3] [--device 0] [--out-dir profiles/mxgemm]

After one warm-up burn-in per format: ``--runs`` rounds of the three burn-ins for ``--seconds``
each, alternating the formats (compare kernels included in the rate, as the burn-in reports it);
then each GEMM alone, 20 back-to-back launches between two events after a warm-up of 5. Writes
``rates.json`` and ``numerics.json``. One condition is checked (exit 1 otherwise): the mxfp8
burn-in's sustained TF/s is at least the bf16 burn-in's of the same run. With the same bytes per
K-tile and twice the K per byte, anything lower would load the chip less than the bf16 burn-in
does. Numbers from different processes are not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from gpumounter_amd.ops import mxgemm, probe  # noqa: E402

N = 8192
CEILING_TFLOPS = {"mxfp8": 5025.0, "mxfp4": 9547.0}     # profiles/r3_mx/sweep.json, best forms
NUMERICS_SHAPE = (512, 512, 8)                          # M, N, K-tiles: the GPU test's


def gemm_only_tflops(fmt: str, iters: int = 20, warmup: int = 5) -> float:
    import torch

    a, sa = mxgemm.fill(fmt, "random", 0x5151, N, N)
    bt, sb = mxgemm.fill(fmt, "random", 0xA3A3, N, N)
    c = torch.empty((N, N), dtype=torch.bfloat16, device=a.device)
    for _ in range(warmup):
        mxgemm.gemm_nt(fmt, a, sa, bt, sb, out=c)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        mxgemm.gemm_nt(fmt, a, sa, bt, sb, out=c)
    t1.record()
    t1.synchronize()
    return 2.0 * N ** 3 * iters / (t0.elapsed_time(t1) * 1e-3) / 1e12


def numerics(fmt: str) -> dict:
    m, n, tiles = NUMERICS_SHAPE
    k = tiles * mxgemm.TILE_K[fmt]
    a, sa = mxgemm.fill(fmt, "random", 0x5151, m, k)
    bt, sb = mxgemm.fill(fmt, "random", 0xA3A3, n, k)
    c = mxgemm.gemm_nt(fmt, a, sa, bt, sb).float().cpu().numpy().astype(np.float64)
    ref, s = mxgemm.expected(fmt, "random", 0x5151, 0xA3A3, m, n, k)
    err = np.abs(c - ref)
    return {"m": m, "n": n, "k": k, "bound": "2^-9 * S + 2^-8 * |ref|",
            "max_error_over_bound": float(np.max(err / (2.0 ** -9 * s + 2.0 ** -8 * np.abs(ref)))),
            "max_error_over_abs_sum": float(np.max(err / s))}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out-dir", default=os.path.join("profiles", "mxgemm"))
    args = ap.parse_args()
    dev = args.device
    os.makedirs(args.out_dir, exist_ok=True)
    import torch

    torch.cuda.set_device(dev)
    out = {"n": N, "seconds": args.seconds, "runs": args.runs, "props": probe.props(dev),
           "kernel_info": {f: mxgemm.kernel_info(f) for f in mxgemm.FORMATS},
           "ceiling_tflops": CEILING_TFLOPS, "burn_in": {f: [] for f in mxgemm.BURN_IN_FORMATS}}
    print(out["props"], flush=True)

    def dump(name, what):
        with open(os.path.join(args.out_dir, name), "w") as fh:
            json.dump(what, fh, indent=1)

    num = {f: numerics(f) for f in mxgemm.FORMATS}
    print("numerics", num, flush=True)
    dump("numerics.json", num)
    for fmt in mxgemm.BURN_IN_FORMATS:                 # warm-up: clocks and the code objects
        mxgemm.run_burn_in(dev, 1.0, fmt)
    for _ in range(args.runs):
        for fmt in mxgemm.BURN_IN_FORMATS:
            r = mxgemm.run_burn_in(dev, args.seconds, fmt)
            out["burn_in"][fmt].append({k: r[k] for k in ("iterations", "tflops", "mismatches",
                                                          "ok")})
            print("burn-in", fmt, out["burn_in"][fmt][-1], flush=True)
        dump("rates.json", out)
    out["gemm_only_tflops"] = {"bf16": [probe.gemm_tflops(dev, N, N, N, 20)
                                        for _ in range(args.runs)]}
    for fmt in mxgemm.FORMATS:
        out["gemm_only_tflops"][fmt] = [gemm_only_tflops(fmt) for _ in range(args.runs)]
    med = {f: statistics.median(r["tflops"] for r in out["burn_in"][f])
           for f in mxgemm.BURN_IN_FORMATS}
    out["burn_in_median_tflops"] = med
    out["gemm_only_median_tflops"] = {f: statistics.median(v)
                                      for f, v in out["gemm_only_tflops"].items()}
    out["fraction_of_ceiling"] = {
        f: {"burn_in": med[f] / CEILING_TFLOPS[f],
            "gemm_only": out["gemm_only_median_tflops"][f] / CEILING_TFLOPS[f]}
        for f in mxgemm.FORMATS}
    out["mxfp8_at_least_bf16"] = med["mxfp8"] >= med["bf16"]
    dump("rates.json", out)

    print("SUMMARY")
    print("burn-in TF/s, median", {f: round(v, 1) for f, v in med.items()})
    print("GEMM only TF/s, median",
          {f: round(v, 1) for f, v in out["gemm_only_median_tflops"].items()})
    print("fraction of the register-resident ceiling", out["fraction_of_ceiling"])
    clean = all(r["ok"] for runs in out["burn_in"].values() for r in runs)
    if not clean or not out["mxfp8_at_least_bf16"]:
        print("a burn-in found mismatches, or the mxfp8 burn-in is slower than the bf16 one")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
