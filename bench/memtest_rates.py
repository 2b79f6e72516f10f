"""Rates of the HBM pattern test against the HBM probes, in one process on one GPU
(BASELINE.md "HBM pattern test"; raw runs in profiles/memtest/README.md).

    python bench/memtest_rates.py [--bytes 16G] [--runs 5] [--out rates.json]

Five runs each of ``probe.hbm_read_gbps``, ``probe.hbm_gbps`` and of the memtest per pattern
(2 passes), with nontemporal and with plain stores, after a warm-up of both; then the default
five-pattern run and the negative control. Numbers from different processes are not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpumounter_amd import _native  # noqa: E402
from gpumounter_amd.ops import memtest, probe  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", default="16G")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, runs, dev = memtest.parse_size(args.bytes), args.runs, args.device
    out = {"bytes": n, "runs": runs, "props": probe.props(dev), "mem": memtest.mem_info(dev)}

    def dump():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    print(out["props"], out["mem"], flush=True)
    probe.hbm_read_gbps(dev, n, 3)                     # warm-up: clocks and code objects
    memtest.memtest(dev, n, patterns=("addr",))
    out["hbm_read_gbps"] = [probe.hbm_read_gbps(dev, n, 10) for _ in range(runs)]
    print("hbm_read_gbps", out["hbm_read_gbps"], flush=True)
    out["hbm_gbps"] = [probe.hbm_gbps(dev, n, 10) for _ in range(runs)]
    print("hbm_gbps", out["hbm_gbps"], flush=True)
    dump()
    lib = _native.probe()
    keys = ("read_gbps", "write_gbps", "rw_gbps", "seconds")
    for variant, name in ((1, "nontemporal"), (0, "plain")):
        lib.gm_probe_memtest_store_variant(variant)
        out[name] = {}
        for p in memtest.ALL_PATTERNS:
            rs = [memtest.memtest(dev, n, patterns=(p,), passes=2) for _ in range(runs)]
            if not all(r["ok"] and r["bytes"] == n for r in rs):
                print("memtest failed or ran short:", rs)
                return 1
            out[name][p] = {k: [r[k] for r in rs] for k in keys}
            print(name, p, {k: [round(x) for x in out[name][p][k]] for k in keys[:3]}, flush=True)
            dump()
    lib.gm_probe_memtest_store_variant(1)
    out["full"] = memtest.memtest(dev, n)
    print("full", out["full"], flush=True)
    flip_at = min(n // 2 + (1 << 30), n - 16) // 8 * 8 + 8      # 9 GiB + 8 of 16 GiB
    out["flip"] = memtest.memtest(dev, n, _flip=(flip_at, 0x10))
    print("flip", {k: out["flip"][k] for k in ("errors", "bit_errors", "stuck_mask", "ok")})
    dump()

    def med(v):
        return round(statistics.median(v))

    print("SUMMARY")
    for k in ("hbm_read_gbps", "hbm_gbps"):
        print(k, med(out[k]), "spread", round(max(out[k]) - min(out[k])))
    for name in ("nontemporal", "plain"):
        for p in memtest.ALL_PATTERNS:
            d = out[name][p]
            print(name, p, "read", med(d["read_gbps"]), "write", med(d["write_gbps"]), "rw",
                  med(d["rw_gbps"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
