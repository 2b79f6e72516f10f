"""Rates of the host-link (PCIe) test, in one process on one GPU (BASELINE.md "Host link
test"; raw runs in profiles/hostlink/README.md).

    python bench/hostlink_rates.py [--bytes 256M] [--runs 5] [--out rates.json]

After a warm-up call: ``--runs`` repeats of the whole default call (six legs, the default
patterns), for the per-leg GB/s, their run-to-run spread and the split of the wall time; then
the grid sweep of the three kernel legs, blocks in {4, 16, 64, 256, 512} x U in {4, 8}, every
configuration once per round and the rounds repeated, so that drift hits all of them alike.
The link files are read at rest first; every call reports what they read under load.
Numbers from different processes are not compared.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpumounter_amd import _native  # noqa: E402
from gpumounter_amd.ops import hostlink, probe  # noqa: E402

KERNEL_LEGS = ("kread", "kwrite", "kduplex")
SWEEP_BLOCKS = (4, 16, 64, 256, 512)
SWEEP_UNROLL = (4, 8)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", default="256M")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, runs, dev = hostlink.parse_size(args.bytes), args.runs, args.device
    props = probe.props(dev)
    out = {"bytes": n, "runs": runs, "props": props,
           "link_at_rest": hostlink.link_state(props["pci_bus_id"])}

    def dump():
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(out, fh, indent=1)

    print(out["props"], "\nlink at rest", out["link_at_rest"], flush=True)
    lib = _native.probe()
    default_u = lib.gm_probe_hostlink_unroll(-1)
    warm = hostlink.hostlink(dev, n, iters=2)              # clocks, code objects, first pin
    if not warm["ok"]:
        print("warm-up found wrong words:", warm)
        return 1

    keys = ("seconds", "host_seconds", "transfer_seconds", "setup_seconds")
    full = [hostlink.hostlink(dev, n) for _ in range(runs)]
    if not all(r["ok"] for r in full):
        print("the default call found wrong words:", full)
        return 1
    out["default"] = {"blocks": full[0]["blocks"], "unroll": default_u,
                      "legs": {leg: [r["legs"][leg]["gbps"] for r in full]
                               for leg in hostlink.ALL_LEGS},
                      "bidir_h2d": [r["legs"]["bidir"]["h2d"]["gbps"] for r in full],
                      "bidir_d2h": [r["legs"]["bidir"]["d2h"]["gbps"] for r in full],
                      "rate_above_link": {leg: [r["legs"][leg]["rate_above_link"] for r in full]
                                          for leg in hostlink.ALL_LEGS},
                      **{k: [r[k] for r in full] for k in keys},
                      "link": [r["link"] for r in full]}
    print("default", json.dumps(out["default"]), flush=True)
    dump()

    sweep = {f"u{u}_b{b}": {leg: [] for leg in KERNEL_LEGS}
             for u in SWEEP_UNROLL for b in SWEEP_BLOCKS}
    try:
        for _ in range(runs):
            for u in SWEEP_UNROLL:
                lib.gm_probe_hostlink_unroll(u)
                for b in SWEEP_BLOCKS:
                    r = hostlink.hostlink(dev, n, legs=KERNEL_LEGS, patterns=("random",), blocks=b)
                    if not r["ok"]:
                        print("sweep found wrong words:", u, b, r)
                        return 1
                    for leg in KERNEL_LEGS:
                        sweep[f"u{u}_b{b}"][leg].append(r["legs"][leg]["gbps"])
    finally:
        lib.gm_probe_hostlink_unroll(default_u)
    out["sweep"] = sweep
    dump()

    def stat(v):
        return f"median {statistics.median(v):.2f} min {min(v):.2f} max {max(v):.2f}"

    print("SUMMARY (GB/s)")
    for leg in hostlink.ALL_LEGS:
        print("default", leg, stat(out["default"]["legs"][leg]))
    print("default bidir h2d", stat(out["default"]["bidir_h2d"]), "d2h",
          stat(out["default"]["bidir_d2h"]))
    for k in keys:
        print("default", k, stat(out["default"][k]))
    for cfg, legs in sweep.items():
        print(cfg, " | ".join(f"{leg} {stat(v)}" for leg, v in legs.items()))
    print("link under load", json.dumps(full[-1]["link"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
