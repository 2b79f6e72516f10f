"""Times of the host-GPU atomics and hand-off test (``ops.hostsync``): the default call repeated,
with the longest polls of both sides, the host-measured round trip and each test's wall time, and
the budget defaults that the measurement rule gives.

    python bench/hostsync_rates.py [--device 0] [--calls 20] [--budget-us 2000]
                                   [--host-budget-us 10000] [--json]

The rule (the atomics test used it for its 200 us): each default is the larger of its floor
(1000 us on the GPU, 5000 us on the host) and 8 x the longest poll measured over the calls on an
idle GPU. The calls themselves run with the generous starting budgets given on the command line,
so that a slow poll is measured and not cut off. No time is a pass or fail condition anywhere.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpumounter_amd.ops import hostsync  # noqa: E402

FLOOR_US = {"h2d": 1000, "d2h": 5000}       # the GPU's budget, the host's


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--budget-us", type=int, default=2000)
    ap.add_argument("--host-budget-us", type=int, default=10000)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args(argv)
    rows = []
    for _ in range(args.calls):
        r = hostsync.run(args.device, budget_us=args.budget_us,
                         host_budget_us=args.host_budget_us)
        if not r["ok"]:
            print(json.dumps(r, indent=1), file=sys.stderr)
            return 1
        rows.append({"seconds": r["seconds"], "ms": r["ms"],
                     "host_ops_in_flight": r["host_ops_in_flight"],
                     "rtt_median_us": r["rtt_median_us"], "rtt_max_us": r["rtt_max_us"],
                     **{d: {k: r[d][k] for k in ("observed", "unseen", "poll_max_us")}
                        for d in hostsync.DIRECTIONS}})
    first = hostsync.run(args.device, tests=("handoff",), budget_us=args.budget_us,
                         host_budget_us=args.host_budget_us)   # geometry of the calls
    longest = {d: max(x[d]["poll_max_us"] for x in rows) for d in hostsync.DIRECTIONS}
    summary = {
        "calls": args.calls, "blocks": first["blocks"], "host_threads": first["host_threads"],
        "rounds": first["rounds"], "lines": first["lines"],
        "atomics_supported": first["atomics_supported"],
        "call_ms_median": sorted(x["seconds"] for x in rows)[len(rows) // 2] * 1e3,
        "call_ms_max": max(x["seconds"] for x in rows) * 1e3,
        "unseen": {d: sum(x[d]["unseen"] for x in rows) for d in hostsync.DIRECTIONS},
        "poll_max_us": longest,
        "rtt_median_us": sorted(x["rtt_median_us"] for x in rows)[len(rows) // 2],
        "rtt_max_us": max(x["rtt_max_us"] for x in rows),
        "host_ops_in_flight_median": sorted(x["host_ops_in_flight"] for x in rows)[len(rows) // 2],
        "defaults_by_the_rule": {
            "budget_us": max(FLOOR_US["h2d"], int(8 * longest["h2d"] + 0.999)),
            "host_budget_us": max(FLOOR_US["d2h"], int(8 * longest["d2h"] + 0.999))},
        "defaults_in_the_source": {"budget_us": hostsync.DEFAULT_BUDGET_US,
                                   "host_budget_us": hostsync.DEFAULT_HOST_BUDGET_US}}
    if args.json:
        print(json.dumps({"summary": summary, "calls": rows}))
        return 0
    for i, x in enumerate(rows):
        ms = " ".join(f"{n} {v:.2f}" for n, v in x["ms"].items())
        print(f"call {i:2d}: {x['seconds'] * 1e3:6.1f} ms ({ms}); polls max h2d "
              f"{x['h2d']['poll_max_us']:.1f} us d2h {x['d2h']['poll_max_us']:.1f} us; round trip "
              f"median {x['rtt_median_us']:.1f} max {x['rtt_max_us']:.1f} us; "
              f"{x['host_ops_in_flight']} host ops in flight")
    print(json.dumps(summary, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
