"""Tenant-side check after an attach: ``python -m gpumounter_amd.parallel.validate``.

Run inside the pod once GPUs were hot-mounted. It answers the questions a tenant has before
starting a job on them — the reference offers nothing here:

1. every visible GPU runs a gfx950 kernel (wave64 liveness probe, :mod:`gpumounter_amd.ops.probe`);
2. every pair has peer access and xGMI-class copy bandwidth (:func:`collectives.xgmi_matrix`);
3. RCCL works across all of them: one process per GPU, ``torch.distributed`` with backend
   ``nccl`` (RCCL on ROCm), a checked bf16 all-reduce with ring bus bandwidth
   (:func:`collectives.allreduce_check`);
4. optionally (``--burn-in SECONDS``) all GPUs under sustained MFMA load at once, each
   result bit-compared with the first: bf16 GEMMs for SECONDS (:func:`probe.burn_in`), and with
   ``--burn-in-format`` also block-scaled fp8 / fp4 ones (:func:`mxgemm.burn_in`). Catches
   silent data corruption and throttling that a short probe misses;
5. optionally (``--memtest [SIZE]``) the HBM pattern test on all GPUs at once
   (:func:`gpumounter_amd.ops.memtest.memtest`): SIZE bytes per GPU, by default 90 % of what is
   free on it, written and read back in both polarities of five patterns;
6. optionally (``--cu-scan``) the per-CU self-test on all GPUs at once
   (:func:`gpumounter_amd.ops.cuscan.scan`): known-answer integer, fp32, MFMA and LDS tests on
   every compute unit, a wrong word attributed to the CU that produced it;
7. optionally (``--host-link [SIZE]``) the host link (PCIe) test on all GPUs at once
   (:func:`gpumounter_amd.ops.hostlink.hostlink`): checked transfers between pinned host memory
   and each GPU in both directions, by the copy engines and by kernels, with per-leg GB/s;
8. optionally (``--atomics``) the cross-XCC atomics and coherence test on all GPUs at once
   (:func:`gpumounter_amd.ops.atomics.run`): known-answer atomics of ten kinds, tickets, a CAS
   loop and in-launch hand-offs between blocks with the agent-scope release and acquire;
9. optionally (``--host-sync``) the host-GPU atomics and hand-off test on all GPUs at once
   (:func:`gpumounter_amd.ops.hostsync.run`): system-scope atomics on pinned host memory with two
   host threads per GPU contending, and release/acquire hand-offs through flags in host memory
   in both directions;
10. optionally (``--mfma-scan``) the per-CU matrix-core format scan on all GPUs at once
   (:func:`gpumounter_amd.ops.mfmascan.scan`): bit-exact MFMAs in f16, fp8, bf8, i8, f32, f64 and
   the block-scaled fp8, bf8, fp6, bf6 and fp4 forms on every compute unit;
11. optionally (``--lane-scan``) the per-CU register, lane and scalar-unit scan on all GPUs at once
   (:func:`gpumounter_amd.ops.lanescan.scan`): bit-exact cross-lane moves, a register-file march,
   a scalar chain, transcendentals at exact points, fp64 and packed arithmetic on every compute
   unit;
12. optionally (``--cache-scan``) the per-CU cache scan on all GPUs at once
   (:func:`gpumounter_amd.ops.cachescan.scan`): a march served by the L2, hit and replacement
   passes through the vector L1, a pointer chase through the scalar data cache and a body larger
   than the instruction cache on every compute unit;
13. optionally (``--lds-scan``) the per-CU LDS scan on all GPUs at once
   (:func:`gpumounter_amd.ops.ldsscan.scan`): sub-dword, wide and paired LDS accesses, the LDS
   atomics, the bank crossbar at every conflict degree, the transposing read and direct
   global-to-LDS loads on every compute unit;
14. optionally (``--sparse-scan``) the per-CU sparse and 32x32 matrix-core scan on all GPUs at once
   (:func:`gpumounter_amd.ops.sparsescan.scan`): bit-exact 2:4 sparse SMFMACs in f16, bf16, i8,
   fp8, bf8 and mixed fp8/bf8 at 16x16 and in f16, bf16, i8 and fp8 at 32x32 on every compute
   unit.

Prints one JSON document; exit code 0 only if every check passed. ``--cpu-ranks N`` runs step 3
with N gloo ranks on the CPU (hermetic tests).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, List

from gpumounter_amd import burnin_options
from gpumounter_amd.ops import cuframe, mxgemm
from gpumounter_amd.ops.probe import ProbeError


def _rank_main(rank: int, world: int, cpu: bool, numel: int, out_dir: str) -> None:
    import torch
    import torch.distributed as dist

    from gpumounter_amd.parallel.collectives import allreduce_check

    # file:// rendezvous in the run's own directory: no TCP port picked ahead of time (another
    # process can take a port between the pick and rank 0's bind)
    rdv = "file://" + os.path.join(out_dir, "rendezvous")
    if cpu:
        dist.init_process_group("gloo", init_method=rdv, rank=rank, world_size=world)
        dev = torch.device("cpu")
    else:
        torch.cuda.set_device(rank)
        dev = torch.device("cuda", rank)
        dist.init_process_group("nccl", init_method=rdv, rank=rank, world_size=world,
                                device_id=dev)
    try:
        res = allreduce_check(numel=numel, device=dev)
    finally:
        dist.destroy_process_group()
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as fh:
        json.dump(res, fh)


def run_allreduce(world: int, cpu: bool, numel: int) -> List[Dict]:
    import tempfile

    import torch.multiprocessing as mp

    with tempfile.TemporaryDirectory(prefix="gm-validate-") as out_dir:
        mp.spawn(_rank_main, args=(world, cpu, numel, out_dir), nprocs=world, join=True)
        res = []
        for r in range(world):
            with open(os.path.join(out_dir, f"rank{r}.json")) as fh:
                res.append(json.load(fh))
    return res


def _run_scan(scan, args, controls: Dict, world: int, report: Dict) -> None:
    """One per-CU scan, if it was asked for, on every GPU at once, booked under its key."""
    if not getattr(args, scan.stem):
        return
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=world) as ex:
        res = list(ex.map(lambda d: scan.run(d, **controls[scan.key]), range(world)))
    for r in res:
        del r["per_cu"]                   # one line per CU and GPU; "failed" names the bad ones
    report[scan.key] = res
    report["ok"] &= all(r["ok"] for r in res)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="gpumounter_amd.parallel.validate")
    ap.add_argument("--cpu-ranks", type=int, default=0,
                    help="skip the GPU checks; all-reduce over N gloo ranks on the CPU")
    ap.add_argument("--numel", type=int, default=1 << 24, help="all-reduce elements (bf16)")
    ap.add_argument("--no-p2p", action="store_true")
    burnin_options.add_options(ap, "then load every GPU at once with bit-checked GEMMs for "
                                   "SECONDS, one format after the other")
    ap.add_argument("--memtest", nargs="?", const="auto", default=None, metavar="SIZE",
                    help="then the HBM pattern test on every GPU at once over SIZE bytes each "
                         "(64M, 8G; default: 90 %% of the free memory)")
    cu, *later = cuframe.all_scans()  # the CU scan: before the host-link and atomics tests
    ap.add_argument("--cu-scan", action="store_true",
                    help=f"then the {cu.title} on every GPU at once")
    ap.add_argument("--host-link", nargs="?", const="auto", default=None, metavar="SIZE",
                    help="then the host link (PCIe) test on every GPU at once over SIZE bytes of "
                         "pinned host memory per buffer (default 256M)")
    ap.add_argument("--atomics", action="store_true",
                    help="then the cross-XCC atomics and coherence test on every GPU at once")
    ap.add_argument("--atomics-inject", default=None, metavar="TEST:...",
                    help="its negative control (see probe --atomics-inject); needs --atomics")
    ap.add_argument("--host-sync", action="store_true",
                    help="then the host-GPU atomics and hand-off test on every GPU at once")
    ap.add_argument("--host-sync-inject", default=None, metavar="TEST:...",
                    help="its negative control (see probe --host-sync-inject); needs --host-sync")
    for scan in later:
        ap.add_argument(f"--{scan.label}", action="store_true",
                        help=f"then the {scan.title}{scan.covers} on every GPU at once")
        for name, (metavar, _, what) in scan.controls.items():
            ap.add_argument(f"--{scan.label}-{name}", default=None, metavar=metavar,
                            help=f"its {what} (see probe --{scan.label}-{name}); needs "
                                 f"--{scan.label}")
    args = ap.parse_args(argv)
    controls: Dict = {cu.key: {}}     # scan → the keyword arguments of its negative controls
    for scan in reversed(later):      # errors have always been reported for the last scan first
        texts = {name: getattr(args, f"{scan.stem}_{name}") for name in scan.controls}
        given = [name for name, text in texts.items() if text is not None]
        if given and not getattr(args, scan.stem):
            ap.error(f"--{scan.label}-{given[0]} needs --{scan.label}")
        try:
            controls[scan.key] = {
                f"_{name}": text if text is None else getattr(scan.module, f"parse_{name}")(text)
                for name, text in texts.items()}
        except ProbeError as e:
            ap.error(str(e))
    error = burnin_options.usage(args, name_pair=True)
    if error:
        ap.error(error)
    burn_in_formats, burn_in_flips = args.burn_in_format or ("bf16",), args.burn_in_flip
    # the attributed mode's keywords, none unless asked for
    burn_in_more = mxgemm.attribute_kwargs(args.burn_in_attribute, args.burn_in_inject)
    atomics_inject = None
    if args.atomics_inject is not None:
        from gpumounter_amd.ops import atomics
        if not args.atomics:
            ap.error("--atomics-inject needs --atomics")
        try:
            atomics_inject = atomics.parse_inject(args.atomics_inject)
        except atomics.ProbeError as e:
            ap.error(str(e))
    host_sync_inject = None
    if args.host_sync_inject is not None:
        from gpumounter_amd.ops import hostsync
        if not args.host_sync:
            ap.error("--host-sync-inject needs --host-sync")
        try:
            host_sync_inject = hostsync.parse_inject(args.host_sync_inject)
        except hostsync.ProbeError as e:
            ap.error(str(e))
    hostlink_bytes = None
    if args.host_link not in (None, "auto"):
        from gpumounter_amd.ops import hostlink
        try:
            hostlink_bytes = hostlink.parse_size(args.host_link)
        except hostlink.ProbeError as e:
            ap.error(str(e))
        if hostlink_bytes < 16 or hostlink_bytes % 16:
            ap.error("--host-link SIZE must be a nonzero multiple of 16 bytes")
    memtest_bytes = None
    if args.memtest not in (None, "auto"):
        from gpumounter_amd.ops import memtest
        try:
            memtest_bytes = memtest.parse_size(args.memtest)
        except memtest.ProbeError as e:
            ap.error(str(e))
    report: Dict = {"ok": True}
    if args.cpu_ranks:
        world = args.cpu_ranks
    else:
        from gpumounter_amd.ops import probe
        from gpumounter_amd.parallel.collectives import xgmi_matrix

        n = probe.device_count()
        if n == 0:
            print(json.dumps({"ok": False, "error": "no GPU visible (nothing attached?)"}))
            return 1
        devs = list(range(n))
        report["gpus"] = [{"device": d, "bdf": probe.props(d)["pci_bus_id"],
                           "arch": probe.props(d)["gcn_arch"], "quick_us": probe.quick(d)}
                          for d in devs]
        if n > 1 and not args.no_p2p:
            m = xgmi_matrix(devs)
            report["p2p"] = m
            report["ok"] &= all(all(row) for row in m["peer"])
        world = n
    ranks = run_allreduce(world, bool(args.cpu_ranks), args.numel)
    report["allreduce"] = {"world": world, "ok": all(r["ok"] for r in ranks),
                           "ms": max(r["ms"] for r in ranks),
                           "busbw_gbps": min(r["busbw_gbps"] for r in ranks),
                           "bytes": ranks[0]["bytes"]}
    report["ok"] &= report["allreduce"]["ok"]
    if args.burn_in and not args.cpu_ranks:
        from concurrent.futures import ThreadPoolExecutor

        # all GPUs at once (shared power/thermal envelope); ctypes drops the GIL in the call
        for fmt in burn_in_formats:
            with ThreadPoolExecutor(max_workers=world) as ex:
                burn = list(ex.map(lambda d: mxgemm.run_burn_in(d, args.burn_in, fmt,
                                                                _flips=burn_in_flips,
                                                                **burn_in_more),
                                   range(world)))
            report[mxgemm.burn_in_key(fmt)] = burn
            report["ok"] &= all(b["ok"] for b in burn)
    if args.memtest is not None and not args.cpu_ranks:
        from concurrent.futures import ThreadPoolExecutor

        from gpumounter_amd.ops import memtest

        with ThreadPoolExecutor(max_workers=world) as ex:
            mt = list(ex.map(lambda d: memtest.memtest(d, memtest_bytes), range(world)))
        report["memtest"] = mt
        report["ok"] &= all(m["ok"] for m in mt)
    if not args.cpu_ranks:
        _run_scan(cu, args, controls, world, report)
    if args.host_link is not None and not args.cpu_ranks:
        from concurrent.futures import ThreadPoolExecutor

        from gpumounter_amd.ops import hostlink

        # all GPUs at once: they share the host's memory and, behind a switch, its upstream link
        with ThreadPoolExecutor(max_workers=world) as ex:
            hl = list(ex.map(lambda d: hostlink.hostlink(d, hostlink_bytes), range(world)))
        report["hostlink"] = hl
        report["ok"] &= all(h["ok"] for h in hl)
    if args.atomics and not args.cpu_ranks:
        from concurrent.futures import ThreadPoolExecutor

        from gpumounter_amd.ops import atomics

        with ThreadPoolExecutor(max_workers=world) as ex:
            at = list(ex.map(lambda d: atomics.run(d, _inject=atomics_inject), range(world)))
        for a in at:
            del a["pairs_stale"]          # 256 zeros per GPU unless something failed:
            #                               "first_errors" names the XCCs then
        report["atomics"] = at
        report["ok"] &= all(a["ok"] for a in at)
    if args.host_sync and not args.cpu_ranks:
        from concurrent.futures import ThreadPoolExecutor

        from gpumounter_amd.ops import hostsync

        # all GPUs at once: they share the host's memory and its root complex; two host threads
        # per GPU
        with ThreadPoolExecutor(max_workers=world) as ex:
            hs = list(ex.map(lambda d: hostsync.run(d, _inject=host_sync_inject), range(world)))
        report["hostsync"] = hs
        report["ok"] &= all(h["ok"] for h in hs)
    for scan in later if not args.cpu_ranks else ():
        _run_scan(scan, args, controls, world, report)
    print(json.dumps(report))
    return 0 if report["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
