"""Command line: daemons and operator tools.

    python -m gpumounter_amd master   [--config f.yaml] [--port 8080]
    python -m gpumounter_amd worker   [--config f.yaml] [--node NAME]
    python -m gpumounter_amd inventory [--amdsmi mock]          # amdsmi view of this node
    python -m gpumounter_amd topology  [--amdsmi mock] [-n 4]   # xGMI/NUMA placement preview
    python -m gpumounter_amd probe     [--bdf 0000:05:00.0] [--full] [--burn-in 60]  # gfx950 kernels
                                       [--burn-in-flip ELEM:MASK]            # its negative control
                                       [--burn-in-format bf16,mxfp8,mxfp4]   # also on the MX pipe
                                       [--burn-in-attribute]                 # rotate tiles, name CUs
                                       [--burn-in-inject ID|first:MASK]      # its negative control
                                       [--memtest [SIZE]] [--memtest-passes N]
                                       [--memtest-patterns addr,solid,checker,walk,random]
                                       [--memtest-flip OFFSET:MASK]          # HBM pattern test
                                       [--cu-scan] [--cu-scan-tests int,f32,mfma,lds]
                                       [--cu-scan-rounds N]                  # per-CU self-test
                                       [--cu-scan-inject ID|any:TEST:THREAD:WORD:MASK]
                                       [--host-link [SIZE]] [--host-link-legs h2d,d2h,...]
                                       [--host-link-patterns addr,random] [--host-link-blocks N]
                                       [--host-link-flip LEG:OFFSET:MASK]    # host link (PCIe) test
                                       [--atomics] [--atomics-tests add,ticket,cas,handoff]
                                       [--atomics-spread N] [--atomics-blocks N]
                                       [--atomics-rounds N]                  # cross-XCC atomics
                                       [--atomics-inject add:KIND:G:S:MASK|cas:G:S:MASK|
                                                         ticket:G:S|handoff:BLOCK:ROUND:WORD:MASK]
                                       [--host-sync] [--host-sync-tests add,ticket,swap,cas,handoff]
                                       [--host-sync-blocks N] [--host-sync-threads N]
                                       [--host-sync-rounds N]     # host-GPU atomics and hand-offs
                                       [--host-sync-inject add:KIND:G:S:MASK|cas:G:S:MASK|
                                                  ticket:G:S|swap:G:S:MASK|
                                                  handoff:DIR:BLOCK:ROUND:WORD:MASK]
                                       [--mfma-scan] [--mfma-scan-formats f16,fp8,...,mxfp4]
                                       [--mfma-scan-iters N] [--mfma-scan-rounds N]
                                       [--mfma-scan-inject ID|any:FORMAT:THREAD:WORD:MASK]
                                                                # per-CU matrix-core format scan
                                       [--lane-scan] [--lane-scan-tests xlane,regfile,...,packed]
                                       [--lane-scan-iters N] [--lane-scan-rounds N]
                                       [--lane-scan-inject ID|any:TEST:THREAD:WORD:MASK]
                                                  # per-CU register, lane and scalar-unit scan
                                       [--cache-scan] [--cache-scan-tests l2,l1,scalar,icache]
                                       [--cache-scan-iters N] [--cache-scan-rounds N]
                                       [--cache-scan-inject ID|any:TEST:THREAD:WORD:MASK]
                                       [--cache-scan-poke TEST:WORD_OFFSET:MASK]
                                           # per-CU vector L1, L2, scalar and instruction caches
    python -m gpumounter_amd add    --master URL --ns NS --pod P -n 2 [--entire] [--lease 3600]
    python -m gpumounter_amd remove --master URL --ns NS --pod P --uuid U [--uuid U2] [--force]
    python -m gpumounter_amd status --master URL --node NODE
    python -m gpumounter_amd bpf-dump --allow 226:128 --allow 511:0   # generated device program
    python -m gpumounter_amd doctor  [--json] [--skip-cluster] [--gpu [--burn-in 30]]  # preflight
                                     [--gpu --memtest [SIZE]] [--gpu --cu-scan]
                                     [--gpu --host-link [SIZE]] [--gpu --atomics]
                                     [--gpu --host-sync]
                                     [--gpu --mfma-scan] [--gpu --lane-scan]
                                     [--gpu --cache-scan]
    python -m gpumounter_amd config-doc > docs/CONFIG.md   # every GM_* setting, from the source

The reference ships only the two daemons and documents curl calls (QuickStart.md:41-92); the
``add``/``remove`` commands speak exactly those HTTP routes.
"""
from __future__ import annotations

import argparse
import asyncio
import json
import os
import sys
from typing import List, Optional

from gpumounter_amd import burnin_options


def _cfg(args, **over):
    from gpumounter_amd.utils.config import Config

    return Config.load(getattr(args, "config", None), **over)


def _run_daemon(serve, cfg) -> int:
    """asyncio.run(serve(cfg)); with GM_PROFILE_OUT=<file> under cProfile, stats written at
    (SIGTERM-clean) shutdown — for finding the hot spots of a live daemon (``{pid}`` in the
    name is replaced, so several daemons can share the setting)."""
    if getattr(cfg, "cpu_affinity", ""):
        from gpumounter_amd.utils import runtime
        runtime.pin_cpus(cfg.cpu_affinity)
    out = os.environ.get("GM_PROFILE_OUT", "").replace("{pid}", str(os.getpid()))
    if not out:
        asyncio.run(serve(cfg))
        return 0
    if os.environ.get("GM_PROFILE_MODE", "cprofile") == "sample":
        # statistical: setitimer(ITIMER_PROF) stack samples (gpumounter_amd/utils/sampler.py)
        from gpumounter_amd.utils.sampler import Sampler

        smp = Sampler(1.0 / float(os.environ.get("GM_PROFILE_HZ", "2000")))
        smp.start()
        try:
            asyncio.run(serve(cfg))
        finally:
            smp.stop()
            smp.dump(out, {"argv": sys.argv[1:]})
        return 0
    import cProfile

    prof = cProfile.Profile()
    prof.enable()
    try:
        asyncio.run(serve(cfg))
    finally:
        prof.disable()
        prof.dump_stats(out)
    return 0


def cmd_master(args) -> int:
    from gpumounter_amd.master.app import serve
    from gpumounter_amd.utils import log

    cfg = _cfg(args, master_port=args.port)
    log.setup(cfg.log_level, cfg.log_json, cfg.log_file)
    return _run_daemon(serve, cfg)


def cmd_worker(args) -> int:
    from gpumounter_amd.utils import log
    from gpumounter_amd.worker.server import serve

    cfg = _cfg(args, node_name=args.node, worker_port=args.port)
    log.setup(cfg.log_level, cfg.log_json, cfg.log_file)
    return _run_daemon(serve, cfg)


def cmd_device_plugin(args) -> int:
    """Standalone amd.com/gpu device plugin (topology-packed allocation for ordinary pods, no
    hot-mount worker). Runs until SIGTERM/SIGINT."""
    import signal

    from gpumounter_amd.deviceplugin.plugin import AmdGpuDevicePlugin
    from gpumounter_amd.hw.inventory import Inventory
    from gpumounter_amd.utils import log

    cfg = _cfg(args)
    log.setup(cfg.log_level, cfg.log_json, cfg.log_file)
    inv = Inventory(args.amdsmi if args.amdsmi is not None else cfg.amdsmi_lib, cfg.kfd_major,
                    cfg.kfd_dev_path)

    async def run():
        plugin = AmdGpuDevicePlugin(inv, cfg.resource_name, args.dir or cfg.device_plugin_dir,
                                    inject_devices=cfg.device_plugin_inject,
                                    health_period_s=cfg.device_plugin_health_s,
                                    policy=cfg.topology_policy)
        await plugin.start(register=not args.no_register)
        stop = asyncio.Event()
        loop = asyncio.get_running_loop()
        for sig in (signal.SIGTERM, signal.SIGINT):
            loop.add_signal_handler(sig, stop.set)
        print(json.dumps({"socket": plugin.socket_path, "devices": len(plugin.health)}),
              flush=True)
        await stop.wait()
        await plugin.stop()

    asyncio.run(run())
    return 0


def cmd_inventory(args) -> int:
    from gpumounter_amd.hw.inventory import Inventory

    inv = Inventory(args.amdsmi)
    out = inv.summary()
    if args.processes:
        out["processes"] = {g.index: [p.__dict__ for p in inv.processes(g.index)]
                            for g in inv.gpus()}
    print(json.dumps(out, indent=2))
    return 0


def cmd_topology(args) -> int:
    from gpumounter_amd.hw import topology
    from gpumounter_amd.hw.inventory import Inventory

    inv = Inventory(args.amdsmi)
    gpus = inv.gpus()
    out = {"describe": topology.describe(gpus, inv.links()), "plans": {}}
    for n in ([args.n] if args.n else range(1, len(gpus) + 1)):
        p = topology.choose(gpus, n, inv.links(), policy=args.policy)
        out["plans"][n] = p.to_dict() if p else None
    print(json.dumps(out, indent=2))
    return 0


MEMTEST_AUTO = -1     # --memtest without a SIZE: most of the device's free memory


def _memtest_bytes(size: int) -> Optional[int]:
    return None if size == MEMTEST_AUTO else size


def _memtest_arg(kind):
    """argparse type for the --memtest-* options: the parser in ops.memtest, with its refusal
    turned into a usage error."""
    def conv(text):
        from gpumounter_amd.ops import memtest
        try:
            return getattr(memtest, kind)(text)
        except memtest.ProbeError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
    conv.__name__ = kind
    return conv


def _burn_in_usage(args, tool: str) -> int:
    """2 with the usage error printed if the burn-in's options do not go together, else 0."""
    error = burnin_options.usage(args, format_first=tool == "doctor")
    if error:
        print(f"{tool}: {error}", file=sys.stderr)
    return 2 if error else 0          # a usage error, not a failed burn-in (exit 1)


def _atomics_arg(kind):
    """argparse type for the --atomics-* options: the parser in ops.atomics, its refusal a usage
    error."""
    def conv(text):
        from gpumounter_amd.ops import atomics
        try:
            return getattr(atomics, kind)(text)
        except atomics.ProbeError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
    conv.__name__ = kind
    return conv


def _add_atomics(p, what: str) -> None:
    p.add_argument("--atomics", action="store_true", help=what)
    p.add_argument("--atomics-inject", type=_atomics_arg("parse_inject"), default=None,
                   metavar="TEST:...",
                   help="negative control: add:KIND:G:S:MASK, cas:G:S:MASK, ticket:G:S or "
                        "handoff:BLOCK:ROUND:WORD:MASK; the test must report it")


def _hostsync_arg(kind):
    """argparse type for the --host-sync-* options: the parser in ops.hostsync, its refusal a
    usage error."""
    def conv(text):
        from gpumounter_amd.ops import hostsync
        try:
            return getattr(hostsync, kind)(text)
        except hostsync.ProbeError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
    conv.__name__ = kind
    return conv


def _add_hostsync(p, what: str) -> None:
    p.add_argument("--host-sync", action="store_true", help=what)
    p.add_argument("--host-sync-inject", type=_hostsync_arg("parse_inject"), default=None,
                   metavar="TEST:...",
                   help="negative control: add:KIND:G:S:MASK, cas:G:S:MASK, ticket:G:S, "
                        "swap:G:S:MASK or handoff:DIR:BLOCK:ROUND:WORD:MASK; the test must "
                        "report it")


def _scans():
    from gpumounter_amd.ops import cuframe

    return cuframe.scans()


def _all_scans():
    from gpumounter_amd.ops import cuframe

    return cuframe.all_scans()


def _scan_arg(scan, kind):
    """argparse type for a per-CU scan's options: the parser in the scan's module, its refusal a
    usage error."""
    def conv(text):
        from gpumounter_amd.ops.probe import ProbeError
        try:
            return getattr(scan.module, kind)(text)
        except ProbeError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
    conv.__name__ = kind
    return conv


def _add_controls(p, scan) -> None:
    for name, (metavar, text, _) in scan.controls.items():
        p.add_argument(f"--{scan.label}-{name}", type=_scan_arg(scan, f"parse_{name}"),
                       default=None, metavar=metavar, help=text)


def _add_probe_scan(p, scan) -> None:
    """probe's options of one scan: the scan and its controls, its selection, iterations and
    rounds."""
    p.add_argument(f"--{scan.label}", action="store_true",
                   help=f"{scan.title} of every probed GPU: {scan.does} on every compute unit "
                        f"(exit 1 on any wrong word)")
    if not scan.plain_cli:
        _add_controls(p, scan)
    p.add_argument(f"--{scan.label}-{scan.selection}",
                   type=_scan_arg(scan, f"parse_{scan.selection}"), metavar="a,b,...",
                   default=scan.all if scan.plain_cli else None,
                   help=None if scan.plain_cli else f"of {','.join(scan.all)} (default: all)")
    if scan.iters_unit:
        p.add_argument(f"--{scan.label}-iters", type=int, default=None, metavar="N",
                       help=f"{scan.iters_unit}, 1..{scan.max_iters} (default "
                            f"{scan.default_iters})")
    p.add_argument(f"--{scan.label}-rounds", type=int, default=1 if scan.plain_cli else None,
                   metavar="N", help="at least N rounds (a round is one block per CU)")
    if scan.plain_cli:
        _add_controls(p, scan)      # the CU scan lists its own last


def _add_doctor_scan(p, scan) -> None:
    p.add_argument(f"--{scan.label}", action="store_true",
                   help=f"with --gpu: {scan.title}{scan.covers} of every GPU; a failing CU is named"
                        + ("" if scan.plain_cli else f" with the {scan.unit}"))
    if not scan.plain_cli:
        _add_controls(p, scan)


def _scan_usage(scan, args, tool: str) -> Optional[str]:
    """What is wrong with the scan's options on ``tool``'s command line (None: nothing), checked
    before any GPU work."""
    from gpumounter_amd.ops.cuframe import MAX_ROUNDS

    got = {name: getattr(args, f"{scan.stem}_{name}", None)
           for name in (*scan.controls, scan.selection, "iters", "rounds")}
    if not getattr(args, scan.stem):
        given = [n for n, v in got.items() if v is not None and not (
            scan.plain_cli and n in (scan.selection, "rounds"))]      # those have defaults
        if given:
            return f"{tool}: --{scan.label}-{given[0]} needs --{scan.label}"
    if got["iters"] is not None and not 1 <= got["iters"] <= scan.max_iters:
        return f"{tool}: --{scan.label}-iters must be between 1 and {scan.max_iters}"
    if got["rounds"] is not None and not 1 <= got["rounds"] <= MAX_ROUNDS:
        return f"{tool}: --{scan.label}-rounds must be between 1 and {MAX_ROUNDS}"
    for name in scan.controls:
        # an injection names its test after the CU, a poke first
        named = got[name] and got[name][1 if name == "inject" else 0]
        if named and got[scan.selection] is not None and named not in got[scan.selection]:
            return (f"{tool}: --{scan.label}-{name} into {named!r}, which "
                    f"--{scan.label}-{scan.selection} leaves out")
    return None


def _run_scan(scan, args, res) -> bool:
    """The scan, if it was asked for, on every probed GPU, booked under its key in ``res``;
    false: one found an error."""
    if not getattr(args, scan.stem):
        return True
    rounds = getattr(args, f"{scan.stem}_rounds") or 1
    kw = {scan.selection: getattr(args, f"{scan.stem}_{scan.selection}") or scan.all}
    if scan.iters_unit:
        kw["iters"] = getattr(args, f"{scan.stem}_iters") or scan.default_iters
    kw.update(min_rounds=rounds, max_rounds=max(16, rounds))
    kw.update({f"_{name}": getattr(args, f"{scan.stem}_{name}") for name in scan.controls})
    for r in res:
        r[scan.key] = scan.run(r["device"], **kw)
    return all(r[scan.key]["ok"] for r in res)


HOSTLINK_AUTO = -1    # --host-link without a SIZE: the test's default size


def _hostlink_arg(kind):
    """argparse type for the --host-link-* options: the parser in ops.hostlink, its refusal a
    usage error."""
    def conv(text):
        from gpumounter_amd.ops import hostlink
        try:
            return getattr(hostlink, kind)(text)
        except hostlink.ProbeError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
    conv.__name__ = kind
    return conv


def _hostlink_bytes(size: int) -> Optional[int]:
    return None if size == HOSTLINK_AUTO else size


def _add_hostlink_size(p, what: str) -> None:
    p.add_argument("--host-link", nargs="?", const=HOSTLINK_AUTO, default=None, metavar="SIZE",
                   type=_hostlink_arg("parse_size"), help=what)


def _add_memtest_size(p, what: str) -> None:
    p.add_argument("--memtest", nargs="?", const=MEMTEST_AUTO, default=None, metavar="SIZE",
                   type=_memtest_arg("parse_size"), help=what)


def cmd_probe(args) -> int:
    from gpumounter_amd.ops import probe

    if _burn_in_usage(args, "probe"):
        return 2
    cu, *later = _all_scans()         # the CU scan: before the host-link and atomics tests
    error = _scan_usage(cu, args, "probe")
    if error:
        print(error, file=sys.stderr)
        return 2
    if args.host_link is None:
        given = [o for o, v in (("--host-link-flip", args.host_link_flip),
                                ("--host-link-legs", args.host_link_legs),
                                ("--host-link-patterns", args.host_link_patterns),
                                ("--host-link-blocks", args.host_link_blocks)) if v is not None]
        if given:
            print(f"probe: {given[0]} needs --host-link", file=sys.stderr)
            return 2
    else:
        if args.host_link != HOSTLINK_AUTO and (args.host_link < 16 or args.host_link % 16):
            print("probe: --host-link SIZE must be a nonzero multiple of 16 bytes",
                  file=sys.stderr)
            return 2
        flip = args.host_link_flip
        if flip and args.host_link_legs is not None and flip[0] not in args.host_link_legs:
            print(f"probe: --host-link-flip into {flip[0]!r}, which --host-link-legs leaves out",
                  file=sys.stderr)
            return 2
        if flip:
            from gpumounter_amd.ops import hostlink as _hl

            size = _hl.DEFAULT_BYTES if args.host_link == HOSTLINK_AUTO else args.host_link
            if flip[1] + 8 > size:
                print(f"probe: --host-link-flip offset {flip[1]} is outside the {size} bytes "
                      f"tested", file=sys.stderr)
                return 2
    if not args.atomics:
        given = [o for o, v in (("--atomics-inject", args.atomics_inject),
                                ("--atomics-tests", args.atomics_tests),
                                ("--atomics-spread", args.atomics_spread),
                                ("--atomics-blocks", args.atomics_blocks),
                                ("--atomics-rounds", args.atomics_rounds)) if v is not None]
        if given:
            print(f"probe: {given[0]} needs --atomics", file=sys.stderr)
            return 2
    else:
        from gpumounter_amd.ops import atomics as _at

        if args.atomics_blocks is not None and not 1 <= args.atomics_blocks <= _at.MAX_BLOCKS:
            print(f"probe: --atomics-blocks must be between 1 and {_at.MAX_BLOCKS}",
                  file=sys.stderr)
            return 2
        if args.atomics_rounds is not None and not 1 <= args.atomics_rounds <= _at.MAX_ROUNDS:
            print(f"probe: --atomics-rounds must be between 1 and {_at.MAX_ROUNDS}",
                  file=sys.stderr)
            return 2
        inj = args.atomics_inject
        if inj and args.atomics_tests is not None and inj[0] not in args.atomics_tests:
            print(f"probe: --atomics-inject into {inj[0]!r}, which --atomics-tests leaves out",
                  file=sys.stderr)
            return 2
    if not args.host_sync:
        given = [o for o, v in (("--host-sync-inject", args.host_sync_inject),
                                ("--host-sync-tests", args.host_sync_tests),
                                ("--host-sync-blocks", args.host_sync_blocks),
                                ("--host-sync-threads", args.host_sync_threads),
                                ("--host-sync-rounds", args.host_sync_rounds)) if v is not None]
        if given:
            print(f"probe: {given[0]} needs --host-sync", file=sys.stderr)
            return 2
    else:
        from gpumounter_amd.ops import hostsync as _hs

        for value, name, lo, hi in (
                (args.host_sync_blocks, "--host-sync-blocks", 1, _hs.MAX_BLOCKS),
                (args.host_sync_threads, "--host-sync-threads", 0, _hs.MAX_HOST_THREADS),
                (args.host_sync_rounds, "--host-sync-rounds", 1, _hs.MAX_ROUNDS)):
            if value is not None and not lo <= value <= hi:
                print(f"probe: {name} must be between {lo} and {hi}", file=sys.stderr)
                return 2
        tests = args.host_sync_tests or _hs.ALL_TESTS
        inj = args.host_sync_inject
        if inj and inj[0] not in tests:
            print(f"probe: --host-sync-inject into {inj[0]!r}, which --host-sync-tests leaves "
                  f"out", file=sys.stderr)
            return 2
        if args.host_sync_threads == 0 and "handoff" in tests:
            print("probe: the hand-off needs --host-sync-threads of at least 1 (or leave it out "
                  "with --host-sync-tests)", file=sys.stderr)
            return 2
    for scan in later:
        error = _scan_usage(scan, args, "probe")
        if error:
            print(error, file=sys.stderr)
            return 2
    if args.bdf:
        bdfs = args.bdf
    else:
        bdfs = [probe.props(i)["pci_bus_id"] for i in range(probe.device_count())]
    res = [r.to_dict() for r in probe.verify(bdfs, full=args.full)]
    bad = False
    if args.burn_in:
        from gpumounter_amd.ops import mxgemm

        for r in res:
            for fmt in args.burn_in_format or ("bf16",):
                key = mxgemm.burn_in_key(fmt)
                r[key] = mxgemm.run_burn_in(
                    r["device"], args.burn_in, fmt, _flips=args.burn_in_flip,
                    **mxgemm.attribute_kwargs(args.burn_in_attribute, args.burn_in_inject))
                bad |= not r[key]["ok"]
    if args.memtest is not None:
        from gpumounter_amd.ops import memtest

        for r in res:
            r["memtest"] = memtest.memtest(
                r["device"], _memtest_bytes(args.memtest), patterns=args.memtest_patterns,
                passes=args.memtest_passes, _flip=args.memtest_flip)
            bad |= not r["memtest"]["ok"]
    bad |= not _run_scan(cu, args, res)
    if args.host_link is not None:
        from gpumounter_amd.ops import hostlink

        for r in res:
            r["hostlink"] = hostlink.hostlink(
                r["device"], _hostlink_bytes(args.host_link),
                legs=args.host_link_legs or hostlink.ALL_LEGS,
                patterns=args.host_link_patterns or hostlink.DEFAULT_PATTERNS,
                blocks=args.host_link_blocks, _flip=args.host_link_flip)
            bad |= not r["hostlink"]["ok"]
    if args.atomics:
        from gpumounter_amd.ops import atomics

        for r in res:
            r["atomics"] = atomics.run(
                r["device"], tests=args.atomics_tests or atomics.ALL_TESTS,
                blocks=args.atomics_blocks or 0,
                spread=args.atomics_spread or atomics.DEFAULT_SPREAD,
                rounds=args.atomics_rounds or atomics.DEFAULT_ROUNDS,
                _inject=args.atomics_inject)
            bad |= not r["atomics"]["ok"]
    if args.host_sync:
        from gpumounter_amd.ops import hostsync

        for r in res:
            r["hostsync"] = hostsync.run(
                r["device"], tests=args.host_sync_tests or hostsync.ALL_TESTS,
                blocks=args.host_sync_blocks or 0,
                host_threads=(hostsync.DEFAULT_HOST_THREADS if args.host_sync_threads is None
                              else args.host_sync_threads),
                rounds=args.host_sync_rounds or hostsync.DEFAULT_ROUNDS,
                _inject=args.host_sync_inject)
            bad |= not r["hostsync"]["ok"]
    for scan in later:
        bad |= not _run_scan(scan, args, res)
    print(json.dumps(res, indent=2))
    return 1 if bad else 0


SA_TOKEN = "/var/run/secrets/kubernetes.io/serviceaccount/token"


def client_token(args) -> str:
    """The bearer token the master authenticates (GM_AUTHZ_MODE=kube: the caller's own
    Kubernetes token; GM_API_TOKEN: the shared one). First of: --token, $GM_TOKEN,
    --token-file, the pod's service-account token, the current kubeconfig user's token."""
    if getattr(args, "token", ""):
        return args.token
    if os.environ.get("GM_TOKEN"):
        return os.environ["GM_TOKEN"]
    for path in (getattr(args, "token_file", ""), SA_TOKEN):
        if path and os.path.exists(path):
            with open(path, encoding="utf-8") as fh:
                return fh.read().strip()
    kc = os.environ.get("KUBECONFIG", "").split(os.pathsep)[0] or \
        os.path.expanduser("~/.kube/config")
    if os.path.exists(kc):
        import yaml
        try:
            with open(kc, encoding="utf-8") as fh:
                doc = yaml.safe_load(fh) or {}
            ctx = next(c["context"] for c in doc.get("contexts", [])
                       if c["name"] == doc.get("current-context"))
            user = next((u["user"] for u in doc.get("users", [])
                         if u["name"] == ctx.get("user")), {})
            return user.get("token", "")
        except (OSError, ValueError, KeyError, StopIteration, yaml.YAMLError):
            return ""
    return ""


def client_tls(args):
    """How an https master is verified: against --ca / $GM_MASTER_CA, the system roots
    otherwise; --insecure skips verification (labs only). None for http URLs."""
    import ssl

    if not getattr(args, "master", "").startswith("https://"):
        return None
    if getattr(args, "insecure", False):
        return False
    ca = getattr(args, "ca", "") or os.environ.get("GM_MASTER_CA", "")
    return ssl.create_default_context(cafile=ca or None)


async def _http(method: str, url: str, data=None, token: str = "", tls=None) -> int:
    import aiohttp

    headers = {"Accept": "application/json"}
    if token:
        headers["Authorization"] = f"Bearer {token}"
        if url.startswith("http://") and not url.startswith(("http://127.", "http://localhost")):
            print("warning: sending a bearer token over plain HTTP; use the master's https:// "
                  "URL", file=sys.stderr)
    async with aiohttp.ClientSession() as s:
        async with s.request(method, url, data=data, headers=headers,
                             ssl=tls if tls is not None else True) as r:
            body = await r.text()
            print(body)
            if r.status == 401 and not token:
                print("unauthorized: the master wants a bearer token (--token, $GM_TOKEN, "
                      "--token-file or a kubeconfig user token)", file=sys.stderr)
            return 0 if r.status == 200 else 1


def cmd_add(args) -> int:
    from urllib.parse import urlencode

    url = (f"{args.master.rstrip('/')}/addgpu/namespace/{args.ns}/pod/{args.pod}/gpu/{args.n}/"
           f"isEntireMount/{'true' if args.entire else 'false'}")
    q = {k: v for k, v in (("container", args.container), ("lease", args.lease)) if v}
    if q:
        url += "?" + urlencode(q)
    return asyncio.run(_http("GET", url, token=client_token(args), tls=client_tls(args)))


def cmd_remove(args) -> int:
    import aiohttp

    url = (f"{args.master.rstrip('/')}/removegpu/namespace/{args.ns}/pod/{args.pod}/force/"
           f"{'true' if args.force else 'false'}")
    data = aiohttp.FormData()
    for u in args.uuid:
        data.add_field("uuids", u)
    return asyncio.run(_http("POST", url, data, token=client_token(args), tls=client_tls(args)))


def cmd_status(args) -> int:
    if args.pod:
        url = f"{args.master.rstrip('/')}/api/v1/namespaces/{args.ns}/pods/{args.pod}/gpus"
    else:
        url = f"{args.master.rstrip('/')}/api/v1/nodes/{args.node}/gpus"
    return asyncio.run(_http("GET", url, token=client_token(args), tls=client_tls(args)))


def disassemble(insns: List[int]) -> List[str]:
    from gpumounter_amd.node import bpfvm

    names = {0x61: "ldxw", 0xbf: "mov64", 0xb7: "mov64", 0x57: "and64", 0x77: "rsh64",
             0x55: "jne", 0x85: "call", 0x95: "exit", 0x18: "lddw"}
    out = []
    skip = False
    for i, raw in enumerate(insns):
        if skip:
            skip = False
            continue
        code, dst, src, off, imm = bpfvm.decode(raw)
        op = names.get(code, f"op{code:#x}")
        if code == 0x61:
            out.append(f"{i:3d}: r{dst} = *(u32 *)(r{src} + {off})")
        elif code == 0xbf:
            out.append(f"{i:3d}: r{dst} = r{src}")
        elif code == 0xb7:
            out.append(f"{i:3d}: r{dst} = {imm}")
        elif code == 0x57:
            out.append(f"{i:3d}: r{dst} &= {imm & 0xffffffff:#x}")
        elif code == 0x77:
            out.append(f"{i:3d}: r{dst} >>= {imm}")
        elif code == 0x55:
            out.append(f"{i:3d}: if r{dst} != {imm} goto +{off}")
        elif code == 0x18:
            out.append(f"{i:3d}: r{dst} = map[prog_array fd={imm}]")
            skip = True
        elif code == 0x85:
            out.append(f"{i:3d}: call bpf_tail_call#{imm}")
        elif code == 0x95:
            out.append(f"{i:3d}: exit")
        else:
            out.append(f"{i:3d}: {op} dst=r{dst} src=r{src} off={off} imm={imm}")
    return out


def cmd_bpf_dump(args) -> int:
    from gpumounter_amd.models.device import DeviceNode
    from gpumounter_amd.node.cgroup import build_program

    nodes = []
    for a in args.allow:
        ma, mi = a.split(":")
        nodes.append(DeviceNode(f"/dev/x{ma}_{mi}", int(ma), int(mi)))
    prog = build_program(nodes, chained=not args.unchained)
    print("\n".join(disassemble(prog)))
    return 0


def cmd_doctor(args) -> int:
    from gpumounter_amd.utils import doctor

    cfg = _cfg(args)
    memtest_bytes = args.memtest if args.memtest is not None else 0   # negative: automatic size
    extra = {}
    if args.host_link is not None:      # negative: the test's default size
        extra["host_link_bytes"] = args.host_link
    if args.atomics_inject and not args.atomics:
        print("doctor: --atomics-inject needs --atomics", file=sys.stderr)
        return 2
    if args.host_sync_inject and not args.host_sync:
        print("doctor: --host-sync-inject needs --host-sync", file=sys.stderr)
        return 2
    if _burn_in_usage(args, "doctor"):
        return 2
    for value, name in ((args.burn_in_format, "burn_in_formats"),
                        (args.burn_in_flip, "burn_in_flip"),
                        (args.burn_in_attribute, "burn_in_attribute"),
                        (args.burn_in_inject, "burn_in_inject")):
        if value:
            extra[name] = value
    if args.atomics:
        extra["atomics"] = True
        if args.atomics_inject:
            extra["atomics_inject"] = args.atomics_inject
    if args.host_sync:
        extra["host_sync"] = True
        if args.host_sync_inject:
            extra["host_sync_inject"] = args.host_sync_inject
    scans = _all_scans()
    for scan in scans:
        error = _scan_usage(scan, args, "doctor")
        if error:
            print(error, file=sys.stderr)
            return 2
        if getattr(args, scan.stem):
            extra[scan.stem] = True
            for name in scan.controls:      # the CU scan's are not on this command line
                if getattr(args, f"{scan.stem}_{name}", None):
                    extra[f"{scan.stem}_{name}"] = getattr(args, f"{scan.stem}_{name}")
    checks = doctor.run(cfg, skip_cluster=args.skip_cluster,
                        gpu=(args.gpu or bool(args.burn_in) or bool(memtest_bytes)
                             or args.host_link is not None or args.atomics or args.host_sync
                             or any(getattr(args, scan.stem) for scan in scans)),
                        burn_in_s=args.burn_in, memtest_bytes=memtest_bytes, **extra)
    print(doctor.render(checks, args.json))
    return 1 if any(c.status == "fail" for c in checks) else 0


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="gpumounter_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("master")
    p.add_argument("--config")
    p.add_argument("--port", type=int)
    p.set_defaults(fn=cmd_master)
    p = sub.add_parser("worker")
    p.add_argument("--config")
    p.add_argument("--node")
    p.add_argument("--port", type=int)
    p.set_defaults(fn=cmd_worker)
    p = sub.add_parser("device-plugin")
    p.add_argument("--config")
    p.add_argument("--amdsmi", default=None)
    p.add_argument("--dir", default="", help="kubelet device-plugin directory")
    p.add_argument("--no-register", action="store_true", help="serve only (testing)")
    p.set_defaults(fn=cmd_device_plugin)
    p = sub.add_parser("inventory")
    p.add_argument("--amdsmi", default="")
    p.add_argument("--processes", action="store_true")
    p.set_defaults(fn=cmd_inventory)
    p = sub.add_parser("topology")
    p.add_argument("--amdsmi", default="")
    p.add_argument("-n", type=int, default=0)
    p.add_argument("--policy", default="xgmi", choices=("xgmi", "first-fit"))
    p.set_defaults(fn=cmd_topology)
    p = sub.add_parser("probe")
    p.add_argument("--bdf", action="append")
    p.add_argument("--full", action="store_true")
    burnin_options.add_options(p, "sustained GEMM load with bit-exact result checks (exit 1 on "
                                  "mismatch)")
    _add_memtest_size(p, "HBM pattern test over SIZE bytes (64M, 8G; default: 90 %% of the free "
                         "memory) of every probed GPU (exit 1 on any bad word)")
    p.add_argument("--memtest-passes", type=int, default=1, metavar="N")
    p.add_argument("--memtest-patterns", type=_memtest_arg("parse_patterns"),
                   default=("addr", "solid", "checker", "walk", "random"), metavar="a,b,...")
    p.add_argument("--memtest-flip", type=_memtest_arg("parse_flip"), default=None,
                   metavar="OFFSET:MASK",
                   help="negative control: corrupt that word after every fill; the test must fail")
    cu, *later = _all_scans()
    _add_probe_scan(p, cu)
    _add_hostlink_size(p, "host link (PCIe) test of every probed GPU over SIZE bytes of pinned "
                          "host memory per buffer (default 256M): checked transfers in both "
                          "directions by the copy engines and by kernels (exit 1 on any bad word)")
    p.add_argument("--host-link-legs", type=_hostlink_arg("parse_legs"), default=None,
                   metavar="a,b,...", help="of h2d,d2h,bidir,kread,kwrite,kduplex (default: all)")
    p.add_argument("--host-link-patterns", type=_hostlink_arg("parse_patterns"), default=None,
                   metavar="a,b,...", help="memtest patterns (default: addr,random)")
    p.add_argument("--host-link-blocks", type=_hostlink_arg("parse_blocks"), default=None,
                   metavar="N", help="grid of the kernel legs (1..1024)")
    p.add_argument("--host-link-flip", type=_hostlink_arg("parse_flip"), default=None,
                   metavar="LEG:OFFSET:MASK",
                   help="negative control: one word of that leg's data arrives XORed with MASK; "
                        "the leg must report it")
    _add_atomics(p, "cross-XCC atomics and coherence test of every probed GPU: known-answer "
                    "atomics, tickets, a CAS loop and in-launch hand-offs between blocks (exit 1 "
                    "on any wrong word, lost or doubled ticket)")
    p.add_argument("--atomics-tests", type=_atomics_arg("parse_tests"), default=None,
                   metavar="a,b,...", help="of add,ticket,cas,handoff (default: all)")
    p.add_argument("--atomics-spread", type=_atomics_arg("parse_spread"), default=None,
                   metavar="N", help="words per table and ticket counters, a power of two "
                                     "1..65536 (default 4096; 1 is one hot word)")
    p.add_argument("--atomics-blocks", type=int, default=None, metavar="N",
                   help="blocks of 256 threads, 1..4096 (default: one per CU)")
    p.add_argument("--atomics-rounds", type=int, default=None, metavar="N",
                   help="hand-off rounds, 1..64 (default 8)")
    _add_hostsync(p, "host-GPU atomics and hand-off test of every probed GPU: system-scope "
                     "atomics on pinned host memory with host threads contending, and "
                     "release/acquire hand-offs through flags in host memory in both directions "
                     "(exit 1 on any wrong, lost or stale word)")
    p.add_argument("--host-sync-tests", type=_hostsync_arg("parse_tests"), default=None,
                   metavar="a,b,...", help="of add,ticket,swap,cas,handoff (default: all)")
    p.add_argument("--host-sync-blocks", type=int, default=None, metavar="N",
                   help="blocks of 256 threads, 1..CUs (default: min(16, CUs))")
    p.add_argument("--host-sync-threads", type=int, default=None, metavar="N",
                   help="host threads, 0..8 (default 2; the hand-off needs one)")
    p.add_argument("--host-sync-rounds", type=int, default=None, metavar="N",
                   help="hand-off rounds, 1..64 (default 8)")
    for scan in later:
        _add_probe_scan(p, scan)
    p.set_defaults(fn=cmd_probe)
    for name, fn in (("add", cmd_add), ("remove", cmd_remove), ("status", cmd_status)):
        p = sub.add_parser(name)
        p.add_argument("--master", default="http://127.0.0.1:8080")
        p.add_argument("--ns", default="default")
        p.add_argument("--pod", default="")
        p.add_argument("--token", default="", help="bearer token for the master (default: "
                       "$GM_TOKEN, --token-file, the service-account token, the kubeconfig "
                       "user's token)")
        p.add_argument("--token-file", default="")
        p.add_argument("--ca", default="", help="CA bundle that signed the master's HTTPS "
                       "certificate (default: $GM_MASTER_CA, else the system roots)")
        p.add_argument("--insecure", action="store_true",
                       help="do not verify the master's HTTPS certificate (labs only)")
        if name == "add":
            p.add_argument("-n", type=int, required=True)
            p.add_argument("--entire", action="store_true")
            p.add_argument("--container", default="")
            p.add_argument("--lease", default="", help="seconds until automatic detach")
        if name == "remove":
            p.add_argument("--uuid", action="append", required=True)
            p.add_argument("--force", action="store_true")
        if name == "status":
            p.add_argument("--node", default="")
        p.set_defaults(fn=fn)
    p = sub.add_parser("doctor", help="node preflight: amdsmi, cgroup/bpf, systemd, kubelet, "
                                      "apiserver")
    p.add_argument("--config")
    p.add_argument("--json", action="store_true")
    p.add_argument("--skip-cluster", action="store_true",
                   help="skip the kubelet and apiserver checks")
    p.add_argument("--gpu", action="store_true",
                   help="also run the gfx950 liveness kernel on every GPU")
    burnin_options.add_options(p, "with --gpu: sustained bit-checked GEMM load per GPU")
    _add_memtest_size(p, "with --gpu: HBM pattern test over SIZE bytes per GPU (default: 90 %% of "
                         "its free memory)")
    _add_doctor_scan(p, cu)
    _add_hostlink_size(p, "with --gpu: host link (PCIe) test of every GPU over SIZE bytes of "
                          "pinned host memory per buffer (default 256M)")
    _add_atomics(p, "with --gpu: cross-XCC atomics and coherence test of every GPU")
    _add_hostsync(p, "with --gpu: host-GPU atomics and hand-off test of every GPU")
    for scan in later:
        _add_doctor_scan(p, scan)
    p.set_defaults(fn=cmd_doctor)
    p = sub.add_parser("bpf-dump")
    p.add_argument("--allow", action="append", default=[])
    p.add_argument("--unchained", action="store_true")
    p.set_defaults(fn=cmd_bpf_dump)
    p = sub.add_parser("config-doc")
    p.add_argument("--metrics", action="store_true", help="the metrics reference instead")
    p.set_defaults(fn=cmd_config_doc)
    return ap


def cmd_config_doc(args) -> int:
    from gpumounter_amd.utils.configdoc import render, render_metrics
    sys.stdout.write(render_metrics() if args.metrics else render())
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    sys.exit(main())
