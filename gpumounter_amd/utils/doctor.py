"""Node preflight: ``python -m gpumounter_amd doctor`` checks everything the worker needs on a node.

The reference has no such tool; its failure modes surface as a failed attach (wrong cgroup driver
env, missing ``mknod`` in the image, no kubelet socket — reference docs/guide/FAQ.md:3-7). Each
check here reports ``ok``, ``warn`` (works, but a feature is degraded) or ``fail`` (attaches
cannot work), with the detail an operator needs. Run it in the worker container (same mounts and
privileges as the DaemonSet) or on the host with the same ``GM_*`` settings.
"""
from __future__ import annotations

import asyncio
import ctypes as C
import errno
import json
import os
from dataclasses import asdict, dataclass
from typing import List

from gpumounter_amd import _native

BPF_FS_MAGIC = 0xCAFE4A11


@dataclass
class Check:
    name: str
    status: str          # ok | warn | fail
    detail: str


def _statfs_type(path: str) -> int:
    class StatFs(C.Structure):
        _fields_ = [("f_type", C.c_long), ("rest", C.c_byte * 120)]

    libc = C.CDLL(None, use_errno=True)
    buf = StatFs()
    if libc.statfs(path.encode(), C.byref(buf)) != 0:
        raise OSError(C.get_errno(), os.strerror(C.get_errno()), path)
    return buf.f_type & 0xFFFFFFFF


def check_inventory(cfg) -> List[Check]:
    from gpumounter_amd.hw.inventory import Inventory

    try:
        inv = Inventory(cfg.amdsmi_lib, cfg.kfd_major, cfg.kfd_dev_path)
        gpus = inv.gpus()
    except Exception as e:  # noqa: BLE001
        return [Check("amdsmi", "fail", f"inventory unavailable: {e}")]
    out = [Check("amdsmi", "ok" if gpus else "fail",
                 f"{len(gpus)} GPU(s) via {inv.lib_path}: "
                 + ", ".join(sorted({g.gfx_target for g in gpus})))]
    hives = {g.xgmi_hive_id for g in gpus}
    out.append(Check("xgmi", "ok" if len(gpus) < 2 or len(hives) == 1 else "warn",
                     f"{len(hives)} hive(s) for {len(gpus)} GPU(s)"))
    kfd_src = "configured" if cfg.kfd_major else (
        cfg.kfd_dev_path if os.path.exists(cfg.kfd_dev_path) else "fallback 511")
    out.append(Check("kfd", "ok" if kfd_src != "fallback 511" else "warn",
                     f"/dev/kfd major {inv.kfd_major} ({kfd_src})"))
    return out


def check_cgroup(cfg) -> List[Check]:
    from gpumounter_amd.node.cgroup import CgroupResolver

    root = cfg.cgroup_root
    if not os.path.isdir(root):
        return [Check("cgroup", "fail", f"{root} is not mounted")]
    mode = CgroupResolver.detect_mode(root) if cfg.cgroup_mode == "auto" else cfg.cgroup_mode
    out = []
    if mode == "v1":
        allow = os.path.join(root, "devices", "devices.allow")
        ok = os.access(allow, os.W_OK)
        out.append(Check("cgroup", "ok" if ok else "fail",
                         f"v1 devices controller, {allow} {'writable' if ok else 'NOT writable'}"))
        return out
    out.append(Check("cgroup", "ok", f"v2 unified hierarchy at {root}"))
    # can this process load a device program? (CAP_BPF + CAP_SYS_ADMIN in the DaemonSet)
    from gpumounter_amd.node.cgroup import _rule_array, rules_for
    from gpumounter_amd.models.device import DeviceNode

    lib = _native.host()
    rules = rules_for([DeviceNode("/dev/null", 1, 3)], allow=True)
    need = -lib.gm_bpf_dev_build(_rule_array(rules), 1, 0, -1, None, 0)
    buf = (C.c_uint64 * need)()
    n = lib.gm_bpf_dev_build(_rule_array(rules), 1, 0, -1, buf, need)
    fd = lib.gm_bpf_dev_load(buf, n, b"gm_doctor", None, 0)
    if fd >= 0:
        os.close(fd)
        out.append(Check("bpf", "ok", "BPF_PROG_TYPE_CGROUP_DEVICE programs load"))
    else:
        out.append(Check("bpf", "fail", f"cannot load a device program: {os.strerror(-fd)} "
                                        "(needs CAP_BPF/CAP_SYS_ADMIN: privileged DaemonSet)"))
    if fd >= 0 and cfg.bpf_set_mode:
        rc = lib.gm_bpf_dev_probe_set()
        out.append(Check("bpf-set", "ok" if rc == 0 else "warn",
                         "allow-set programs load (grants are map updates)" if rc == 0 else
                         f"allow-set program refused ({os.strerror(-rc)}): set "
                         "GM_BPF_SET_MODE=false for straight-line programs"))
    pin = cfg.bpf_pin_dir
    if pin:
        parent = pin if os.path.isdir(pin) else os.path.dirname(pin)
        try:
            is_bpffs = _statfs_type(parent) == BPF_FS_MAGIC
        except OSError as e:
            is_bpffs = False
            parent = f"{parent} ({e.strerror})"
        out.append(Check("bpffs", "ok" if is_bpffs else "warn",
                         f"{parent} is {'a' if is_bpffs else 'not a'} bpffs: tail-call maps "
                         + ("survive worker restarts" if is_bpffs else
                            "are kept in-process only (lost on restart until reconciled)")))
    return out


def check_devnodes(cfg) -> List[Check]:
    """User-namespaced Pods (hostUsers: false) get bind-mounted nodes (open_tree + move_mount,
    node/devnodes.py), which needs CAP_SYS_ADMIN and a ≥5.2 kernel."""
    if cfg.devnode_userns == "off" or cfg.devnode_mode == "emulate":
        return [Check("devnodes-userns", "ok", f"bind mode not used (devnode_userns="
                                               f"{cfg.devnode_userns}, mode={cfg.devnode_mode})")]
    rc = _native.host().gm_devnodes_bind_probe()
    if rc == 0:
        return [Check("devnodes-userns", "ok", "open_tree/move_mount available: user-namespaced "
                                               "Pods get bind-mounted device nodes")]
    return [Check("devnodes-userns", "warn",
                  f"open_tree refused ({os.strerror(-rc)}): attaches to user-namespaced Pods "
                  "(hostUsers: false) will fail; other Pods are unaffected")]


def check_pidns(cfg) -> List[Check]:
    """Busy detection's process tables (KFD's and amdsmi's) name host-namespace PIDs
    (``profiles/r6_kfd_probe/``); the worker uses them only in the host PID namespace."""
    from gpumounter_amd.node import procs

    host = procs.host_pid_ns()
    table = ""
    if cfg.kfd_proc_path:
        try:
            n = len({p for t in procs.kfd_table(cfg.kfd_proc_path).values() for p in t})
            table = f"; KFD process table readable ({n} process(es) on a GPU)"
        except OSError as e:
            table = f"; KFD process table {cfg.kfd_proc_path}: {e.strerror} (amdsmi's is used)"
    if host:
        return [Check("pidns", "ok", "host PID namespace (hostPID): busy detection can use the "
                                     "KFD/amdsmi process tables" + table)]
    return [Check("pidns", "warn",
                  "not in the host PID namespace: busy detection relies on the render-fd scan "
                  "alone (the KFD/amdsmi tables name host PIDs); run the DaemonSet with "
                  "hostPID: true" + table)]


def check_systemd(cfg) -> List[Check]:
    from gpumounter_amd.node import systemd

    if cfg.systemd_device_allow == "off":
        return [Check("systemd", "ok", "DeviceAllow persistence disabled")]
    bus = systemd.find_bus(cfg.systemd_bus)
    if bus is None:
        status = "fail" if cfg.systemd_device_allow == "on" else (
            "warn" if cfg.cgroup_driver == "systemd" else "ok")
        detail = ("no systemd bus socket mounted (/run/systemd or /run/dbus): on "
                  "systemd-driver nodes a daemon-reload can drop hot-mounted devices until the "
                  "reconciler restores them") if status != "ok" else \
            "no systemd bus socket (needed only with the systemd cgroup driver)"
        return [Check("systemd", status, detail)]
    err = C.create_string_buffer(256)
    out = C.create_string_buffer(1 << 12)
    rc = _native.host().gm_sd_get_device_allow(bus.encode(), b"-.slice", out, 1 << 12, err, 256)
    if rc >= 0 or rc == -errno.EPROTO:   # a D-Bus answer (even an error) means we are talking
        return [Check("systemd", "ok", f"systemd reachable on {bus}")]
    return [Check("systemd", "warn", f"{bus}: {err.value.decode() or os.strerror(-rc)}")]


async def _check_dra(cfg) -> List[Check]:
    """gpu_allocation=dra: the node's ResourceSlice must publish its GPUs with a PCI address
    the worker can map to amdsmi's inventory."""
    from gpumounter_amd.cluster.kube import KubeClient
    from gpumounter_amd.hw.inventory import Inventory
    from gpumounter_amd.models.device import normalize_device_id
    from gpumounter_amd.node.dra import DraLedger

    try:
        kube = KubeClient.from_config(cfg)
    except Exception as e:  # noqa: BLE001
        return [Check("dra", "fail", f"no credentials: {e}")]
    led = DraLedger(kube, cfg.node_name, cfg.dra_driver, cfg.dra_device_class,
                    cfg.dra_bdf_attribute)
    try:
        devs = await led.allocatable()
        allocs = await led.list()
    except Exception as e:  # noqa: BLE001
        return [Check("dra", "fail", f"resource.k8s.io/v1: {e}")]
    finally:
        await kube.close()
    if not devs:
        return [Check("dra", "fail", f"no ResourceSlice device of driver {cfg.dra_driver} on "
                                     f"{cfg.node_name} carries a PCI address "
                                     f"(attribute {cfg.dra_bdf_attribute!r})")]
    try:
        have = {normalize_device_id(g.bdf) for g in Inventory(
            cfg.amdsmi_lib, cfg.kfd_major, cfg.kfd_dev_path).gpus()}
    except Exception:  # noqa: BLE001 - reported by the amdsmi check
        have = set()
    unknown = [d for d in devs if have and normalize_device_id(d) not in have]
    if unknown:
        return [Check("dra", "warn", f"ResourceSlice devices not in the amdsmi inventory: "
                                     f"{unknown}")]
    return [Check("dra", "ok", f"{len(devs)} {cfg.dra_driver} device(s) in ResourceSlices, "
                               f"{len(allocs)} claim reservation(s) on this node")]


async def _check_kubelet(cfg) -> List[Check]:
    from gpumounter_amd.node.ledger import LedgerClient

    if getattr(cfg, "gpu_allocation", "device-plugin") == "dra":
        return await _check_dra(cfg)
    if not os.path.exists(cfg.kubelet_socket):
        return [Check("kubelet", "fail", f"PodResources socket {cfg.kubelet_socket} missing")]
    lc = LedgerClient(cfg.kubelet_socket, cfg.resource_name, cfg.kubelet_timeout_s,
                      cfg.podresources_api)
    try:
        allocs = await lc.list()
        alloc = await lc.allocatable()
        return [Check("kubelet", "ok",
                      f"PodResources {lc.api_version}: {len(allocs)} {cfg.resource_name} "
                      f"allocation(s)" + (f", {len(alloc)} allocatable" if alloc else ""))]
    except Exception as e:  # noqa: BLE001
        return [Check("kubelet", "fail", f"PodResources List failed: {e}")]
    finally:
        await lc.close()


async def _check_apiserver(cfg) -> List[Check]:
    from gpumounter_amd.cluster.kube import KubeClient

    try:
        kube = KubeClient.from_config(cfg)
    except Exception as e:  # noqa: BLE001
        return [Check("apiserver", "fail", f"no credentials: {e}")]
    try:
        pods, _ = await kube.list_pods(cfg.pool_namespace)
        out = [Check("apiserver", "ok", f"{kube.base}: {len(pods)} pod(s) in "
                                        f"{cfg.pool_namespace}")]
    except Exception as e:  # noqa: BLE001
        await kube.close()
        return [Check("apiserver", "fail", f"{kube.base}: {e}")]
    try:
        return out + await _check_priority(cfg, kube)
    finally:
        await kube.close()


async def _check_priority(cfg, kube) -> List[Check]:
    """The placeholders' floor PriorityClass exists (and the pool's, when one is set). Without
    it placeholders rank as their tenants do, and a higher-priority Pod can preempt a
    placeholder — revoking a GPU a tenant is using."""
    from gpumounter_amd.cluster.kube import NotFound

    out = []
    for what, name in (("placeholder", cfg.placeholder_priority_class),
                       ("pool", getattr(cfg, "pool_priority_class", ""))):
        if not name:
            if what == "placeholder":
                out.append(Check("priority", "warn", "no placeholder_priority_class: "
                                 "placeholders rank as their tenants"))
            continue
        try:
            pc = await kube.get_priority_class(name)
        except NotFound:
            out.append(Check("priority", "fail", f"{what} PriorityClass {name} missing "
                                                 f"(kubectl apply -f deploy/placeholder-"
                                                 f"priority.yaml)"))
            continue
        except Exception as e:  # noqa: BLE001
            out.append(Check("priority", "warn", f"{what} PriorityClass {name}: {e}"))
            continue
        out.append(Check("priority", "ok", f"{what} PriorityClass {name}: value "
                                           f"{pc.get('value')}, preemptionPolicy "
                                           f"{pc.get('preemptionPolicy', 'PreemptLowerPriority')}"))
    return out


def _scan_segment(scan, dev: int, given) -> tuple:
    """(what one per-CU scan adds to a GPU's detail line, whether it fails the check); ``given``
    holds check_gpus' parameters: the scan runs only if its switch is on."""
    if not given[scan.stem]:
        return "", False
    r = scan.run(dev, **{f"_{name}": given[f"{scan.stem}_{name}"] for name in scan.controls})
    counted = "" if scan.plain_cli else f" {len(r[scan.selection])} {scan.selection}"
    text = (f", {scan.label}{counted} {r['cus_seen']}/{r['cus_expected']} CUs in {r['rounds']} "
            f"round(s) {r['kernel_ms']:.2f} ms {r['words_in_error']} wrong words")
    if not r["complete"]:
        text += " (incomplete: not every CU was reached)"
    if not r["ok"]:
        text += f", failed: {scan.describe_failed(r)}"
    return text, not r["ok"]


def check_gpus(cfg, burn_in_s: float = 0.0, *, memtest_bytes: int = 0,
               memtest_flip=None, burn_in_flip=None, cu_scan: bool = False,
               cu_scan_inject=None, host_link_bytes: int = 0,
               host_link_flip=None, atomics: bool = False,
               atomics_inject=None, mfma_scan: bool = False,
               mfma_scan_inject=None, lane_scan: bool = False,
               lane_scan_inject=None, cache_scan: bool = False,
               cache_scan_inject=None, cache_scan_poke=None,
               burn_in_formats=("bf16",), lds_scan: bool = False,
               lds_scan_inject=None, lds_scan_poke=None, burn_in_attribute: bool = False,
               burn_in_inject=None, sparse_scan: bool = False,
               sparse_scan_inject=None, host_sync: bool = False,
               host_sync_inject=None) -> List[Check]:
    """Run the gfx950 probe kernels on every GPU of the node (``doctor --gpu``): each amdsmi GPU
    must be visible to HIP and pass the wave64 liveness kernel. With ``burn_in_s`` also a
    sustained bit-checked GEMM load per GPU, once per format in ``burn_in_formats`` (bf16, and the
    block-scaled mxfp8 and mxfp4 of :func:`gpumounter_amd.ops.mxgemm.burn_in`); a format with a
    mismatching word fails the check and is named. With ``memtest_bytes`` also the HBM pattern
    test over that many bytes per GPU (negative: 90 % of what is free on it); ``memtest_flip``
    = (offset, mask) is its negative control, ``burn_in_flip`` = [(element, mask), ...] the
    burn-in's (see :func:`probe.burn_in`). With ``burn_in_attribute`` the burn-ins rotate their
    tiles over the CUs and a failing one names the units it blames, as the scans name theirs, with
    their role and the format; ``burn_in_inject`` = (id or "first", mask) is that mode's negative
    control. With ``cu_scan`` also the per-CU self-test
    (:func:`gpumounter_amd.ops.cuscan.scan`): a CU with a wrong word fails the check and is named;
    a scan that did not reach every CU is stated and does not fail it; ``cu_scan_inject`` is its
    negative control. With ``host_link_bytes`` also the host link (PCIe) test
    (:func:`gpumounter_amd.ops.hostlink.hostlink`) over that many bytes of pinned host memory per
    buffer (negative: its default size): a wrong word or a refused pin fails the check, a link
    that stayed below its maximum speed or width under load is a warning; ``host_link_flip`` =
    (leg, offset, mask) is its negative control. With ``atomics`` also the cross-XCC atomics and
    coherence test (:func:`gpumounter_amd.ops.atomics.run`): a wrong table word, a lost or doubled
    ticket, a given-up CAS or a stale or lost hand-off word fails the check and is named; hand-offs
    not seen within the budget do not, but when none at all was seen the check warns that the
    hand-off proved nothing; ``atomics_inject`` is its negative control. With ``mfma_scan`` also
    the per-CU matrix-core format scan (:func:`gpumounter_amd.ops.mfmascan.scan`): a CU with a
    wrong accumulator word fails the check and is named as the CU scan names it, with the format;
    ``mfma_scan_inject`` is its negative control. With ``lane_scan`` also the per-CU register,
    lane and scalar-unit scan (:func:`gpumounter_amd.ops.lanescan.scan`): a CU with a wrong
    signature word fails the check and is named the same way, with the test; a scan that did not
    reach every CU is stated, not failed; ``lane_scan_inject`` is its negative control. With
    ``cache_scan`` also the per-CU cache scan (:func:`gpumounter_amd.ops.cachescan.scan`: vector
    L1, L2, scalar and instruction caches), failed, named and stated in the same way;
    ``cache_scan_inject`` and ``cache_scan_poke`` are its negative controls. With ``lds_scan``
    also the per-CU LDS scan (:func:`gpumounter_amd.ops.ldsscan.scan`: access widths, LDS atomics,
    bank crossbar, transposing read, global-to-LDS loads), failed, named and stated in the same
    way; ``lds_scan_inject`` and ``lds_scan_poke`` are its negative controls. With ``sparse_scan``
    also the per-CU sparse and 32x32 matrix-core scan (:func:`gpumounter_amd.ops.sparsescan.scan`:
    the 2:4 ``v_smfmac_*`` forms), after the LDS scan, failed, named with the format and stated in
    the same way; ``sparse_scan_inject`` is its negative control. With ``host_sync``
    also the host-GPU atomics and hand-off test (:func:`gpumounter_amd.ops.hostsync.run`), after
    the atomics test: a wrong table word, a lost or doubled ticket, a missing, doubled or foreign
    swap value, a given-up CAS or a stale or lost hand-off word fails the check and names the
    test, the direction and the first record; hand-offs not seen within the budgets do not, but
    the check warns when a direction saw none at all, and when the device reports no native host
    atomics so that the atomic tests were skipped; ``host_sync_inject`` is its negative control.
    A GPU that fails here should not be handed out."""
    given = dict(locals())            # the scans' switches and controls, by parameter name
    from gpumounter_amd.hw.inventory import Inventory
    from gpumounter_amd.ops import cuframe, mxgemm, probe

    cu, *later = cuframe.all_scans()  # the CU scan: before the host-link and atomics tests
    try:
        n = probe.device_count()
    except Exception as e:  # noqa: BLE001 - no HIP runtime / driver
        return [Check("gpu", "fail", f"HIP unavailable: {e}")]
    if n == 0:
        return [Check("gpu", "fail", "no GPU visible to HIP")]
    try:
        want = [g.bdf for g in Inventory(cfg.amdsmi_lib, cfg.kfd_major,
                                         cfg.kfd_dev_path).gpus()]
    except Exception:  # noqa: BLE001 - reported by the amdsmi check
        want = []
    out: List[Check] = []
    seen = set()
    for d in range(n):
        try:
            pr = probe.props(d)
            seen.add(pr["pci_bus_id"])
            cold = probe.quick(d)          # includes loading the code object
            us = probe.quick(d)
            arch = pr["gcn_arch"].split(":")[0]
            detail = (f"{pr['pci_bus_id']} {arch}: liveness kernel {us:.0f} µs "
                      f"(first launch {cold / 1e3:.0f} ms)")
            status = "ok" if arch == "gfx950" else "warn"
            for fmt in burn_in_formats if burn_in_s > 0 else ():
                b = mxgemm.run_burn_in(d, burn_in_s, fmt, _flips=burn_in_flip,
                                       **mxgemm.attribute_kwargs(burn_in_attribute,
                                                                 burn_in_inject))
                detail += (f", burn-in {'' if fmt == 'bf16' else fmt + ' '}{b['seconds']:g} s "
                           f"{b['tflops']:.0f} TF/s {b['mismatches']} mismatching words")
                if "attribution" in b:
                    a = b["attribution"]
                    detail += (f", {a['tiles']} tiles over {a['cus_seen']} CUs, "
                               f"{a['tiles_moved']} moved")
                if not b["ok"]:
                    detail += "" if fmt == "bf16" else f", failed: {fmt} burn-in"
                    if "attribution" in b:
                        detail += (f", {fmt} burn-in blames: {probe.describe_blamed(b)}"
                                   + (" (log overflowed: only the logged events are blamed)"
                                      if b["attribution"]["log_overflow"] else ""))
                    status = "fail"
            if memtest_bytes:
                from gpumounter_amd.ops import memtest

                m = memtest.memtest(d, memtest_bytes if memtest_bytes > 0 else None,
                                    _flip=memtest_flip)
                detail += (f", memtest {m['bytes'] / 2**30:.2f} GiB {m['read_gbps']:.0f} / "
                           f"{m['write_gbps']:.0f} GB/s {m['errors']} bad words")
                status = status if m["ok"] else "fail"
            text, failed = _scan_segment(cu, d, given)
            detail, status = detail + text, "fail" if failed else status
            if host_link_bytes:
                from gpumounter_amd.ops import hostlink

                try:
                    h = hostlink.hostlink(d, host_link_bytes if host_link_bytes > 0 else None,
                                          _flip=host_link_flip)
                except hostlink.HostlinkError as e:
                    detail += f", host-link failed: {e}"
                    status = "fail"
                else:
                    rates = " ".join(f"{n} {leg['gbps']:.1f}" for n, leg in h["legs"].items())
                    detail += (f", host-link {h['bytes'] / 2**20:.0f} MiB GB/s {rates}, "
                               f"{h['errors']} wrong words")
                    if not h["ok"]:
                        detail += f", failed: {hostlink.describe_errors(h)}"
                        status = "fail"
                    if h["link"]["degraded"]:
                        detail += (f", link below its maximum under load: "
                                   f"{hostlink.describe_link(h['link'])}")
                        status = "warn" if status == "ok" else status
            if atomics:
                from gpumounter_amd.ops import atomics as at

                a = at.run(d, _inject=atomics_inject)
                detail += (f", atomics {'+'.join(a['tests'])} {a['blocks']} blocks on "
                           f"{a['xccs_seen']} XCCs {a['seconds'] * 1e3:.0f} ms "
                           f"{a['words_in_error']} wrong words, hand-offs "
                           f"{a['observed']}/{a['handoffs']} seen "
                           f"({a['observed_cross_xcc']} across XCCs)")
                if not a["ok"]:
                    detail += f", failed: {at.describe_failed(a)}"
                    status = "fail"
                elif a["handoff_vacuous"]:
                    detail += ", no hand-off was seen within the budget: it proved nothing"
                    status = "warn" if status == "ok" else status
            if host_sync:
                from gpumounter_amd.ops import hostsync as hs

                h = hs.run(d, _inject=host_sync_inject)
                detail += (f", host-sync {'+'.join(h['tests'])} {h['blocks']} blocks and "
                           f"{h['host_threads']} host threads {h['seconds'] * 1e3:.0f} ms "
                           f"{h['words_in_error']} wrong words, hand-offs "
                           f"{h['h2d']['observed']}/{h['h2d']['handoffs']} seen by the GPU "
                           f"{h['d2h']['observed']}/{h['d2h']['handoffs']} by the host")
                if not h["ok"]:
                    detail += f", failed: {hs.describe_failed(h)}"
                    status = "fail"
                else:
                    if h["handoff_vacuous"]:
                        detail += (", a direction saw no hand-off within its budget: it proved "
                                   "nothing there")
                        status = "warn" if status == "ok" else status
                    if h["tests_skipped"]:
                        detail += (f", skipped {'+'.join(h['tests_skipped'])}: "
                                   f"{hs.NO_ATOMICS}")
                        status = "warn" if status == "ok" else status
            for scan in later:
                text, failed = _scan_segment(scan, d, given)
                detail, status = detail + text, "fail" if failed else status
            out.append(Check(f"gpu{d}", status, detail))
        except Exception as e:  # noqa: BLE001 - a faulting GPU is exactly what this finds
            out.append(Check(f"gpu{d}", "fail", f"probe failed: {e}"))
    missing = [b for b in want if b.lower() not in seen]
    if missing:
        out.append(Check("gpu", "warn", f"amdsmi GPUs not visible to HIP here: {missing}"))
    return out


def run(cfg, skip_cluster: bool = False, gpu: bool = False,
        burn_in_s: float = 0.0, *, memtest_bytes: int = 0, cu_scan: bool = False,
        host_link_bytes: int = 0, atomics: bool = False, atomics_inject=None,
        mfma_scan: bool = False, mfma_scan_inject=None, lane_scan: bool = False,
        lane_scan_inject=None, cache_scan: bool = False, cache_scan_inject=None,
        cache_scan_poke=None, burn_in_formats=None, burn_in_flip=None,
        lds_scan: bool = False, lds_scan_inject=None, lds_scan_poke=None,
        burn_in_attribute: bool = False, burn_in_inject=None, sparse_scan: bool = False,
        sparse_scan_inject=None, host_sync: bool = False,
        host_sync_inject=None) -> List[Check]:
    given = dict(locals())            # the scans' switches and controls, by parameter name
    from gpumounter_amd.ops import cuframe

    checks = check_inventory(cfg) + check_cgroup(cfg) + check_devnodes(cfg) + \
        check_pidns(cfg) + check_systemd(cfg)
    if gpu:
        extra = {}
        if burn_in_formats is not None:
            extra["burn_in_formats"] = burn_in_formats
        if burn_in_flip is not None:
            extra["burn_in_flip"] = burn_in_flip
        if burn_in_attribute:
            extra["burn_in_attribute"] = True
        if burn_in_inject is not None:
            extra["burn_in_inject"] = burn_in_inject
        if host_link_bytes:
            extra["host_link_bytes"] = host_link_bytes
        if atomics:
            extra["atomics"] = True
            if atomics_inject is not None:
                extra["atomics_inject"] = atomics_inject
        if host_sync:
            extra["host_sync"] = True
            if host_sync_inject is not None:
                extra["host_sync_inject"] = host_sync_inject
        for scan in cuframe.all_scans():
            if given[scan.stem]:
                extra[scan.stem] = True
                for name in scan.controls:     # the CU scan's are not among the parameters
                    if given.get(f"{scan.stem}_{name}") is not None:
                        extra[f"{scan.stem}_{name}"] = given[f"{scan.stem}_{name}"]
        checks += check_gpus(cfg, burn_in_s, memtest_bytes=memtest_bytes, **extra)
    if not skip_cluster:
        async def both():
            return await _check_kubelet(cfg) + await _check_apiserver(cfg)
        checks += asyncio.run(both())
    checks.append(Check("roctx", "ok" if _native.host().gm_roctx_available() else "warn",
                        "rocprofiler roctx markers " + (
                            "available" if _native.host().gm_roctx_available()
                            else "unavailable (attach/detach ranges not traced)")))
    return checks


def render(checks: List[Check], as_json: bool = False) -> str:
    if as_json:
        return json.dumps([asdict(c) for c in checks], indent=1)
    w = max(len(c.name) for c in checks)
    return "\n".join(f"{c.status.upper():4}  {c.name:<{w}}  {c.detail}" for c in checks)
