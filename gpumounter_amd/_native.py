"""ctypes bindings to the in-tree native libraries (built by ``native/Makefile`` into ``_lib/``).

* ``libgm_smi.so``      — amdsmi inventory shim        (native/include/gm_smi.h)
* ``libamd_smi_mock.so``— amdsmi stand-in for CPU hosts (native/src/amdsmi_mock.cpp)
* ``libgm_host.so``     — cgroup v1/v2, device nodes, processes, roctx (native/include/gm_host.h)
* ``libgm_probe.so``    — gfx950 HIP validation kernels (native/include/gm_probe.h)

Nothing here falls back silently: a missing library raises :class:`NativeError` with the build
command to run. The struct layouts below must match the C headers field-for-field.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading
from typing import Optional

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib")
NATIVE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "native")

_lock = threading.Lock()
_libs: dict = {}


class NativeError(RuntimeError):
    pass


def lib_path(name: str) -> str:
    return os.path.join(LIB_DIR, name)


def build(target: str = "all", quiet: bool = True) -> None:
    """Run the native Makefile (``host`` needs only g++; ``all`` also needs hipcc). Processes
    that autobuild at the same time (daemons started together in a fresh tree) take turns on
    a lock file; the Makefile renames each library into place whole."""
    import fcntl
    cmd = ["make", "-C", NATIVE_DIR, target, f"-j{min(8, os.cpu_count() or 1)}"]
    os.makedirs(LIB_DIR, exist_ok=True)
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        res = subprocess.run(cmd, capture_output=quiet, text=True)
    if res.returncode != 0:
        raise NativeError(f"native build failed ({' '.join(cmd)}):\n{res.stdout}\n{res.stderr}")


def _load(name: str, autobuild_target: Optional[str]) -> C.CDLL:
    with _lock:
        if name in _libs:
            return _libs[name]
        path = lib_path(name)
        if not os.path.exists(path) and autobuild_target and os.environ.get("GM_NO_AUTOBUILD") != "1":
            build(autobuild_target)
        if not os.path.exists(path):
            raise NativeError(f"{path} missing — run `make -C native` (or __graft_entry__.build())")
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL if name == "libamd_smi_mock.so" else C.RTLD_LOCAL)
        _libs[name] = lib
        return lib


# ------------------------------------------------------------------------------ gm_smi
class GpuInfo(C.Structure):
    _fields_ = [
        ("index", C.c_uint32), ("render_minor", C.c_uint32), ("card_minor", C.c_uint32),
        ("hsa_id", C.c_uint32), ("hip_id", C.c_uint32), ("kfd_node_id", C.c_uint32),
        ("partition_id", C.c_uint32), ("xgmi_lanes", C.c_uint32), ("numa_node", C.c_int32),
        ("num_cu", C.c_uint32), ("bdf_id", C.c_uint64), ("kfd_gpu_id", C.c_uint64),
        ("xgmi_hive_id", C.c_uint64), ("xgmi_node_id", C.c_uint64), ("vram_bytes", C.c_uint64),
        ("device_id", C.c_uint64), ("uuid", C.c_char * 64), ("bdf", C.c_char * 32),
        ("market_name", C.c_char * 128), ("gfx_target", C.c_char * 32),
        ("compute_partition", C.c_char * 16), ("memory_partition", C.c_char * 16),
    ]


class ProcInfo(C.Structure):
    _fields_ = [("pid", C.c_uint32), ("cu_occupancy", C.c_uint32), ("vram_bytes", C.c_uint64),
                ("gtt_bytes", C.c_uint64), ("name", C.c_char * 64)]


class LinkInfo(C.Structure):
    _fields_ = [("link_type", C.c_uint32), ("reserved", C.c_uint32), ("hops", C.c_uint64),
                ("weight", C.c_uint64)]


def smi() -> C.CDLL:
    lib = _load("libgm_smi.so", "host")
    if not getattr(lib, "_gm_typed", False):
        lib.gm_smi_open.argtypes = [C.c_char_p]
        lib.gm_smi_count.argtypes = [C.POINTER(C.c_uint32)]
        lib.gm_smi_gpu_info.argtypes = [C.c_uint32, C.POINTER(GpuInfo)]
        lib.gm_smi_all_gpu_info.argtypes = [C.POINTER(GpuInfo), C.c_uint32, C.POINTER(C.c_uint32)]
        lib.gm_smi_link.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(LinkInfo)]
        lib.gm_smi_link_matrix.argtypes = [C.POINTER(LinkInfo), C.c_uint32]
        lib.gm_smi_process_list.argtypes = [C.c_uint32, C.POINTER(ProcInfo), C.c_uint32,
                                            C.POINTER(C.c_uint32)]
        lib.gm_smi_ecc.argtypes = [C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64)]
        lib.gm_smi_strerror.argtypes = [C.c_int]
        lib.gm_smi_strerror.restype = C.c_char_p
        lib.gm_smi_lib_path.restype = C.c_char_p
        lib._gm_typed = True
    return lib


def mock_smi_path() -> str:
    _load("libamd_smi_mock.so", "host")
    return lib_path("libamd_smi_mock.so")


def mock_smi() -> C.CDLL:
    lib = _load("libamd_smi_mock.so", "host")
    lib.gm_mock_set_procs_file.argtypes = [C.c_char_p]
    lib.gm_mock_set_ecc.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
    return lib


# ------------------------------------------------------------------------------ gm_host
class DevRule(C.Structure):
    _fields_ = [("type", C.c_char), ("access", C.c_uint8), ("allow", C.c_uint8),
                ("pad", C.c_uint8), ("major", C.c_int32), ("minor", C.c_int32)]


class DevNode(C.Structure):
    _fields_ = [("path", C.c_char * 112), ("major", C.c_uint32), ("minor", C.c_uint32),
                ("mode", C.c_uint32), ("uid", C.c_int32), ("gid", C.c_int32)]


class BpfTiming(C.Structure):
    _fields_ = [("query_ns", C.c_uint64), ("map_ns", C.c_uint64), ("build_ns", C.c_uint64),
                ("load_ns", C.c_uint64), ("attach_ns", C.c_uint64), ("programs", C.c_uint32),
                ("insns", C.c_uint32)]


HOST_ABI_VERSION = 6          # native/include/gm_host.h GM_HOST_ABI_VERSION
GM_ACC_MKNOD, GM_ACC_READ, GM_ACC_WRITE = 1, 2, 4
GM_DEV_EMULATE, GM_DEV_VIA_SETNS, GM_DEV_REPLACE, GM_DEV_BIND = 1, 2, 4, 8


def host() -> C.CDLL:
    lib = _load("libgm_host.so", "host")
    if not getattr(lib, "_gm_typed", False):
        abi = lib.gm_host_abi_version()
        if abi != HOST_ABI_VERSION:
            raise RuntimeError(f"libgm_host.so ABI {abi} != {HOST_ABI_VERSION} expected: stale "
                               f"build, run `make -C native`")
        lib.gm_cg1_apply.argtypes = [C.c_char_p, C.POINTER(DevRule), C.c_int]
        lib.gm_cg1_format_rule.argtypes = [C.POINTER(DevRule), C.c_char_p, C.c_int]
        lib.gm_bpf_dev_build.argtypes = [C.POINTER(DevRule), C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_uint64), C.c_int]
        lib.gm_bpf_dev_load.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_char_p, C.c_char_p,
                                        C.c_int]
        lib.gm_bpf_dev_query.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32,
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.gm_bpf_prog_name.argtypes = [C.c_uint32, C.c_char_p, C.c_int]
        lib.gm_bpf_dev_program.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.gm_bpf_dev_program_at.argtypes = [C.c_char_p, C.c_uint32, C.c_int,
                                              C.POINTER(C.c_uint64),
                                              C.c_uint32, C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.gm_bpf_dev_install.argtypes = [C.c_char_p, C.POINTER(DevRule), C.c_int,
                                           C.POINTER(DevRule), C.c_int, C.c_char_p,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.gm_bpf_dev_restore.argtypes = [C.c_char_p, C.c_char_p]
        lib.gm_bpf_dev_build_set.argtypes = [C.c_int, C.POINTER(DevRule), C.c_int, C.c_int,
                                             C.c_int, C.POINTER(C.c_uint64), C.c_int]
        lib.gm_bpf_dev_probe_set.argtypes = []
        lib.gm_devnodes_bind_probe.argtypes = []
        lib.gm_bpf_dev_straight_line.argtypes = [C.c_int]
        lib.gm_bpf_dev_straight_line.restype = None
        lib.gm_bpf_dev_set_at.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32),
                                          C.c_uint32, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]
        lib.gm_bpf_dev_last_timing.argtypes = [C.POINTER(BpfTiming)]
        lib.gm_bpf_dev_last_timing.restype = None
        lib.gm_devnodes_create.argtypes = [C.c_int, C.c_char_p, C.POINTER(DevNode), C.c_int,
                                           C.c_int, C.POINTER(C.c_int)]
        lib.gm_devnodes_remove.argtypes = lib.gm_devnodes_create.argtypes
        lib.gm_devnodes_guard.argtypes = [C.c_char_p]
        lib.gm_devnodes_stage.argtypes = [C.c_char_p, C.c_int]
        lib.gm_devnode_stat.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.gm_devnodes_present.argtypes = [C.c_int, C.c_char_p, C.POINTER(DevNode), C.c_int,
                                            C.c_int, C.POINTER(C.c_uint8)]
        lib.gm_proc_dev_users.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_int,
                                          C.POINTER(C.c_int)]
        lib.gm_proc_scan_devs.argtypes = [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint32),
                                          C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
        lib.gm_proc_filter_dev_users.argtypes = [C.POINTER(C.c_int32), C.c_int, C.c_uint32,
                                                 C.c_uint32, C.POINTER(C.c_int32)]
        lib.gm_proc_read_pids.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_int,
                                          C.POINTER(C.c_int)]
        lib.gm_sd_get_device_allow.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                               C.c_char_p, C.c_int]
        lib.gm_sd_set_device_allow.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p),
                                               C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                               C.c_char_p, C.c_int]
        lib.gm_sd_unit_path.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        lib.gm_roctx_push.argtypes = [C.c_char_p]
        lib.gm_roctx_mark.argtypes = [C.c_char_p]
        lib.gm_roctx_start.argtypes = [C.c_char_p]
        lib.gm_roctx_start.restype = C.c_uint64
        lib.gm_roctx_stop.argtypes = [C.c_uint64]
        lib.gm_roctx_stop.restype = None
        lib.gm_now_ns.restype = C.c_uint64
        lib._gm_typed = True
    return lib


# ------------------------------------------------------------------------------ gm_probe
class ProbeProps(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("gcn_arch", C.c_char * 64),
                ("pci_bus_id", C.c_char * 32), ("cu_count", C.c_int32), ("warp_size", C.c_int32),
                ("total_mem", C.c_uint64), ("lds_per_block", C.c_uint64),
                ("clock_khz", C.c_int32), ("mem_clock_khz", C.c_int32)]


class MemtestRecord(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("expected", C.c_uint64), ("got", C.c_uint64),
                ("pattern", C.c_uint32), ("pass_", C.c_uint32)]


MEMTEST_MAX_RECORDS = 16      # native/include/gm_probe.h GM_MEMTEST_MAX_RECORDS


class MemtestResult(C.Structure):
    _fields_ = [("bytes_tested", C.c_uint64), ("words_in_error", C.c_uint64),
                ("bit_errors", C.c_uint64), ("stuck_mask", C.c_uint64),
                ("records_filled", C.c_uint32), ("allocations", C.c_uint32),
                ("records", MemtestRecord * MEMTEST_MAX_RECORDS),
                ("seconds", C.c_double), ("write_gbps", C.c_double),
                ("read_gbps", C.c_double), ("rw_gbps", C.c_double)]


CUSCAN_MAX_RECORDS = 16       # native/include/gm_probe.h GM_CUSCAN_MAX_RECORDS
CUSCAN_IDS = 4096             # GM_CUSCAN_IDS
CUSCAN_ANY = 0xFFFFFFFF       # GM_CUSCAN_ANY


class CuscanRecord(C.Structure):
    _fields_ = [("id", C.c_uint32), ("simd", C.c_uint32), ("test", C.c_uint32),
                ("thread", C.c_uint32), ("word", C.c_uint32), ("expected", C.c_uint32),
                ("got", C.c_uint32), ("pad", C.c_uint32)]


class CuscanInject(C.Structure):
    _fields_ = [("id", C.c_uint32), ("test", C.c_uint32), ("thread", C.c_uint32),
                ("word", C.c_uint32), ("mask", C.c_uint32)]


class CuscanCu(C.Structure):
    _fields_ = [("id", C.c_uint32), ("xcc", C.c_uint32), ("se", C.c_uint32), ("sh", C.c_uint32),
                ("cu", C.c_uint32), ("runs", C.c_uint32), ("failed_runs", C.c_uint32),
                ("tests_failed", C.c_uint32), ("simds_seen", C.c_uint32),
                ("simds_failed", C.c_uint32)]


class CuscanResult(C.Structure):
    _fields_ = [("cus_expected", C.c_uint32), ("cus_seen", C.c_uint32), ("complete", C.c_uint32),
                ("rounds", C.c_uint32), ("blocks_run", C.c_uint64),
                ("words_in_error", C.c_uint64), ("blocks_four_simds", C.c_uint64),
                ("failed_cus", C.c_uint32), ("records_filled", C.c_uint32),
                ("xcc_cus", C.c_uint32 * 16),
                ("records", CuscanRecord * CUSCAN_MAX_RECORDS),
                ("seconds", C.c_double), ("kernel_ms", C.c_double)]


class CachescanPoke(C.Structure):     # gm_cachescan_poke_t
    _fields_ = [("test", C.c_uint32), ("word_offset", C.c_uint32), ("mask", C.c_uint32)]


class CachescanTiming(C.Structure):   # gm_cachescan_timing_t: [test][min, median, max]
    _fields_ = [("first", (C.c_uint64 * 3) * 4), ("last", (C.c_uint64 * 3) * 4),
                ("blocks", C.c_uint32), ("pad", C.c_uint32)]


class LdsscanPoke(C.Structure):       # gm_ldsscan_poke_t
    _fields_ = [("test", C.c_uint32), ("word_offset", C.c_uint32), ("mask", C.c_uint32)]


BURNIN_LOG_CAP = 1024         # native/include/gm_probe.h GM_BURNIN_LOG_CAP
BURNIN_MAX_RECORDS = 16       # GM_BURNIN_MAX_RECORDS


class BurninEvent(C.Structure):       # gm_burnin_event_t
    _fields_ = [("iteration", C.c_uint32), ("tile", C.c_uint32), ("worker", C.c_uint32),
                ("reference", C.c_uint32), ("words", C.c_uint32)]


class BurninState(C.Structure):       # gm_burnin_state_t
    _fields_ = [("total", C.c_uint64), ("cursor", C.c_uint32), ("pad", C.c_uint32),
                ("log", BurninEvent * BURNIN_LOG_CAP)]


class BurninInject(C.Structure):      # gm_burnin_inject_t
    _fields_ = [("id", C.c_uint32), ("mask", C.c_uint32), ("first", C.c_uint32)]


class BurninBlamed(C.Structure):      # gm_burnin_blamed_t
    _fields_ = [("id", C.c_uint32), ("events", C.c_uint32), ("as_worker", C.c_uint32),
                ("as_reference", C.c_uint32), ("words", C.c_uint64)]


class BurninAttr(C.Structure):        # gm_burnin_attr_t
    _fields_ = [("tiles", C.c_uint32), ("grid", C.c_uint32), ("step", C.c_uint32),
                ("rotations", C.c_uint32), ("cus_seen", C.c_uint32),
                ("tiles_moved", C.c_uint32), ("tiles_exonerated", C.c_uint32),
                ("logged", C.c_uint32), ("log_overflow", C.c_uint32), ("first_id", C.c_uint32),
                ("inject_id", C.c_uint32), ("n_blamed", C.c_uint32),
                ("records_filled", C.c_uint32), ("events", C.c_uint64),
                ("records", BurninEvent * BURNIN_MAX_RECORDS)]


HOSTLINK_LEGS = 6             # native/include/gm_probe.h GM_HOSTLINK_LEGS
HOSTLINK_MAX_RECORDS = 16     # GM_HOSTLINK_MAX_RECORDS
HOSTLINK_MAX_BLOCKS = 1024    # GM_HOSTLINK_MAX_BLOCKS


class HostlinkLeg(C.Structure):
    _fields_ = [("bytes", C.c_uint64), ("ms", C.c_double), ("gbps", C.c_double),
                ("words_in_error", C.c_uint64)]


class HostlinkRecord(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("expected", C.c_uint64), ("got", C.c_uint64),
                ("leg", C.c_uint32), ("pattern", C.c_uint32), ("pass_", C.c_uint32),
                ("pad", C.c_uint32)]


class HostlinkResult(C.Structure):
    _fields_ = [("bytes", C.c_uint64), ("pinned_bytes", C.c_uint64),
                ("words_in_error", C.c_uint64), ("bit_errors", C.c_uint64),
                ("stuck_mask", C.c_uint64), ("records_filled", C.c_uint32),
                ("legs_run", C.c_uint32), ("legs", HostlinkLeg * HOSTLINK_LEGS),
                ("bidir_h2d", HostlinkLeg), ("bidir_d2h", HostlinkLeg),
                ("records", HostlinkRecord * HOSTLINK_MAX_RECORDS),
                ("seconds", C.c_double), ("host_seconds", C.c_double),
                ("transfer_seconds", C.c_double), ("setup_seconds", C.c_double),
                ("stage", C.c_char * 16)]


ATOMICS_KINDS = 13            # native/include/gm_probe.h GM_ATOMICS_NKINDS
ATOMICS_MAX_RECORDS = 16      # GM_ATOMICS_MAX_RECORDS
ATOMICS_XCC_UNKNOWN = 0xFFFFFFFF


class AtomicsKind(C.Structure):
    _fields_ = [("ops", C.c_uint64), ("words_in_error", C.c_uint64), ("ms", C.c_double),
                ("gops", C.c_double), ("width", C.c_uint32), ("pad", C.c_uint32)]


class AtomicsRecord(C.Structure):
    _fields_ = [("index", C.c_uint64), ("expected", C.c_uint64), ("got", C.c_uint64),
                ("test", C.c_uint32), ("kind", C.c_uint32), ("xcc_producer", C.c_uint32),
                ("xcc_consumer", C.c_uint32)]


class AtomicsInject(C.Structure):
    _fields_ = [("test", C.c_uint32), ("kind", C.c_uint32), ("a", C.c_uint32),
                ("b", C.c_uint32), ("word", C.c_uint32), ("mask", C.c_uint32)]


class AtomicsResult(C.Structure):
    _fields_ = [("tests_run", C.c_uint32), ("blocks", C.c_uint32), ("iters", C.c_uint32),
                ("spread", C.c_uint32), ("rounds", C.c_uint32), ("lines", C.c_uint32),
                ("budget_us", C.c_uint32), ("xccs_seen", C.c_uint32),
                ("kinds", AtomicsKind * ATOMICS_KINDS),
                ("words_in_error", C.c_uint64),
                ("tickets", C.c_uint64), ("holes", C.c_uint64), ("duplicates", C.c_uint64),
                ("counter_errors", C.c_uint64), ("order_violations", C.c_uint64),
                ("out_of_range", C.c_uint64), ("cas_giveups", C.c_uint64),
                ("handoffs", C.c_uint64), ("observed", C.c_uint64),
                ("observed_cross_xcc", C.c_uint64), ("unseen", C.c_uint64),
                ("stale_words", C.c_uint64), ("lost_words", C.c_uint64),
                ("poll_max_us", C.c_double), ("poll_mean_us", C.c_double),
                ("pairs_observed", (C.c_uint32 * 16) * 16),
                ("pairs_stale", (C.c_uint32 * 16) * 16),
                ("xcc_blocks", C.c_uint32 * 16),
                ("records_filled", C.c_uint32), ("pad", C.c_uint32),
                ("records", AtomicsRecord * ATOMICS_MAX_RECORDS),
                ("seconds", C.c_double)]


HOSTSYNC_MAX_RECORDS = 16     # native/include/gm_probe.h GM_HOSTSYNC_MAX_RECORDS
HOSTSYNC_WHERE_STALE = 1      # GM_HOSTSYNC_WHERE_STALE
HOSTSYNC_WHERE_LOST = 2       # GM_HOSTSYNC_WHERE_LOST


class HostsyncRecord(C.Structure):
    _fields_ = [("index", C.c_uint64), ("expected", C.c_uint64), ("got", C.c_uint64),
                ("test", C.c_uint32), ("kind", C.c_uint32), ("where", C.c_uint32),
                ("pad", C.c_uint32)]


class HostsyncInject(C.Structure):
    _fields_ = [("test", C.c_uint32), ("kind", C.c_uint32), ("a", C.c_uint32),
                ("b", C.c_uint32), ("word", C.c_uint32), ("mask", C.c_uint32)]


class HostsyncDir(C.Structure):
    _fields_ = [("handoffs", C.c_uint64), ("observed", C.c_uint64), ("unseen", C.c_uint64),
                ("stale_words", C.c_uint64), ("poll_max_us", C.c_double)]


class HostsyncResult(C.Structure):
    _fields_ = [("tests_run", C.c_uint32), ("tests_skipped", C.c_uint32),
                ("atomics_supported", C.c_uint32), ("blocks", C.c_uint32),
                ("host_threads", C.c_uint32), ("iters", C.c_uint32), ("spread", C.c_uint32),
                ("rounds", C.c_uint32), ("lines", C.c_uint32), ("budget_us", C.c_uint32),
                ("host_budget_us", C.c_uint32), ("cas_width", C.c_uint32),
                ("words_in_error", C.c_uint64), ("add_u32_errors", C.c_uint64),
                ("add_u64_errors", C.c_uint64), ("cas_errors", C.c_uint64),
                ("tickets", C.c_uint64), ("holes", C.c_uint64), ("duplicates", C.c_uint64),
                ("counter_errors", C.c_uint64), ("out_of_range", C.c_uint64),
                ("swaps", C.c_uint64), ("swap_missing", C.c_uint64),
                ("swap_duplicates", C.c_uint64), ("swap_foreign", C.c_uint64),
                ("cas_giveups", C.c_uint64), ("host_ops_in_flight", C.c_uint64),
                ("lost_words", C.c_uint64), ("dir", HostsyncDir * 2),
                ("rtt_median_us", C.c_double), ("rtt_max_us", C.c_double),
                ("ms", C.c_double * 5), ("records_filled", C.c_uint32), ("pad", C.c_uint32),
                ("records", HostsyncRecord * HOSTSYNC_MAX_RECORDS), ("seconds", C.c_double)]


def _prefer_torch_hip_runtime() -> None:
    """A process can hold only one HIP runtime, and ``libamdhip64.so.7`` is resolved by soname:
    whichever copy is loaded first (ROCm's /opt/rocm/lib or the one PyTorch bundles) serves
    every later user. PyTorch does not work on a newer runtime than it was built for, so when it
    is installed its bundled runtime is loaded first (by path, without importing torch) and the
    probe binds to it — the probe then works whether torch is imported before or after."""
    if "libgm_probe.so" in _libs or os.environ.get("GM_PROBE_SYSTEM_HIP") == "1":
        return
    import importlib.util

    spec = importlib.util.find_spec("torch")
    for loc in (spec.submodule_search_locations or []) if spec else []:
        hip = os.path.join(loc, "lib", "libamdhip64.so")
        if os.path.exists(hip):
            try:
                C.CDLL(hip, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def probe() -> C.CDLL:
    _prefer_torch_hip_runtime()
    lib = _load("libgm_probe.so", "hip")
    if not getattr(lib, "_gm_typed", False):
        lib.gm_probe_device_count.argtypes = [C.POINTER(C.c_int)]
        lib.gm_probe_props.argtypes = [C.c_int, C.POINTER(ProbeProps)]
        lib.gm_probe_find_device.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        lib.gm_probe_quick.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        lib.gm_probe_quick_expected.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        lib.gm_probe_quick_verdict.argtypes = [C.POINTER(C.c_uint32), C.c_uint32,
                                               C.POINTER(C.c_uint32)]
        lib.gm_probe_quick_words.argtypes = [C.c_int, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32)]
        lib.gm_probe_quick_flip.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int),
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        lib.gm_probe_mfma_peak_values.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int,
                                                  C.c_void_p, C.c_void_p]
        lib.gm_probe_hbm_copy.argtypes = [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
        lib.gm_probe_hbm_copy_variant.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int,
                                                  C.POINTER(C.c_double)]
        lib.gm_probe_hbm_read.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int,
                                          C.POINTER(C.c_double)]
        lib.gm_probe_mfma_peak.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
        lib.gm_probe_gemm_bf16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p]
        lib.gm_probe_gemm_nt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p]
        lib.gm_probe_gemm_nt_variant.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.gm_probe_gemm_nt_tflops.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(C.c_double)]
        lib.gm_probe_burn_in.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        lib.gm_probe_burn_in_flip.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint16),
                                              C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_int)]
        lib.gm_probe_count_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                            C.POINTER(C.c_uint64)]
        lib.gm_probe_fill_bf16.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
        lib.gm_probe_copy.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                      C.c_void_p]
        lib.gm_probe_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        lib.gm_probe_gemm_check.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.gm_probe_p2p.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_double)]
        lib.gm_probe_mem_info.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.gm_probe_memtest_expected.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64,
                                                  C.c_uint64, C.POINTER(C.c_uint64)]
        lib.gm_probe_memtest_fill.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                              C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]
        lib.gm_probe_memtest_verify.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                                C.c_int, C.c_uint64, C.c_uint32, C.c_uint64,
                                                C.c_void_p, C.POINTER(MemtestResult)]
        lib.gm_probe_memtest.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int,
                                         C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.POINTER(MemtestResult)]
        lib.gm_probe_memtest_store_variant.argtypes = [C.c_int]
        lib.gm_probe_cuscan_expected.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32,
                                                 C.POINTER(C.c_uint32)]
        lib.gm_probe_cuscan_signature.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        lib.gm_probe_cuscan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int,
                                        C.c_int, C.POINTER(CuscanInject),
                                        C.POINTER(CuscanResult), C.POINTER(CuscanCu), C.c_int,
                                        C.POINTER(C.c_int)]
        lib.gm_probe_mfmascan_expected.argtypes = lib.gm_probe_cuscan_expected.argtypes
        lib.gm_probe_mfmascan_images.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32,
                                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.gm_probe_mfmascan_signature.argtypes = lib.gm_probe_cuscan_signature.argtypes
        lib.gm_probe_mfmascan.argtypes = lib.gm_probe_cuscan.argtypes
        lib.gm_probe_mx_fill.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gm_probe_mxgemm_nt.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p]
        lib.gm_probe_mxgemm_expected.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                                 C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        lib.gm_probe_mxgemm_kernel_info.argtypes = [C.c_int, C.POINTER(C.c_int),
                                                    C.POINTER(C.c_int)]
        lib.gm_probe_mx_burn_in_flip.argtypes = [C.c_int] + lib.gm_probe_burn_in_flip.argtypes
        lib.gm_probe_burn_in_blame.argtypes = [C.POINTER(BurninEvent), C.c_int64,
                                               C.POINTER(C.c_uint8), C.c_int,
                                               C.POINTER(BurninAttr), C.POINTER(BurninBlamed),
                                               C.c_int]
        lib.gm_probe_burn_in_tile_map.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 3
        traced = [C.c_int, C.c_void_p, C.POINTER(BurninInject), C.c_void_p]
        lib.gm_probe_gemm_nt_traced.argtypes = lib.gm_probe_gemm_nt.argtypes[:-1] + traced
        lib.gm_probe_mxgemm_nt_traced.argtypes = lib.gm_probe_mxgemm_nt.argtypes[:-1] + traced
        lib.gm_probe_gemm_nt_traced_info.argtypes = [C.POINTER(C.c_int)] * 2
        lib.gm_probe_mxgemm_nt_traced_info.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 2
        lib.gm_probe_count_diff_tiles.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_uint32] + [C.c_void_p] * 5)
        lib.gm_probe_burn_in_state_bytes.argtypes = []
        lib.gm_probe_burn_in_state_bytes.restype = C.c_uint64
        lib.gm_probe_burn_in_attr.argtypes = (
            lib.gm_probe_burn_in_flip.argtypes[:6] + [C.POINTER(BurninInject)] +
            lib.gm_probe_burn_in_flip.argtypes[6:] +
            [C.POINTER(BurninAttr), C.POINTER(BurninBlamed), C.c_int])
        lib.gm_probe_mx_burn_in_attr.argtypes = [C.c_int] + lib.gm_probe_burn_in_attr.argtypes
        lib.gm_probe_lanescan_expected.argtypes = lib.gm_probe_cuscan_expected.argtypes
        lib.gm_probe_lanescan_lanes.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int),
                                                C.POINTER(C.c_uint32)]
        lib.gm_probe_lanescan_signature.argtypes = lib.gm_probe_cuscan_signature.argtypes
        lib.gm_probe_lanescan.argtypes = lib.gm_probe_cuscan.argtypes
        lib.gm_probe_lanescan_kernel_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.gm_probe_cachescan_expected.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32,
                                                    C.POINTER(CachescanPoke),
                                                    C.POINTER(C.c_uint32)]
        lib.gm_probe_cachescan_signature.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32,
                                                     C.POINTER(CachescanPoke), C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
        lib.gm_probe_cachescan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int,
                                           C.c_int, C.POINTER(CuscanInject),
                                           C.POINTER(CachescanPoke), C.POINTER(CuscanResult),
                                           C.POINTER(CuscanCu), C.c_int, C.POINTER(C.c_int),
                                           C.POINTER(CachescanTiming)]
        lib.gm_probe_cachescan_kernel_info.argtypes = [C.POINTER(C.c_int)] * 3
        lib.gm_probe_cachescan_geometry.argtypes = [C.POINTER(C.c_uint32)] * 4
        lib.gm_probe_ldsscan_expected.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32,
                                                  C.POINTER(LdsscanPoke), C.POINTER(C.c_uint32)]
        lib.gm_probe_ldsscan_signature.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32,
                                                   C.POINTER(LdsscanPoke), C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        lib.gm_probe_ldsscan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int,
                                         C.c_int, C.POINTER(CuscanInject), C.POINTER(LdsscanPoke),
                                         C.POINTER(CuscanResult), C.POINTER(CuscanCu), C.c_int,
                                         C.POINTER(C.c_int)]
        lib.gm_probe_ldsscan_kernel_info.argtypes = [C.POINTER(C.c_int)] * 2
        lib.gm_probe_ldsscan_geometry.argtypes = [C.POINTER(C.c_uint32)] * 4
        lib.gm_probe_sparsescan_expected.argtypes = lib.gm_probe_cuscan_expected.argtypes
        lib.gm_probe_sparsescan_signature.argtypes = lib.gm_probe_cuscan_signature.argtypes
        lib.gm_probe_sparsescan.argtypes = lib.gm_probe_cuscan.argtypes
        lib.gm_probe_sparsescan_images.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32] + \
            [C.POINTER(C.c_uint32)] * 4
        lib.gm_probe_sparsescan_apply.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gm_probe_hostlink_geometry.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.gm_probe_hostlink_unroll.argtypes = [C.c_int]
        lib.gm_probe_hostlink_kwrite.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                                 C.c_uint64, C.c_uint32, C.c_uint64, C.c_int,
                                                 C.c_uint64, C.c_uint64, C.c_void_p]
        lib.gm_probe_hostlink_kread.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int,
                                                C.c_uint64, C.c_uint32, C.c_uint64, C.c_int,
                                                C.c_void_p, C.POINTER(MemtestResult)]
        lib.gm_probe_hostlink_kcopy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                                C.c_int, C.c_uint64, C.c_uint32, C.c_uint64,
                                                C.c_int, C.c_uint64, C.c_uint64, C.c_void_p,
                                                C.POINTER(MemtestResult)]
        lib.gm_probe_hostlink.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int,
                                          C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint64,
                                          C.c_uint64, C.POINTER(HostlinkResult)]
        lib.gm_probe_atomics_expected.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_uint64, C.c_void_p, C.c_uint64]
        lib.gm_probe_atomics_widths.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_uint64)]
        lib.gm_probe_atomics_payload.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.gm_probe_atomics_payload.restype = C.c_uint32
        lib.gm_probe_atomics_add.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint64, C.POINTER(AtomicsInject),
                                             C.c_void_p]
        lib.gm_probe_atomics_cas.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint64, C.POINTER(AtomicsInject),
                                             C.c_void_p, C.POINTER(AtomicsResult)]
        lib.gm_probe_atomics_ticket.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                C.POINTER(AtomicsInject), C.c_void_p,
                                                C.POINTER(AtomicsResult)]
        lib.gm_probe_atomics_handoff.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                 C.c_uint32, C.c_uint32, C.c_uint64,
                                                 C.POINTER(AtomicsInject), C.c_void_p,
                                                 C.POINTER(AtomicsResult)]
        lib.gm_probe_atomics.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                         C.POINTER(AtomicsInject), C.POINTER(AtomicsResult)]
        u32, inj_p, res_p = C.c_uint32, C.POINTER(HostsyncInject), C.POINTER(HostsyncResult)
        lib.gm_probe_hostsync_expected.argtypes = [u32, u32, u32, u32, u32, C.c_uint64,
                                                   C.c_void_p, C.c_uint64]
        lib.gm_probe_hostsync_cas_width.argtypes = [u32, u32, u32, u32, C.POINTER(u32)]
        lib.gm_probe_hostsync_payload.argtypes = [C.c_uint64, u32, u32, u32, u32]
        lib.gm_probe_hostsync_payload.restype = u32
        lib.gm_probe_hostsync_supported.argtypes = [C.c_int, C.POINTER(C.c_int)]
        lib.gm_probe_hostsync_add.argtypes = [u32, u32, u32, u32, u32, C.c_uint64, inj_p,
                                              C.c_void_p, C.c_void_p, res_p]
        lib.gm_probe_hostsync_ticket.argtypes = [u32, u32, u32, u32, C.c_uint64, inj_p,
                                                 C.c_void_p, res_p]
        lib.gm_probe_hostsync_swap.argtypes = [u32, u32, u32, u32, C.c_uint64, inj_p,
                                               C.c_void_p, res_p]
        lib.gm_probe_hostsync_cas.argtypes = [u32, u32, u32, u32, C.c_uint64, inj_p,
                                              C.c_void_p, C.c_void_p, res_p]
        lib.gm_probe_hostsync_handoff.argtypes = [u32, u32, u32, u32, u32, u32, C.c_uint64,
                                                  inj_p, C.c_void_p, res_p]
        lib.gm_probe_hostsync.argtypes = [C.c_int, u32, u32, u32, u32, u32, u32, u32, u32, u32,
                                          C.c_uint64, inj_p, res_p]
        lib.gm_probe_strerror.argtypes = [C.c_int]
        lib.gm_probe_strerror.restype = C.c_char_p
        lib._gm_typed = True
    return lib


def loaded_libraries() -> list:
    """Paths of native libraries loaded into this process (for diagnostics/tests)."""
    return sorted(lib_path(n) for n in _libs)


def mapped_in_tree() -> list:
    """In-tree shared objects this process has mapped (``/proc/self/maps``): what the driver's
    round-end check observes. Used by ``GM_RECORD_MAPS`` in tests/conftest.py and smoke()."""
    root = os.path.dirname(LIB_DIR.rstrip("/"))
    root = os.path.dirname(root)
    seen = set()
    try:
        with open("/proc/self/maps") as fh:
            for ln in fh:
                path = ln.rstrip("\n").split(None, 5)[-1] if ln.count(" ") >= 5 else ""
                if path.startswith(root) and ".so" in os.path.basename(path):
                    seen.add(path)
    except OSError:
        pass
    return sorted(seen)


def record_maps(dest: Optional[str] = None) -> None:
    dest = dest or os.environ.get("GM_RECORD_MAPS")
    if not dest:
        return
    with open(dest, "a") as fh:
        for p in mapped_in_tree():
            fh.write(f"{os.getpid()} {p}\n")
