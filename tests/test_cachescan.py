"""Cache scan without a GPU: the host tables (gm_probe_cachescan_expected) against a second, naive
implementation of all four tests written here in numpy from the formulas in gm_probe.h, with the
segment and the table simulated as arrays, with and without a poke; the host table's invariants;
what a poke changes; the parsers, the refusals before any HIP call, the command lines; the
build's geometry; and the span of the icache body in the cross-compiled library."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import cachescan, cuscan
from gpumounter_amd.ops.probe import ProbeError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0x0123456789ABCDEF, 5)
ITERS = (1, 2, 63)
U = np.uint32
T = np.arange(256, dtype=np.uint32)
SEG, TABLE, STEPS = 16384, 8192, 3072


# ---------------------------------------------------------------- the reference, in numpy
def H(seed, test, idx):
    """The CU scan's hash over an array of indices (uint32 arithmetic wraps)."""
    idx = np.asarray(idx, dtype=np.uint32)
    h = U(seed & 0xFFFFFFFF) ^ (idx * U(0x9E3779B1))
    h ^= h >> U(16)
    h = h * U(0x85EBCA6B)
    h ^= h >> U(13)
    h = h + U(((seed >> 32) ^ (test * 0xC2B2AE35)) & 0xFFFFFFFF)
    h ^= h >> U(16)
    h = h * U(0xC2B2AE35)
    h ^= h >> U(13)
    h = h * U(0x27D4EB2F)
    h ^= h >> U(16)
    return h


def rotl(v, s):
    return (v << U(s)) | (v >> U(32 - s))


def fold(s, v):
    return rotl(s, 5) + v


def ref_l2(seed, iters, poke=None):
    s = np.zeros((256, 4), dtype=np.uint32)
    for r in range(iters):
        clean = H(seed, 0x400, 65536 * r + np.arange(SEG))
        seg = clean.copy()                               # the fill
        if r == 0 and poke:
            seg[poke[0]] ^= U(poke[1])
        for i in range(64):
            a = ((256 * i + T.astype(np.int64)) * 6151 + 3) % SEG
            g = seg[a]
            s[:, 0] = rotl(s[:, 0], 5) + g
            s[:, 3] += g != clean[a]
            seg[a] = ~g
        for k in range(16):
            v = 256 * k + (T.astype(np.int64) + 64) % 256
            for c in range(4):
                g = seg[4 * v + c]
                s[:, 1] = rotl(s[:, 1], 7) ^ g
                s[:, 2] += g
                s[:, 3] += g != ~clean[4 * v + c]
    return s


def ref_l1(seed, iters, poke=None):
    s = np.zeros((256, 4), dtype=np.uint32)
    clean = H(seed, 0x400, 65536 * 64 + np.arange(SEG))
    seg = clean.copy()
    if poke:
        seg[poke[0]] ^= U(poke[1])

    def probe(a):
        g1, g2 = seg[a], seg[a]           # through the L1, and past it: one array here
        s[:, 0] = fold(s[:, 0], g1)
        s[:, 1] = fold(s[:, 1], g2)
        s[:, 2] += g1 != g2
        s[:, 3] += g1 != clean[a]
    t = T.astype(np.int64)
    w, lane = t // 64, t % 64
    for _ in range(iters):
        for i in range(16):
            j = ((64 * i + lane) * 389 + 11) % 1024
            probe(1024 * (j // 256) + 256 * ((w + 1) % 4) + j % 256)
    for i in range(64):
        a = ((256 * i + t) * 4099 + 5) % SEG
        probe(a)
        probe(a)
    return s


def scalar_path(seed, iters, poke=None):
    """(signature, the table indices the four chains read)."""
    table = H(seed, 0x410, np.arange(TABLE))
    if poke:
        table[poke[0]] ^= U(poke[1])
    v = H(seed, 0x412, np.arange(1024)).reshape(256, 4)
    lane = np.arange(64, dtype=np.uint32)
    M = 0xFFFFFFFF
    visited = set()
    for w in range(4):
        i, a, b = (int(x) for x in H(seed, 0x411, 4 * w + np.arange(3)))
        i %= TABLE
        x = v[64 * w:64 * w + 64]
        for s in range(64 * iters):
            visited.add(i)
            k = int(table[i])
            a = (((a << 5) | (a >> 27)) + k) & M
            b = ((b ^ a) * 0x9E3779B1) & M
            b ^= b >> 15
            m = (((i ^ k) + s) * 0x85EBCA6B) & M
            m ^= m >> 13
            i = m % TABLE
            x[:, s & 3] = rotl(x[:, s & 3], 7) + (U(a) ^ lane * U(0x01000193))
            x[:, (s + 2) & 3] ^= U(b) + lane
    return v, visited


def ref_scalar(seed, iters, poke=None):
    return scalar_path(seed, iters, poke)[0]


def ic_consts():
    idx = 4 * np.arange(STEPS, dtype=np.uint32)[:, None] + np.arange(3, dtype=np.uint32)
    h = idx * U(0x9E3779B1) + U(0x7F4A7C15)
    h ^= h >> U(16)
    h = h * U(0x85EBCA6B)
    h ^= h >> U(13)
    h = h * U(0xC2B2AE35)
    h ^= h >> U(16)
    return h


def ref_icache_all(seeds, passes):
    """{(seed, iters): signature} for every iters in 1..passes: both seeds side by side, and the
    signature at n iters is the state after n executions of the body."""
    c = ic_consts()
    c[:, 1] |= U(1)
    x = np.concatenate([H(s, 0x420, 2 * T) for s in seeds])
    y = np.concatenate([H(s, 0x420, 2 * T + 1) for s in seeds])
    sx, sy = np.zeros_like(x), np.zeros_like(y)
    out = {}
    for it in range(1, passes + 1):
        for j in range(STEPS):
            x = rotl(x, 1 + j % 31) + c[j, 0]
            x ^= y
            x = x * c[j, 1]
            y = rotl(y, 1 + (j // 31) % 31) ^ x
            y = y + c[j, 2]
        sx, sy = fold(sx, x), fold(sy, y)
        sig = np.stack([x, y, sx, sy], axis=1)
        for n, s in enumerate(seeds):
            out[s, it] = sig[256 * n:256 * n + 256].copy()
    return out


REF = {"l2": ref_l2, "l1": ref_l1, "scalar": ref_scalar}
FAR, NEAR = (4099, 0x10), (100, 0x80000000)      # outside and inside l1's hit region


@pytest.fixture(scope="module")
def tables():
    return {(t, s, i): cachescan.expected(t, s, i)
            for t in cachescan.ALL_TESTS for s in SEEDS for i in ITERS}


@pytest.fixture(scope="module")
def icache_ref():
    return ref_icache_all(SEEDS, max(ITERS))


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("test", ("l2", "l1", "scalar"))
def test_expected_equals_the_reference(tables, test, seed, iters):
    got = tables[test, seed, iters]
    assert got.shape == (256, 4) and got.dtype == np.uint32
    np.testing.assert_array_equal(got, REF[test](seed, iters))


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
def test_expected_icache_equals_the_reference(tables, icache_ref, seed, iters):
    np.testing.assert_array_equal(tables["icache", seed, iters], icache_ref[seed, iters])


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("test,poke", (("l2", FAR), ("l2", NEAR), ("l1", FAR), ("l1", NEAR)))
def test_expected_with_a_poke_equals_the_reference(tables, test, poke, seed, iters):
    got = cachescan.expected(test, seed, iters, poke=(test, *poke))
    np.testing.assert_array_equal(got, REF[test](seed, iters, poke))
    diff = got != tables[test, seed, iters]
    t = np.arange(256)
    if test == "l2":
        # the thread that reads the word in phase 2: s0 and s3; the one that reads its element
        # in phase 3: s1, s2 and s3
        (j,) = [j for j in range(SEG) if (j * 6151 + 3) % SEG == poke[0]]
        reader2 = j % 256
        (reader3,) = t[(t + 64) % 256 == (poke[0] // 4) % 256]
        want = np.zeros((256, 4), dtype=bool)
        want[reader2, [0, 3]] = True
        want[reader3, [1, 2, 3]] = True
        np.testing.assert_array_equal(diff, want)
        assert int(got[:, 3].sum()) == 2
    else:
        # the sweep's reader, twice; inside the hit region also the hit phase's reader, per pass
        readers = {int(r) for i in range(64) for r in t[((256 * i + t) * 4099 + 5) % SEG == poke[0]]}
        hits = 0
        if poke[0] < 4096:
            w, lane = t // 64, t % 64
            for i in range(16):
                j = ((64 * i + lane) * 389 + 11) % 1024
                a = 1024 * (j // 256) + 256 * ((w + 1) % 4) + j % 256
                readers |= {int(r) for r in t[a == poke[0]]}
            hits = iters
        want = np.zeros((256, 4), dtype=bool)
        for r in readers:
            want[r, [0, 1, 3]] = True
        np.testing.assert_array_equal(diff, want)
        assert int(got[:, 3].sum()) == 2 + hits and not got[:, 2].any()
        np.testing.assert_array_equal(got[:, 0], got[:, 1])      # both paths see the poked word


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
def test_expected_scalar_with_a_poke(tables, seed, iters):
    clean, visited = scalar_path(seed, iters)
    on = min(visited)
    got = cachescan.expected("scalar", seed, iters, poke=("scalar", on, 1))
    np.testing.assert_array_equal(got, ref_scalar(seed, iters, (on, 1)))
    assert (got != clean).any()
    off = next(i for i in range(TABLE) if i not in visited)      # a word no chain reads
    np.testing.assert_array_equal(
        cachescan.expected("scalar", seed, iters, poke=("scalar", off, 1)), clean)


def test_a_poke_leaves_the_other_tests_tables_alone(tables):
    seed, iters = SEEDS[0], 2
    for poked in ("l2", "l1", "scalar"):
        for other in cachescan.ALL_TESTS:
            if other != poked:
                np.testing.assert_array_equal(
                    cachescan.expected(other, seed, iters, poke=(poked, 100, 0x10)),
                    tables[other, seed, iters])


def test_tables_differ_between_tests_seeds_and_iters(tables):
    keys = list(tables)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert (tables[a] != tables[b]).mean() > 0.4, (a, b)


def test_host_table_invariants(tables):
    for (test, _, _), tab in tables.items():
        if test == "l2":
            assert not tab[:, 3].any()
        if test == "l1":
            np.testing.assert_array_equal(tab[:, 0], tab[:, 1])
            assert not tab[:, 2].any() and not tab[:, 3].any()


def test_the_permutations_visit_every_word_once():
    j = np.arange(SEG, dtype=np.int64)
    assert sorted((j * 6151 + 3) % SEG) == list(range(SEG))              # l2, phase 2
    assert sorted((j * 4099 + 5) % SEG) == list(range(SEG))              # l1, the sweep
    t = T.astype(np.int64)
    vecs = np.concatenate([256 * k + (t + 64) % 256 for k in range(16)])   # l2, phase 3
    assert sorted(vecs) == list(range(4096))
    for w in range(4):                      # a wave's hit addresses: the next wave's 1024 words
        lane = np.arange(64)
        a = np.concatenate([1024 * (jj // 256) + 256 * ((w + 1) % 4) + jj % 256
                            for jj in (((64 * i + lane) * 389 + 11) % 1024 for i in range(16))])
        assert len(set(a.tolist())) == 1024 and a.max() < 4096
        assert set(((a // 256) % 4).tolist()) == {(w + 1) % 4}


def test_geometry_agrees_with_the_header():
    text = open(os.path.join(ROOT, "native", "include", "gm_cachescan_ref.h")).read()

    def const(name):
        return int(re.search(rf"#define {name} (\d+)", text).group(1))
    geo = cachescan.geometry()
    assert geo == {"seg_bytes": const("GM_CACHESCAN_SEG_BYTES"),
                   "l1_hit_bytes": const("GM_CACHESCAN_L1_HIT_BYTES"),
                   "table_bytes": const("GM_CACHESCAN_TABLE_BYTES"),
                   "icache_steps": const("GM_CACHESCAN_ICACHE_STEPS")}
    assert geo == {"seg_bytes": 65536, "l1_hit_bytes": 16384, "table_bytes": 32768,
                   "icache_steps": STEPS}
    assert cachescan.SEG_WORDS * 4 == geo["seg_bytes"]
    assert cachescan.TABLE_WORDS * 4 == geo["table_bytes"]
    assert cachescan.DEFAULT_ITERS == const("GM_CACHESCAN_DEFAULT_ITERS")
    assert cachescan.MAX_ITERS == const("GM_CACHESCAN_MAX_ITERS") == 63


def test_the_icache_body_spans_twice_the_instruction_cache(tmp_path):
    """The body is a function of its own; the size of its symbol in the gfx950 code object of the
    cross-compiled library is its span. (On a GPU, kernel_info() reads the same span from the
    program counter.)"""
    lib = open(os.path.join(ROOT, "gpumounter_amd", "_lib", "libgm_probe.so"), "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    sizes = []
    for m in re.finditer(magic, lib):
        base = m.start()
        (n,) = struct.unpack_from("<Q", lib, base + len(magic))
        pos = base + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", lib, pos)
            triple = lib[pos + 24:pos + 24 + tlen]
            pos += 24 + tlen
            if b"gfx950" not in triple or lib[base + off:base + off + 4] != b"\x7fELF":
                continue
            obj = tmp_path / f"bundle_{base}.co"
            obj.write_bytes(lib[base + off:base + off + size])
            out = subprocess.run([readelf, "-sW", str(obj)], capture_output=True, text=True,
                                 check=True).stdout
            sizes += [int(line.split()[2]) for line in out.splitlines()
                      if "FUNC" in line and line.rstrip().endswith("ic_bodyEjj")]
    print("icache body symbol sizes:", sizes)
    assert len(sizes) == 1 and sizes[0] >= cachescan.ICACHE_MIN_BODY_BYTES == 131072, sizes


# ---------------------------------------------------------------- parsers and refusals
def test_parsers():
    assert cachescan.ALL_TESTS == ("l2", "l1", "scalar", "icache")
    assert cachescan.TESTS == {"l2": 1, "l1": 2, "scalar": 4, "icache": 8}
    assert cachescan.parse_tests("l2, icache") == ("l2", "icache")
    assert cachescan.parse_inject("any:l2:0:0:1") == ("any", "l2", 0, 0, 1)
    assert cachescan.parse_inject("0x123:icache:130:2:0x10000") == (0x123, "icache", 130, 2, 0x10000)
    assert cachescan.parse_poke("l1:4099:0x10") == ("l1", 4099, 0x10)
    assert cachescan.parse_poke("scalar:8191:1") == ("scalar", 8191, 1)
    for bad in ("nope", "l2,nope", ""):
        with pytest.raises(ProbeError):
            cachescan.parse_tests(bad)
    for bad in ("any:l2:0:0", "any:nope:0:0:1", "any:l2:256:0:1", "any:l2:0:4:1", "any:l2:0:0:0",
                "4096:l2:0:0:1", "any:l2:x:0:1", "any:l2:0:0:0x100000000"):
        with pytest.raises(ProbeError):
            cachescan.parse_inject(bad)
    for bad in ("l1:4099", "nope:0:1", "icache:0:1", "l1:16384:1", "l2:-1:1", "scalar:8192:1",
                "l1:0:0", "l1:x:1", "l1:0:0x100000000"):
        with pytest.raises(ProbeError):
            cachescan.parse_poke(bad)


def test_scan_validates_before_any_hip_call(monkeypatch):
    """Every refusal below is made in Python with the native library unreachable."""
    def unreachable():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_native, "probe", unreachable)
    for kw in (dict(tests=()), dict(tests=("l2", "nope")), dict(tests=16), dict(iters=0),
               dict(iters=cachescan.MAX_ITERS + 1), dict(iters=1.5), dict(iters=True),
               dict(seed=-1), dict(seed=1 << 64), dict(min_rounds=0),
               dict(min_rounds=3, max_rounds=2), dict(max_rounds=1025),
               dict(_inject=("any", "l1", 0, 0, 0)), dict(_inject=("any", "l1", 256, 0, 1)),
               dict(_inject=("any", "l1", 0, 4, 1)), dict(_inject=(4096, "l1", 0, 0, 1)),
               dict(_inject=("any", "l1", 0, 0)), dict(tests=("l2",), _inject=("any", "l1", 0, 0, 1)),
               dict(_poke=("icache", 0, 1)), dict(_poke=("l1", 16384, 1)),
               dict(_poke=("scalar", 8192, 1)), dict(_poke=("l1", 0, 0)), dict(_poke=("l1", 0)),
               dict(tests=("l2",), _poke=("l1", 0, 1)), dict(_poke=("nope", 0, 1))):
        with pytest.raises(ProbeError):
            cachescan.scan(0, **kw)
    with pytest.raises(ProbeError):
        cachescan.scan(-1)
    for call in (lambda: cachescan.expected("nope", 0, 1), lambda: cachescan.expected("l1", 0, 0),
                 lambda: cachescan.expected("l1", 0, 64),
                 lambda: cachescan.expected("l1", 0, 1, poke=("icache", 0, 1)),
                 lambda: cachescan.signature("l1", 0, 0), lambda: cachescan.signature(3, 0, 1),
                 lambda: cachescan.signature("l1", 0, 64),
                 lambda: cachescan.signature("l1", 0, 1, poke=("l2", 0, 1)),
                 lambda: cachescan.signature("l1", 0, 1, poke=("l1", 16384, 1))):
        with pytest.raises(ProbeError):
            call()
    with pytest.raises(AssertionError):                  # a good call does get there
        cachescan.scan(0)


def test_native_entry_points_validate_before_selecting_a_device():
    """hipErrorInvalidValue (1) on a host without a GPU proves no HIP call came first."""
    lib = _native.probe()
    res, n = _native.CuscanResult(), C.c_int(7)
    cus = (_native.CuscanCu * 4)()
    timing = _native.CachescanTiming()
    out = (C.c_uint32 * 1024)()
    P, W = C.c_void_p(4096), C.c_void_p(8192)   # never dereferenced: every call is refused first
    poke = _native.CachescanPoke
    for test, iters in ((0, 1), (3, 1), (16, 1), (1, 0), (1, 64)):
        assert lib.gm_probe_cachescan_expected(test, 0, iters, None, out) == 1
        assert lib.gm_probe_cachescan_signature(test, 0, iters, None, P, W, None) == 1
    assert lib.gm_probe_cachescan_expected(1, 0, 1, None, None) == 1
    assert lib.gm_probe_cachescan_expected(8, 0, 1, None, out) == 0
    for o, w in ((None, W), (P, None), (C.c_void_p(4096 + 4), W), (P, C.c_void_p(8194))):
        assert lib.gm_probe_cachescan_signature(1, 0, 1, None, o, w, None) == 1
    bad_pokes = (poke(8, 0, 1), poke(2, 16384, 1), poke(4, 8192, 1), poke(2, 0, 0), poke(3, 0, 1),
                 poke(16, 0, 1), poke(0, 0, 1))
    for pk in bad_pokes:
        assert lib.gm_probe_cachescan_expected(2, 0, 1, C.byref(pk), out) == 1
        assert lib.gm_probe_cachescan_signature(2, 0, 1, C.byref(pk), P, W, None) == 1
    assert lib.gm_probe_cachescan_signature(2, 0, 1, C.byref(poke(1, 0, 1)), P, W, None) == 1
    assert lib.gm_probe_cachescan_kernel_info(None, None, None) == 1
    assert lib.gm_probe_cachescan_geometry(None, None, None, None) == 1

    def scan(mask=15, iters=1, lo=1, hi=1, inj=None, pk=None, cap=4, table=cus):
        return lib.gm_probe_cachescan(0, mask, iters, 0, lo, hi,
                                      C.byref(inj) if inj is not None else None,
                                      C.byref(pk) if pk is not None else None, C.byref(res),
                                      table, cap, C.byref(n), C.byref(timing))
    assert scan(mask=0) == 1 and n.value == 0
    assert scan(mask=16) == 1
    assert scan(iters=0) == 1 and scan(iters=64) == 1
    assert scan(lo=0) == 1 and scan(lo=2, hi=1) == 1 and scan(hi=1025) == 1
    assert scan(cap=-1) == 1 and scan(cap=4, table=None) == 1
    inject = _native.CuscanInject
    for inj in (inject(0, 8, 0, 0, 0), inject(0, 6, 0, 0, 1), inject(0, 8, 256, 0, 1),
                inject(0, 8, 0, 4, 1), inject(4096, 8, 0, 0, 1), inject(0, 16, 0, 0, 1)):
        assert scan(inj=inj) == 1
    assert scan(mask=1, inj=inject(0, 8, 0, 0, 1)) == 1          # a test that is not selected
    for pk in bad_pokes:
        assert scan(pk=pk) == 1
    assert scan(mask=1, pk=poke(2, 0, 1)) == 1                   # a test that is not selected
    assert lib.gm_probe_cachescan(0, 15, 1, 0, 1, 1, None, None, None, cus, 4, C.byref(n),
                                  None) == 1


# ---------------------------------------------------------------- command lines
def test_command_lines_parse_the_cache_scan_options():
    from gpumounter_amd.cli import build_parser, cmd_doctor, cmd_probe

    ap = build_parser()
    a = ap.parse_args(["probe"])
    assert a.cache_scan is False and a.cache_scan_inject is None and a.cache_scan_poke is None
    assert a.cache_scan_tests is None and a.cache_scan_iters is None and a.cache_scan_rounds is None
    a = ap.parse_args(["probe", "--cache-scan", "--cache-scan-tests", "l2,l1",
                       "--cache-scan-iters", "3", "--cache-scan-rounds", "2", "--cache-scan-inject",
                       "any:l2:0:0:1", "--cache-scan-poke", "l1:4099:0x10"])
    assert a.cache_scan and tuple(a.cache_scan_tests) == ("l2", "l1")
    assert a.cache_scan_iters == 3 and a.cache_scan_rounds == 2
    assert a.cache_scan_inject == ("any", "l2", 0, 0, 1) and a.cache_scan_poke == ("l1", 4099, 16)
    for bad in (["--cache-scan-tests", "l2,nope"], ["--cache-scan-inject", "any:l2:0:0"],
                ["--cache-scan-inject", "any:l2:0:0:0"], ["--cache-scan-iters", "x"],
                ["--cache-scan-poke", "icache:0:1"], ["--cache-scan-poke", "l1:16384:1"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["probe", "--cache-scan", *bad])
    # usage errors (2), not a failed scan (1), before any GPU work
    for opt in (["--cache-scan-inject", "any:l2:0:0:1"], ["--cache-scan-poke", "l1:0:1"],
                ["--cache-scan-iters", "3"], ["--cache-scan-tests", "l2"],
                ["--cache-scan-rounds", "2"]):
        assert cmd_probe(ap.parse_args(["probe", *opt])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--cache-scan", "--cache-scan-tests", "scalar",
                                    "--cache-scan-inject", "any:l2:0:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--cache-scan", "--cache-scan-tests", "scalar",
                                    "--cache-scan-poke", "l1:0:1"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--cache-scan", "--cache-scan-iters", "64"])) == 2
    assert cmd_probe(ap.parse_args(["probe", "--cache-scan", "--cache-scan-rounds", "0"])) == 2
    d = ap.parse_args(["doctor", "--gpu", "--cache-scan", "--cache-scan-inject", "any:l1:1:2:4",
                       "--cache-scan-poke", "l2:7:8"])
    assert d.cache_scan is True and d.cache_scan_inject == ("any", "l1", 1, 2, 4)
    assert d.cache_scan_poke == ("l2", 7, 8)
    assert ap.parse_args(["doctor", "--gpu"]).cache_scan is False
    assert cmd_doctor(ap.parse_args(["doctor", "--cache-scan-poke", "l2:7:8"])) == 2
    assert cmd_doctor(ap.parse_args(["doctor", "--cache-scan-inject", "any:l1:1:2:4"])) == 2


def test_probe_passes_the_options_on(monkeypatch, capsys):
    from gpumounter_amd.cli import build_parser, cmd_probe
    from gpumounter_amd.ops import probe

    class Res:
        def to_dict(self):
            return {"device": 0}
    calls = []

    def fake_scan(dev, **kw):
        calls.append((dev, kw))
        return {"ok": kw["_inject"] is None and kw["_poke"] is None}
    monkeypatch.setattr(probe, "verify", lambda bdfs, full=False: [Res()])
    monkeypatch.setattr(cachescan, "scan", fake_scan)
    ap = build_parser()
    assert cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--cache-scan"])) == 0
    assert calls[-1] == (0, dict(tests=cachescan.ALL_TESTS, iters=cachescan.DEFAULT_ITERS,
                                 min_rounds=1, max_rounds=16, _inject=None, _poke=None))
    assert cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--cache-scan",
                                    "--cache-scan-tests", "l1", "--cache-scan-iters", "63",
                                    "--cache-scan-rounds", "20", "--cache-scan-inject",
                                    "any:l1:0:0:1"])) == 1
    assert calls[-1] == (0, dict(tests=("l1",), iters=63, min_rounds=20, max_rounds=20,
                                 _inject=("any", "l1", 0, 0, 1), _poke=None))
    assert cmd_probe(ap.parse_args(["probe", "--bdf", "0000:05:00.0", "--cache-scan",
                                    "--cache-scan-poke", "l1:4099:0x10"])) == 1
    assert calls[-1][1]["_poke"] == ("l1", 4099, 16) and calls[-1][1]["_inject"] is None
    assert '"cachescan"' in capsys.readouterr().out


def test_validate_parses_the_cache_scan_options():
    from gpumounter_amd.parallel import validate

    with pytest.raises(SystemExit):
        validate.main(["--cache-scan-inject", "any:l2:0:0:1"])           # needs --cache-scan
    with pytest.raises(SystemExit):
        validate.main(["--cache-scan-poke", "l1:0:1"])
    with pytest.raises(SystemExit):
        validate.main(["--cache-scan", "--cache-scan-inject", "any:nope:0:0:1"])
    with pytest.raises(SystemExit):
        validate.main(["--cache-scan", "--cache-scan-poke", "icache:0:1"])


def test_doctor_passes_the_scan_on_and_names_the_unit_and_test(monkeypatch):
    from gpumounter_amd.ops import probe
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    sig = inspect.signature(doctor.check_gpus).parameters
    assert sig["cache_scan"].default is False
    assert sig["cache_scan"].kind is sig["cache_scan"].KEYWORD_ONLY
    assert sig["cache_scan_inject"].default is None and sig["cache_scan_poke"].default is None
    assert inspect.signature(doctor.run).parameters["cache_scan"].default is False

    calls = []

    def fake_scan(dev, _inject=None, _poke=None):
        calls.append((dev, _inject, _poke))
        bad = _inject is not None or _poke is not None
        failed = [{"id": 0x123, "xcc": 1, "se": 1, "sh": 0, "cu": 3, "runs": 1, "failed_runs": 1,
                   "tests_failed": ["l1"], "simds_failed": [2]}] if bad else []
        return {"tests": list(cachescan.ALL_TESTS), "cus_seen": 250, "cus_expected": 256,
                "complete": False, "rounds": 16, "kernel_ms": 1.0, "words_in_error": int(bad),
                "ok": not bad, "failed": failed, "timing": {}}
    monkeypatch.setattr(probe, "device_count", lambda: 1)
    monkeypatch.setattr(probe, "props", lambda d: {"pci_bus_id": "0000:05:00.0",
                                                   "gcn_arch": "gfx950:sramecc+:xnack-"})
    monkeypatch.setattr(probe, "quick", lambda d: 10.0)
    monkeypatch.setattr(cachescan, "scan", fake_scan)
    cfg = Config.load(env={}, amdsmi_lib="mock")
    (plain,) = [c for c in doctor.check_gpus(cfg) if c.name == "gpu0"]
    assert "cache-scan" not in plain.detail and calls == []
    (ok,) = [c for c in doctor.check_gpus(cfg, cache_scan=True) if c.name == "gpu0"]
    assert ok.status == "ok" and "cache-scan 4 tests 250/256 CUs" in ok.detail   # stated, not failed
    assert "incomplete" in ok.detail and " 0 wrong words" in ok.detail
    inj, pk = (0x123, "l1", 130, 2, 0x10000), ("l1", 4099, 0x10)
    (bad,) = [c for c in doctor.check_gpus(cfg, cache_scan=True, cache_scan_inject=inj)
              if c.name == "gpu0"]
    assert bad.status == "fail" and bad.detail.endswith("xcc 1 se 1 sh 0 cu 3 (id 0x123) simd 2 l1")
    (bad,) = [c for c in doctor.check_gpus(cfg, cache_scan=True, cache_scan_poke=pk)
              if c.name == "gpu0"]
    assert bad.status == "fail" and bad.detail.endswith("simd 2 l1")
    assert calls == [(0, None, None), (0, inj, None), (0, None, pk)]


def test_the_result_decoder_is_shared_with_the_cu_scan():
    unit = {"id": 0x225, "xcc": 2, "se": 1, "sh": 0, "cu": 5, "simds_failed": [1, 3],
            "tests_failed": ["l2", "icache"]}
    assert cachescan.describe_failed({"failed": [unit]}) == (
        "xcc 2 se 1 sh 0 cu 5 (id 0x225) simd 1,3 l2+icache")
    assert cuscan.describe_failed({"failed": [unit]}) == cachescan.describe_failed({"failed": [unit]})
    t = _native.CachescanTiming()
    t.blocks = 3
    t.first[1][0], t.first[1][1], t.first[1][2] = 5, 6, 7
    t.last[1][1] = 9
    assert cachescan.decode_timing(2, t) == {
        "blocks": 3, "l1": {"first": {"min": 5, "median": 6, "max": 7},
                            "last": {"min": 0, "median": 9, "max": 0}}}
    assert C.sizeof(_native.CachescanTiming) == 2 * 4 * 3 * 8 + 8
