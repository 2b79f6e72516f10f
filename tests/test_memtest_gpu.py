"""HBM pattern test on the MI355X (``pytest -m gpu``): the gfx950 kernels of
native/hip/gm_memtest.hip against the host evaluation of the same pattern function, the error
path against injected bit flips, the allocating driver, and the command line. Nothing here
holds more than 1 GiB of device memory, and nothing uses the default "most of free memory" size.

Geometry the shapes below rely on (gm_memtest.hip): 16-byte elements, 256-thread blocks, an
unrolled step of 8 × 256 elements = 32 KiB per block, each block's chunk a whole number of
steps, at most CUs × 2 blocks. A 1 MiB + 4112 byte buffer therefore runs as 32 blocks of one
full step plus one block that has only the 16-byte tail loop (257 elements)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpumounter_amd import _native
from gpumounter_amd.ops import memtest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
STEP = 32 * 1024                     # bytes per block per unrolled step
BIG = (1 << 20) + 4112               # 32 full chunks + a tail-only block, not a chunk multiple
SIZES = (16, 4096 - 16, STEP + 16, BIG)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a host without a GPU")


def _buf(nbytes: int):
    return torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")


def _host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _want(pattern, invert, pass_, base, nbytes) -> np.ndarray:
    e = memtest.expected(pattern, SEED, pass_, base, nbytes // 8)
    return ~e if invert else e


def _signed(v: int) -> int:
    return v - (1 << 64) if v >= 1 << 63 else v


def _flip(t, flips) -> None:
    """XOR mask into the word at byte offset off, for (off, mask) in flips, with torch."""
    idx = torch.tensor([off // 8 for off, _ in flips], device=t.device)
    masks = torch.tensor([_signed(m) for _, m in flips], dtype=torch.int64, device=t.device)
    t[idx] = t[idx] ^ masks


def _fill_matches_the_host_reference(pattern, invert):
    for nbytes in SIZES:
        t = _buf(nbytes + 32)
        t.fill_(0x1111111111111111)
        body = t[2:-2]                                   # 16-byte aligned, guard words around
        memtest.fill(body, pattern, invert=invert, seed=SEED, pass_=3)
        got = _host(t)
        np.testing.assert_array_equal(got[2:-2], _want(pattern, invert, 3, 0, nbytes),
                                      err_msg=f"{pattern} invert={invert} {nbytes} B")
        assert (got[:2] == 0x1111111111111111).all() and (got[-2:] == 0x1111111111111111).all()


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", memtest.ALL_PATTERNS)
def test_fill_matches_the_host_reference(pattern, invert):
    _fill_matches_the_host_reference(pattern, invert)


@pytest.mark.parametrize("pattern", memtest.ALL_PATTERNS)
def test_fill_uses_64_bit_offsets(pattern):
    """A 128 KiB buffer placed at 2^35 - 64 KiB of the region crosses the 2^32-word and the
    2^35-byte boundary: 32-bit index arithmetic anywhere would write something else."""
    base, nbytes = 2**35 - 65536, 128 * 1024
    t = _buf(nbytes)
    for invert in (False, True):
        memtest.fill(t, pattern, invert=invert, seed=SEED, pass_=1, base_offset=base)
        np.testing.assert_array_equal(_host(t), _want(pattern, invert, 1, base, nbytes))
    assert memtest.verify(t, pattern, invert=True, seed=SEED, pass_=1,
                          base_offset=base)["errors"] == 0


# byte offset, XOR mask: first two words, last word, both sides of a block-chunk boundary, a word
# of the 16-byte tail loop, and one in the middle of an unrolled step
FLIPS = [(0, 0x1), (8, 0x8000000000000000), (BIG - 8, 0x0000000100000001),
         (STEP - 8, 0x00F0000000000000), (STEP, 0x2), (5 * STEP, 0xFFFFFFFFFFFFFFFF),
         ((1 << 20) + 16 * 5 + 8, 0x0000040000000400), (3 * STEP + 4096 + 16, 0x80)]


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", ["addr", "walk", "random"])
def test_verify_reports_exactly_the_injected_flips(pattern, invert):
    base = 1 << 33
    t = _buf(BIG)
    memtest.fill(t, pattern, invert=invert, seed=SEED, pass_=2, base_offset=base)
    clean = memtest.verify(t, pattern, invert=invert, seed=SEED, pass_=2, base_offset=base)
    assert clean["errors"] == 0 and clean["bit_errors"] == 0 and clean["first_errors"] == []
    assert clean["ok"] and int(clean["stuck_mask"], 16) == 0 and clean["bytes"] == BIG
    _flip(t, FLIPS)
    r = memtest.verify(t, pattern, invert=invert, seed=SEED, pass_=2, base_offset=base)
    want = _want(pattern, invert, 2, base, BIG)
    assert r["errors"] == len(FLIPS) and not r["ok"], r
    assert r["bit_errors"] == sum(bin(m).count("1") for _, m in FLIPS)
    stuck = 0
    for _, m in FLIPS:
        stuck |= m
    assert int(r["stuck_mask"], 16) == stuck
    got = sorted((x["offset"], int(x["expected"], 16), int(x["got"], 16), int(x["xor"], 16))
                 for x in r["first_errors"])
    exp = sorted((base + off, int(want[off // 8]), int(want[off // 8]) ^ m, m)
                 for off, m in FLIPS)
    assert got == exp
    assert all(x["pattern"] == pattern and x["pass"] == 2 for x in r["first_errors"])
    json.dumps(r)                                        # everything survives JSON


def test_verify_keeps_16_records_of_40_errors():
    t = _buf(BIG)
    memtest.fill(t, "random", seed=SEED)
    offs = [8 * ((k * 3301 + 17) % (BIG // 8)) for k in range(40)]
    assert len(set(offs)) == 40
    _flip(t, [(o, 1 << (k % 64)) for k, o in enumerate(offs)])
    r = memtest.verify(t, "random", seed=SEED)
    assert r["errors"] == 40 and r["bit_errors"] == 40, r
    recs = [x["offset"] for x in r["first_errors"]]
    assert len(recs) == 16 and len(set(recs)) == 16 and set(recs) <= set(offs)
    for x in r["first_errors"]:
        assert int(x["xor"], 16) == 1 << (offs.index(x["offset"]) % 64)


def _verify_and_invert_leaves_the_inverse_everywhere(pattern):
    t = _buf(BIG)
    memtest.fill(t, pattern, seed=SEED, pass_=1)
    _flip(t, FLIPS)
    r = memtest.verify(t, pattern, write_inverse=True, seed=SEED, pass_=1)
    assert r["errors"] == len(FLIPS)
    assert r["bit_errors"] == sum(bin(m).count("1") for _, m in FLIPS)
    np.testing.assert_array_equal(_host(t), _want(pattern, True, 1, 0, BIG))
    again = memtest.verify(t, pattern, invert=True, seed=SEED, pass_=1)
    assert again["errors"] == 0 and again["first_errors"] == []
    # and back: checking ~P while writing P
    r = memtest.verify(t, pattern, invert=True, write_inverse=True, seed=SEED, pass_=1)
    assert r["errors"] == 0
    np.testing.assert_array_equal(_host(t), _want(pattern, False, 1, 0, BIG))


@pytest.mark.parametrize("pattern", ["addr", "solid", "random"])
def test_verify_and_invert_leaves_the_inverse_everywhere(pattern):
    _verify_and_invert_leaves_the_inverse_everywhere(pattern)


@pytest.mark.parametrize("pattern", memtest.ALL_PATTERNS)
def test_plain_store_kernels_fill_and_invert_like_the_nontemporal_ones(pattern):
    """The writing kernels exist twice, with nontemporal (the default) and with plain stores
    (bench/memtest_rates.py times both): the same shapes, flips and expectations for the
    plain-store ones."""
    lib = _native.probe()
    was = lib.gm_probe_memtest_store_variant(0)
    try:
        assert lib.gm_probe_memtest_store_variant(-1) == 0
        for invert in (False, True):
            _fill_matches_the_host_reference(pattern, invert)
        _verify_and_invert_leaves_the_inverse_everywhere(pattern)
    finally:
        lib.gm_probe_memtest_store_variant(was)
    assert lib.gm_probe_memtest_store_variant(-1) == was


def test_uint8_and_uint64_tensors_are_accepted():
    for dtype, n in ((torch.uint8, 4096), (torch.uint64, 512)):
        t = torch.empty(n, dtype=dtype, device="cuda")
        memtest.fill(t, "checker")
        assert memtest.verify(t, "checker")["errors"] == 0
        assert (t.view(torch.uint8).cpu().numpy() == 0x55).all()
    with pytest.raises(memtest.ProbeError):                       # misaligned view
        memtest.fill(torch.empty(4096 + 8, dtype=torch.uint8, device="cuda")[8:], "addr")


def test_driver_spans_several_allocations():
    n = 3 * 2**20 + 4112
    r = memtest.memtest(0, nbytes=n, chunk_bytes=2**20, passes=2)
    print(r)
    assert r["errors"] == 0 and r["ok"] and r["first_errors"] == [], r
    assert r["bytes"] == n and r["allocations"] == 4 and r["passes"] == 2
    assert r["patterns"] == list(memtest.ALL_PATTERNS)
    assert r["hbm_exercised"] is False
    json.dumps(r)


def test_driver_finds_a_flip_in_the_second_allocation():
    n, off, mask = 3 * 2**20 + 4112, 2**20 + 8, 0x0000000100000001
    r = memtest.memtest(0, nbytes=n, chunk_bytes=2**20, passes=2, _flip=(off, mask))
    assert r["errors"] == len(memtest.ALL_PATTERNS) * 2 and not r["ok"], r
    assert r["bit_errors"] == 2 * r["errors"] and int(r["stuck_mask"], 16) == mask
    assert len(r["first_errors"]) == r["errors"]
    assert all(x["offset"] == off and int(x["xor"], 16) == mask for x in r["first_errors"])
    assert {(x["pattern"], x["pass"]) for x in r["first_errors"]} == {
        (p, k) for p in memtest.ALL_PATTERNS for k in range(2)}


def test_mem_info_and_default_plan():
    mi = memtest.mem_info(0)
    assert 0 < mi["free"] <= mi["total"] and mi["total"] > 200 * (1 << 30)
    assert memtest.plan_bytes(mi["free"], mi["total"]) <= mi["free"]


def _cli(*args, env=None):
    return subprocess.run([sys.executable, "-m", "gpumounter_amd", *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=180,
                          env={**os.environ, **(env or {})})


def test_probe_cli_memtest():
    res = _cli("probe", "--memtest", "64M")
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout)
    assert out and all(r["memtest"]["ok"] and r["memtest"]["bytes"] == 64 << 20 for r in out), out


def test_probe_cli_memtest_flip_fails():
    res = _cli("probe", "--memtest", "64M", "--memtest-flip", "4096:0x10",
               "--memtest-patterns", "addr,random")
    assert res.returncode == 1, (res.stdout[-2000:], res.stderr[-2000:])
    out = json.loads(res.stdout)
    assert all(r["memtest"]["errors"] == 2 and not r["memtest"]["ok"] for r in out), out
    assert all(x["offset"] == 4096 and int(x["xor"], 16) == 0x10
               for r in out for x in r["memtest"]["first_errors"])


def test_doctor_memtest():
    res = _cli("doctor", "--json", "--skip-cluster", "--gpu", "--memtest", "64M",
               env={"GM_SYSTEMD_DEVICE_ALLOW": "off"})
    checks = [c for c in json.loads(res.stdout)
              if c["name"].startswith("gpu") and c["name"] != "gpu"]
    assert checks, res.stdout[-2000:]
    for c in checks:
        assert c["status"] == "ok" and "memtest 0.06 GiB" in c["detail"], c
        assert " 0 bad words" in c["detail"], c


def test_doctor_memtest_reports_a_flip_as_failed():
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    cfg = Config.load(env={}, amdsmi_lib="mock")
    checks = [c for c in doctor.check_gpus(cfg, memtest_bytes=64 << 20, memtest_flip=(4096, 0x10))
              if c.name != "gpu"]
    assert checks and all(c.status == "fail" and " 5 bad words" in c.detail for c in checks), checks


def test_memtest_rates():
    """The project's own "2 TB/s = sick GPU" floor (test_probe_hbm_and_mfma_rates): a copy at
    that floor reads 1000 and writes 1000 GB/s. Nothing tighter is asserted here; the measured
    table is in BASELINE.md."""
    r = memtest.memtest(0, nbytes=1 << 30, patterns=("addr",))
    print(f"memtest 1 GiB addr: read {r['read_gbps']:.0f} GB/s, write {r['write_gbps']:.0f} GB/s, "
          f"read+write {r['rw_gbps']:.0f} GB/s")
    assert r["ok"] and r["hbm_exercised"] is True, r
    assert r["read_gbps"] > 2000 and r["write_gbps"] > 1000, r
