"""The attributed burn-in on the MI355X (``pytest -m gpu``): a rotated tile map changes no bit of
the three GEMMs, the CU map the blocks store is valid, a clean run blames nobody, a flipped
reference blames the CU that computed that reference tile, a consistently wrong CU (the
injection) is the only unit blamed, through the Python entry, the command line and doctor, and the
traced kernels use no scratch. Nothing here asserts a rate or a placement.

Shapes: n = 768 is 9 tiles, a grid that is no multiple of 8 (XCDs get 2, 1, 1, ... blocks);
n = 2048 is 64 tiles, 8 per XCD and a full group of 8 tile rows. K = n, so 12 and 32 K-tiles of
bf16, 6 / 3 and 16 / 8 of mxfp8 / mxfp4: odd and even counts through the two LDS stages."""
import functools
import json
import os
import re
import subprocess
import sys

import pytest

from gpumounter_amd.ops import cuframe, mxgemm, probe

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_A, SEED_B = 0x5151, 0xA3A3
FORMATS = mxgemm.BURN_IN_FORMATS
SHAPES = (768, 2048)
BURN_S = 0.3


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu test on a host without a GPU")


@functools.lru_cache(maxsize=None)
def operands(fmt, n):
    """The burn-in's operands at n × n × n, filled once per case and never written to."""
    if fmt == "bf16":
        a = probe.fill_bf16(torch.empty((n, n), dtype=torch.bfloat16, device="cuda"), SEED_A)
        bt = probe.fill_bf16(torch.empty((n, n), dtype=torch.bfloat16, device="cuda"), SEED_B)
        return a, bt
    return mxgemm.fill(fmt, "random", SEED_A, n, n) + mxgemm.fill(fmt, "random", SEED_B, n, n)


def plain(fmt, n):
    ops = operands(fmt, n)
    return probe.gemm_nt(*ops) if fmt == "bf16" else mxgemm.gemm_nt(fmt, *ops)


def traced(fmt, n, r, _inject=None):
    ops = operands(fmt, n)
    if fmt == "bf16":
        return probe.gemm_nt_traced(*ops, r=r, _inject=_inject)
    return mxgemm.gemm_nt_traced(fmt, *ops, r=r, _inject=_inject)


def burn_in(fmt, n, **kw):
    if fmt == "bf16":
        return probe.burn_in(0, BURN_S, n, **kw)
    return mxgemm.burn_in(0, BURN_S, fmt, n=n, **kw)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_rotation_changes_no_bit(fmt, n):
    """A wrong map leaves tiles unwritten or written twice; a rotation that leaks into the operand
    addressing computes another tile's values: either differs from the untraced result."""
    grid = (n // 256) ** 2
    want = plain(fmt, n)
    c0, cus0 = traced(fmt, n, 0)
    assert probe.count_diff(c0, want) == 0
    for r in (1, 7, grid - 1):
        c, cus = traced(fmt, n, r)
        assert probe.count_diff(c, c0) == 0, (fmt, n, r)
        ids = cus.cpu().tolist()
        assert all(0 <= i < 4096 and cuframe.decode_id(i)["xcc"] < 8 for i in ids), ids
        moved = sum(a != b for a, b in zip(ids, cus0.cpu().tolist()))
        print(f"{fmt} n={n} r={r}: cus_seen={len(set(ids))} tiles_moved={moved}/{grid}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_cu_map_is_valid_and_the_injection_flips_one_element_per_tile_of_that_cu(fmt):
    n, grid = 2048, 64
    c0, cus = traced(fmt, n, 0)
    ids = cus.cpu().tolist()
    assert len(ids) == grid and all(0 <= i < 4096 for i in ids), ids
    assert all(cuframe.decode_id(i)["xcc"] < 8 for i in ids)
    print(f"{fmt}: cus_seen={len(set(ids))} of {grid} tiles")
    # the control, on one GEMM: the tiles of the injected CU, and only those, differ, in element
    # (0, 0) alone. Where the blocks run is the run's own, so the flipped tiles are read from its map.
    target = ids[0]
    c, cus = traced(fmt, n, 0, _inject=(target, 0x1))
    hit = [t for t, i in enumerate(cus.cpu().tolist()) if i == target]
    diff = (c.view(torch.int16) != c0.view(torch.int16)).nonzero().cpu().tolist()
    assert sorted(diff) == sorted([t // 8 * 256, t % 8 * 256] for t in hit), (diff, hit)
    for row, col in diff:
        assert int(c.view(torch.int16)[row, col]) ^ int(c0.view(torch.int16)[row, col]) == 1


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_clean_run_blames_nobody(fmt, n):
    r = burn_in(fmt, n, attribute=True)
    a = r["attribution"]
    print(f"{fmt} n={n}: iterations={r['iterations']} tflops={r['tflops']:.0f} "
          f"cus_seen={a['cus_seen']} tiles_moved={a['tiles_moved']}/{a['tiles']} "
          f"exonerated={a['tiles_exonerated']}")
    assert r["ok"] is True and r["mismatches"] == 0 and r["iterations"] >= 1, r
    assert a["events"] == 0 and a["logged"] == 0 and a["blamed"] == [] and not a["log_overflow"]
    grid = (n // 256) ** 2
    assert a["tiles"] == a["grid"] == grid and a["step"] == probe.burn_in_tile_map(n)[1]
    assert a["rotations"] == min(r["iterations"], grid) and a["cus_seen"] >= 1
    assert a["tiles_exonerated"] == a["tiles_moved"]     # every move reproduced the reference
    assert "inject_id" not in a and "flipped_words" not in r
    json.dumps(r)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_flipped_reference_blames_the_cu_that_computed_it(fmt, n):
    row, col = 300, 700                       # tile (1, 2) at both shapes
    tile = (row // 256) * (n // 256) + col // 256
    r = burn_in(fmt, n, _flips=[(row * n + col, 0x8000)], attribute=True)
    a = r["attribution"]
    assert r["ok"] is False and r["mismatches"] == r["iterations"] >= 1, r
    assert r["flipped_words"] == 1 and a["events"] == r["iterations"], r
    assert a["tiles_exonerated"] < a["tiles"], a          # that tile never matches
    first = a["first_events"][0]
    assert first["tile"] == tile and first["words"] == 1 and first["iteration"] >= 1, first
    (b,) = a["blamed"]
    assert b["id"] == first["reference"], (b, first)      # the reference map's id for that tile
    assert b["as_reference"] > 0 and b["events"] == a["logged"] and b["words"] == a["logged"]
    assert all(e["tile"] == tile and e["reference"] == b["id"] for e in a["first_events"])


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_consistently_wrong_cu_is_the_only_unit_blamed(fmt):
    """Needs the CU called ``first`` to compute a tile again after the warm-up, which HIP does
    not promise: should it not, the events are 0 and this fails, as a finding about placement,
    not about the GPU (profiles/burnin_attr/README.md: on the box this was written on it came
    back every second iteration: 2164 events in 4328 bf16 iterations)."""
    r = burn_in(fmt, 2048, _inject=("first", 0x1), attribute=True)
    a = r["attribution"]
    print(f"{fmt}: iterations={r['iterations']} events={a['events']} logged={a['logged']} "
          f"inject_id={a['inject_id']:#05x} blamed={a['blamed']}")
    assert a["inject_id"] == a["first_id"] < 4096
    assert r["ok"] is False and r["mismatches"] == a["events"] > 0, r
    assert a["blamed"] and a["blamed"][0]["id"] == a["inject_id"], a
    assert [b["id"] for b in a["blamed"]] == [a["inject_id"]], a["blamed"]


def test_probe_cli_names_the_injected_unit_and_exits_1():
    res = subprocess.run([sys.executable, "-m", "gpumounter_amd", "probe", "--burn-in", "0.3",
                          "--burn-in-format", "bf16,mxfp4", "--burn-in-attribute",
                          "--burn-in-inject", "first:0x1"], cwd=ROOT, capture_output=True,
                         text=True, timeout=180)
    assert res.returncode == 1, (res.stdout[-2000:], res.stderr[-2000:])
    out = json.loads(res.stdout)
    assert out
    for r in out:
        for key in ("burn_in", "burn_in_mxfp4"):
            b, a = r[key], r[key]["attribution"]
            print(f"{key}: iterations={b['iterations']} tflops={b['tflops']:.0f} "
                  f"events={a['events']} cus_seen={a['cus_seen']} "
                  f"tiles_moved={a['tiles_moved']}/{a['tiles']}")
            assert b["ok"] is False and b["mismatches"] > 0 and a["tiles"] == 1024, b
            assert [u["id"] for u in a["blamed"]] == [a["inject_id"]], a["blamed"]
        assert "burn_in_mxfp8" not in r


def test_doctor_names_the_blamed_unit_and_the_format():
    from gpumounter_amd.utils import doctor
    from gpumounter_amd.utils.config import Config

    cfg = Config.load(env={}, amdsmi_lib="mock")
    checks = doctor.check_gpus(cfg, BURN_S, burn_in_formats=("mxfp8",), burn_in_attribute=True,
                               burn_in_inject=("first", 0x1))
    (c,) = [c for c in checks if c.name == "gpu0"]
    print(c.detail)
    assert c.status == "fail" and "failed: mxfp8 burn-in" in c.detail
    blames = c.detail.split("mxfp8 burn-in blames: ")[1]
    assert re.match(r"xcc \d+ se \d+ sh \d+ cu \d+ \(id 0x[0-9a-f]{3}\) ", blames), blames
    assert " as worker" in blames or " as reference" in blames
    assert "; " not in blames.split(" (log overflowed")[0]        # one unit


@pytest.mark.parametrize("fmt", FORMATS)
def test_traced_kernels_use_no_scratch(fmt):
    info = probe.traced_kernel_info(fmt)
    print(f"{fmt}: traced kernel {info['num_regs']} registers")
    assert info["scratch_bytes"] == 0, info
