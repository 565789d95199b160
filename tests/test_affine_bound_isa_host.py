"""CPU: the gap-affine bound pass keeps its state in registers and its packed score loop waits for no vector memory — from the ISA.

`wfa_affine.hip` is compiled once to assembly with the library's flags; scripts/isa_bound_pass.py finds the score loops of every
wfa_affine_bound1_kernel instantiation from LLVM's loop annotations.  For each instantiation:
  * no private memory at all (`.private_segment_fixed_size` 0, no spilled register): the kernel's rows live in registers;
  * the packed score loop (the one that probes LDS) advances four scores per trip with the first probe inline, and neither it nor its rolled
    probe loop holds an `s_waitcnt` that names `vmcnt` or a `scratch_` access;
  * the LDS of a block is what the template's SEQW words per wave come to, and the blocks per CU the launcher asks for (SHAPES below, restated
    from otg_launch_affine_todo) fit the CU's 160 KB; the shape of reads up to 8 kb keeps eight waves per SIMD.
The instruction counts per score are printed, not asserted."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (SEQW words per wave, waves per block): blocks per CU the launcher sizes its grid for
SHAPES = {(1030, 4): 8, (1542, 4): 6, (2054, 4): 4, (4102, 2): 4}
LDS_PER_CU = 160 * 1024


def _tool():
    spec = importlib.util.spec_from_file_location("isa_bound_pass", os.path.join(ROOT, "scripts", "isa_bound_pass.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def report():
    from otter_amd import build as B
    try:
        B.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    tool = _tool()
    rep = tool.report(ROOT)
    tool.show("bound pass", rep)
    return {(k[2], k[3]): v for k, v in rep.items()}


def test_every_launched_shape_is_built(report):
    assert sorted(report) == sorted(SHAPES), sorted(report)


@pytest.mark.parametrize("shape", sorted(SHAPES), ids=["%d-%d" % s for s in sorted(SHAPES)])
def test_bound_pass_registers_lds_and_waits(report, shape):
    r = report[shape]
    m = r["meta"]
    seqw, wpb = shape
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert r["waves_per_block"] == wpb and m["group_segment_fixed_size"] == 4 * seqw * wpb, m
    assert SHAPES[shape] * m["group_segment_fixed_size"] <= LDS_PER_CU, (SHAPES[shape], m["group_segment_fixed_size"])
    assert m["vgpr_count"] <= 64, m                                      # eight waves per SIMD as far as registers go
    if seqw == 1030:
        assert SHAPES[shape] * wpb == 32 and r["waves_per_simd"] == 8, r["waves_per_simd"]
    packed = [lp for lp in r["loops"] if lp["probe_inline"]]
    assert len(packed) == 1, [lp["probes"] for lp in r["loops"]]
    lp = packed[0]
    print("<%d,%d>: %d VGPR, %d SGPR, LDS %d; packed loop per score %s, each further probe %s" % (
        shape + (m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"], lp["per_score"], lp["further_probe"])))
    assert lp["scores_per_trip"] == 4 and lp["leader_reductions"] == 2, lp
    assert lp["probes"] == ["lds"] and len(lp["inner_loops"]) == 4, lp
    assert lp["vmcnt_waits"] == 0 and lp["scratch"] == 0, lp
    assert all(q["vmcnt_waits"] == 0 and q["scratch"] == 0 and q["trip"]["vmem"] == 0 for q in lp["inner_loops"]), lp["inner_loops"]
    assert lp["body"]["vmem"] == 0, lp["body"]
