"""CPU: the two-body score loop of the gap-affine register tiers, from the ISA — no swaps, and none come back as copies.

`wfa_affine_reg.hip` is compiled once to assembly with the library's flags and read by scripts/isa_reg_loop.py, as
tests/test_affine_reg_isa_host.py does.  The score loop runs two scores per trip, each in a body compiled for its parity, so for the four
default shapes and <8,8>:
  * the loop holds no `v_swap_b32` (the one-body loop had 2 S2 per score: the two parity sets of M rows traded places);
  * it holds 2 S2 provenance `global_store_short`, S2 per body;
  * no `s_waitcnt` in it names `vmcnt` and nothing in it touches private memory (`scratch_`);
  * `.vgpr_count` and the vector registers spilled are not above the one-body loop's (PARENT below);
  * it holds at most twice the `v_mov_b32` the one-body loop held per score: the swaps have not come back as copies.
PARENT: the figures of the one-body loop, taken with the same script from commit 0626e08 (the last one with that loop)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (NW, S2): (.vgpr_count, vector registers spilled, v_mov_b32 in the score loop = per score) at 0626e08
PARENT = {(1, 8): (128, 10, 215), (1, 12): (168, 11, 315), (2, 8): (128, 8, 209), (4, 8): (128, 8, 211), (8, 8): (128, 8, 213)}
DEFAULT_LB = 2      # <1,12> also exists as an alternative shape with LB = 0: not the default
DEFAULT_WPEU = {(1, 12): 3}


def _tool():
    spec = importlib.util.spec_from_file_location("isa_reg_loop", os.path.join(ROOT, "scripts", "isa_reg_loop.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    from otter_amd import build as B
    try:
        B.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    tool = _tool()
    asm = str(tmp_path_factory.mktemp("isa") / "wfa_affine_reg.s")
    tool.compile_reg(asm)
    out = tool.analyse(open(asm).read(), with_visit=False)
    shutil.rmtree(os.path.dirname(asm), ignore_errors=True)
    return {(k[0], k[1]): v for k, v in out.items() if (k[0], k[1]) in PARENT and k[5] == DEFAULT_LB and k[3] == DEFAULT_WPEU.get((k[0], k[1]), 4)}


@pytest.mark.parametrize("shape", sorted(PARENT), ids=["%d-%d" % s for s in sorted(PARENT)])
def test_two_body_score_loop(report, shape):
    r = report[shape]
    m, lp = r["meta"], r["loop"]
    assert lp is not None, "score loop not found"
    vgpr, spilled, v_mov = PARENT[shape]
    print("<%d,%d>: vgpr %d (spilled %d; one body %d, %d), score loop %d instructions, %d provenance stores, %d v_swap, %d v_mov (one body %d per score), %d v_readlane" % (
        shape + (m["vgpr_count"], m["vgpr_spill_count"], vgpr, spilled, lp["instructions"], lp["prov_stores"], lp["v_swap"], lp["v_mov"], v_mov, lp["v_readlane"])))
    assert lp["v_swap"] == 0, lp["v_swap"]
    assert lp["prov_stores"] == 2 * shape[1], lp["prov_stores"]
    assert lp["vmcnt_waits"] == [], lp["vmcnt_waits"]
    assert lp["scratch"] == [], lp["scratch"]
    assert m["vgpr_count"] <= vgpr, m
    assert m["vgpr_spill_count"] <= spilled, m
    assert lp["v_mov"] <= 2 * v_mov, (lp["v_mov"], v_mov)
