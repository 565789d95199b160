"""CPU: what the closed-form score ranges and the score 0 in front of the loop buy the gap-affine register tiers, from the ISA.

`wfa_affine_reg.hip` is compiled once to assembly with the library's flags and read by scripts/isa_reg_loop.py, as
tests/test_affine_reg_parity_isa_host.py does.  With no range history, no score-0 code and no path for an unreachable score in either loop
body, for the four default shapes and <8,8>:
  * no vector register is spilled and the private segment is empty;
  * `.vgpr_count` is at most 96 for the S2 = 8 shapes and at most 128 for <1,12>: the register granules of five and of four waves per SIMD
    on a file of 512 registers per lane;
  * the score loop holds no more `v_mov_b32` and no more instructions than it did with the history (PARENT), no `s_waitcnt` in it names
    `vmcnt`, nothing in it touches private memory (`scratch_`), and it holds 2 S2 provenance `global_store_short`.
PARENT: the loop's figures at commit 80c7124, taken with the same script."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (NW, S2): (v_mov_b32 in the score loop, instructions in the score loop) at 80c7124
PARENT = {(1, 8): (307, 7396), (1, 12): (430, 10474), (2, 8): (282, 7475), (4, 8): (286, 7489), (8, 8): (337, 7494)}
VGPR_MAX = {(1, 8): 96, (1, 12): 128, (2, 8): 96, (4, 8): 96, (8, 8): 96}
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
def test_no_spill_and_a_leaner_loop(report, shape):
    r = report[shape]
    m, lp = r["meta"], r["loop"]
    assert lp is not None, "score loop not found"
    v_mov, instructions = PARENT[shape]
    print("<%d,%d>: vgpr %d (spilled %d), private segment %d bytes, score loop %d instructions (with the history %d), %d v_mov (%d), %d provenance stores, %d v_readlane" % (
        shape + (m["vgpr_count"], m["vgpr_spill_count"], m["private_segment_fixed_size"], lp["instructions"], instructions, lp["v_mov"], v_mov, lp["prov_stores"], lp["v_readlane"])))
    assert m["vgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= VGPR_MAX[shape], m
    assert lp["v_mov"] <= v_mov, (lp["v_mov"], v_mov)
    assert lp["instructions"] <= instructions, (lp["instructions"], instructions)
    assert lp["vmcnt_waits"] == [], lp["vmcnt_waits"]
    assert lp["scratch"] == [], lp["scratch"]
    assert lp["prov_stores"] == 2 * shape[1], lp["prov_stores"]
