"""CPU: the score loop of the gap-affine register tiers waits for no vector memory and reads no private memory — from the ISA.

`wfa_affine_reg.hip` is compiled once to assembly with the library's flags.  For the four default shapes and <8,8> the score loop is the
innermost loop that holds the S2 provenance `global_store_short` (scripts/isa_reg_loop.py finds it from the control flow).  In it:
  * no `s_waitcnt` names `vmcnt`: the provenance stores are never read back, so the only reason for such a wait is state that fell into
    private memory (two flags of the queue did: two dependent reloads per score, each behind every store of the sweep);
  * no instruction whose mnemonic begins with `scratch_`;
and in the metadata `.vgpr_count` stays within each shape's granule and `.private_segment_fixed_size` is at least 8 bytes (the two flags) below
what it was with the flags: 52 / 56 / 44 / 44 / 44 then.  Spill counts are printed, not asserted."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (NW, S2): (.vgpr_count bound of the granule, .private_segment_fixed_size with the two flags in private memory)
SHAPES = {(1, 8): (128, 52), (1, 12): (168, 56), (2, 8): (128, 44), (4, 8): (128, 44), (8, 8): (128, 44)}
DEFAULT_LB = 2      # <1,12> also exists as an alternative shape with LB = 0 (vector registers spilled on purpose): not the default


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
    return {(k[0], k[1]): v for k, v in out.items() if (k[0], k[1]) in SHAPES and k[5] == DEFAULT_LB}


@pytest.mark.parametrize("shape", sorted(SHAPES), ids=["%d-%d" % s for s in sorted(SHAPES)])
def test_score_loop_has_no_memory_wait(report, shape):
    r = report[shape]
    m, lp = r["meta"], r["loop"]
    assert lp is not None, "score loop not found"
    print("<%d,%d>: vgpr %d (spilled %d), sgpr spilled %d, private segment %d bytes; score loop %d instructions, %d v_readlane, %d v_writelane" % (
        shape + (m["vgpr_count"], m["vgpr_spill_count"], m["sgpr_spill_count"], m["private_segment_fixed_size"], lp["instructions"], lp["v_readlane"], lp["v_writelane"])))
    assert lp["prov_stores"] >= shape[1], lp["prov_stores"]
    assert lp["vmcnt_waits"] == [], lp["vmcnt_waits"]
    assert lp["scratch"] == [], lp["scratch"]
    vgpr, private_then = SHAPES[shape]
    assert m["vgpr_count"] <= vgpr, m
    assert m["private_segment_fixed_size"] <= private_then - 8, m
