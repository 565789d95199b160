"""The operator-level adapter on ends-free edit alignments: WFAlignerEdit(Alignment)::alignEndsFree + getAlignmentScore() +
getAlignmentCigar() give the score and op string of the CPU restatement (tests/edit_align_endsfree_ref.cpp) after setHeuristicNone and
after setHeuristicWFadaptive; alignEnd2End on the same object keeps giving the end-to-end alignment."""
import os
import subprocess

import pytest

import span_align_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "adapter", "wfa_adapter_span_driver.cpp")


def build(tmp):
    exe = os.path.join(tmp, "wfa_adapter_span_driver")
    lib = os.path.join(ROOT, "otter_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include", "wfa_adapter"), "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, SRC, "-L" + lib, "-lotter_gpu", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_span_driver_builds(tmp_path):
    assert os.path.exists(build(str(tmp_path)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [("none",), ("wfadaptive", "10", "50", "1"), ("wfadaptive", "2", "3", "2")], ids=["none", "wfadaptive", "wfadaptive-2-3-2"])
def test_adapter_ends_free_edit_alignment_equals_the_restatement(tmp_path, mode):
    exe = build(str(tmp_path))
    cases = list(fx.input_set("FORMS")[:40]) + list(fx.input_set("EDGE")) + list(fx.input_set("TIES")[:20])
    e2e = [(p, t, (0, 0, 0, 0)) for p, t, _ in fx.input_set("FORMS")[:10]]
    text = b"".join(b"%s %s 1 %d %d %d %d\n" % ((p or b"-", t or b"-") + tuple(f)) for p, t, f in cases)
    text += b"".join(b"%s %s 0 0 0 0 0\n" % (p or b"-", t or b"-") for p, t, _ in e2e)
    r = subprocess.run([exe] + list(mode), input=text, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-500:]
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(cases) + len(e2e)
    ref_mode = ("full",) if mode[0] == "none" else ("adaptive",) + tuple(int(x) for x in mode[1:])
    want = fx.run_span_ref(cases + e2e, ref_mode)
    assert any(o for _, _, o in want)
    for i, (ln, (s, _, o)) in enumerate(zip(lines, want)):
        st, sc, c = ln.split(" ")
        assert int(st) == 0
        assert int(sc) == s, i
        assert (b"" if c == "-" else c.encode()) == o, i
