"""The score ranges of the gap-affine register tiers in closed form (otter_amd/csrc/affine_score_range.hpp) on the host:
tests/affine_score_range_host.cpp, built with -fsanitize=address,undefined as a stand-alone program, runs the helper beside a transcription
of the range bookkeeping the kernel carried from score to score at commit 80c7124 (five-deep history, clamps, diamond clip), on every score
up to and including the failing one, exhaustively over pl, tl in 1..12, lo0 in -4..0, hi0 in 0..4, end ranges from end-free lengths 0..4
and U in 0..40, and checks that score 1 is the only empty one."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "affine_score_range_host.cpp")


def test_closed_form_against_recurrence(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "affine_score_range_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"^sets (\d+) scores (\d+) empty (\d+) ended (\d+) fails 0$", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    sets, scores, empty, ended = map(int, m.groups())
    assert sets == 12 * 12 * 5 * 5 * 5 * 5 * 41
    # every parameter set runs into its failing score, and has exactly one empty score on the way (score 1) unless it fails at score 0 or 1
    assert ended == sets and scores > 2 * sets and empty <= sets
