"""The match-mask builder of the bit-parallel edit tiers (otter_amd/csrc/myers_masks.hpp) on the host: tests/edit_masks_host.cpp, built
with -fsanitize=address,undefined as a stand-alone program, runs the block builder (with a ballot that loops over the 64 rows) and the
plane-to-row derivation against the per-base definition of the five mask rows on random byte strings of lengths 0-200, bytes outside
A C G T included."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "edit_masks_host.cpp")


def test_block_masks_against_per_base(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "edit_masks_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"^strings (\d+) blocks (\d+) flagged (\d+) one_extra (\d+) unsupported (\d+)$", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    strings, blocks, flagged, one_extra, unsupported = map(int, m.groups())
    # every kind of string was met: plain, flagged with one extra symbol (built and derived), and unsupported
    assert strings > 4000 and blocks > 8000 and one_extra > 1000 and unsupported > 500 and flagged >= one_extra
