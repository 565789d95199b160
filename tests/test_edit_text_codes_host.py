"""The text row codes of the bit-parallel edit tiers (otter_amd/csrc/myers_masks.hpp) on the host: tests/edit_text_codes_host.cpp, built
with -fsanitize=address,undefined as a stand-alone program, checks text_row_code on all byte values, the eight-at-a-time text_row_codes8
against it, and the reversed copy, codes and table blocks of byte strings of lengths 1-200, bytes outside A C G T included."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "edit_text_codes_host.cpp")


def test_text_codes_against_definition(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "edit_text_codes_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"^words (\d+) strings (\d+) flagged (\d+) fails 0$", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    words, strings, flagged = map(int, m.groups())
    assert words == 8 * 256 * 8 and strings == 200 * 12 and 400 < flagged < strings
