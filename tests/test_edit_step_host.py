"""The column step of the bit-parallel edit tiers (otter_amd/csrc/myers_step.hpp) on the host: tests/edit_step_host.cpp, built with
-fsanitize=address,undefined as a stand-alone program, drives block_step() column by column over edge-case and random pairs (m up to 300)
and compares every value of the last column with a textbook DP.  On the host the function evaluates the boolean expressions from which the
device's v_bitop3_b32 truth tables are derived at compile time; the program prints the derived bytes."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "edit_step_host.cpp")


def test_block_step_against_dp(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "edit_step_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "otter_amd", "csrc"), "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    tables = dict(re.findall(r"^table (\S+) (0x[0-9a-f]{2})$", r.stdout, re.M))
    # the bytes a reader can check by hand: bit (4a + 2b + c) = f(a, b, c)
    assert tables == {"(a^b)|c": "0xbe", "a|~(b|c)": "0xf1"}
    m = re.search(r"^pairs (\d+) columns (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 100000
