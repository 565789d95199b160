"""otg_bam_sink / otg_bam_merge under AddressSanitizer and UBSan: tools/fuzz_bam_sink.cpp has its own main and is compiled together with
otter_amd/csrc/bam_sink.cpp alone (that source needs nothing else of the library), so nothing is loaded into Python.  It feeds sinks seeded
mutations of a clean allele text and merges BAMs whose records were mutated INSIDE still-valid BGZF blocks (the technique of
tests/test_host_sanitizers.py).  Every call must come back with OTG_OK or an error code and no sanitizer report, leaks on the refusal paths included
(LeakSanitizer needs ptrace; where a container forbids that it says so itself, and only then the run is repeated without the leak check).
CPU only; skipped when the compiler is absent."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import test_bam_sink as T
from test_host_sanitizers import _bgzf_blocks, _bgzf_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if not os.path.exists(CLANGXX):
        pytest.skip("clang++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("san_sink")), "fuzz_bam_sink")
    p = subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tools", "fuzz_bam_sink.cpp"), os.path.join(ROOT, "otter_amd", "csrc", "bam_sink.cpp"), "-o", exe, "-lz", "-pthread"],
                       capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return exe


def test_sanitized_sink_and_merge(fuzz_bin, tmp_path):
    rng = np.random.default_rng(17)
    text = T.sorted_text(T.allele_text(seed=14, n=120))
    sam = str(tmp_path / "clean.sam")
    open(sam, "wb").write(text)
    clean = str(tmp_path / "clean_in.bam")
    T.sink_bam(text, clean)
    raw = open(clean, "rb").read()
    blocks = _bgzf_blocks(raw)
    assert len(blocks) >= 3
    bams = [clean]
    for trial in range(12):
        mut = [bytearray(b) for b in blocks]
        for _ in range(int(rng.integers(1, 12))):
            bi = int(rng.integers(0 if trial % 6 == 5 else 1, len(mut) - 1))      # mostly past the header block; never the EOF block
            pos = int(rng.integers(0, len(mut[bi])))
            kind = trial % 4
            if kind == 0:
                mut[bi][pos] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:
                mut[bi][pos] = int(rng.integers(0, 256))
            elif kind == 2:                                                       # a plausible but wrong 32-bit field
                mut[bi][pos:pos + 4] = struct.pack("<I", int(rng.choice([0, 1, 0x7fffffff, 0xffffffff, 0x80000000, 65536, 1 << 29])))[:max(0, min(4, len(mut[bi]) - pos))]
            else:
                del mut[bi][pos:pos + int(rng.integers(1, 40))]
        p = str(tmp_path / ("m%d.bam" % trial))
        _bgzf_write(p, [bytes(b) for b in mut])
        bams.append(p)
    for trial in range(3):                                                        # truncations of the compressed file
        p = str(tmp_path / ("t%d.bam" % trial))
        open(p, "wb").write(raw[:int(rng.integers(30, len(raw)))])
        bams.append(p)
    for leaks in (1, 0):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=%d:abort_on_error=0:allocator_may_return_null=1" % leaks, UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([fuzz_bin, sam, str(tmp_path)] + bams, capture_output=True, timeout=600, env=env)
        err = r.stderr.decode(errors="replace")
        if "LeakSanitizer has encountered a fatal error" not in err and "LeakSanitizer does not work" not in err:
            break                                                                 # the leak check ran (or nothing went wrong without it)
    assert "Sanitizer" not in err and "runtime error" not in err and r.returncode == 0, (r.returncode, err[-3000:])
    out = r.stdout.decode()
    assert out.startswith("done:"), out
    refused, total = int(out.split()[1]), int(out.split()[3])
    assert total == 60 and 10 < refused < 60, out                                 # the mutations do reach the refusals, and not every text is refused
    m_ref, m_tot = int(out.split(";")[1].split()[0]), int(out.split(";")[1].split()[2])
    assert m_tot == 2 * 15 and 0 < m_ref < m_tot, out
