"""Builds libotter_gpu.so (hand-written HIP for gfx950) in-tree with hipcc.  No CPU fallback is built."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libotter_gpu.so")
SOURCES = ["otg_api.hip", "wfa_edit.hip", "edit_align.hip", "myers_edit.hip", "wfa_affine.hip", "wfa_affine_reg.hip", "wfa_adaptive.hip", "cluster.hip", "poa.hip", "pipeline.hip", "emit.hip", "compare.hip", "kmer_usage.hip", "vcf2mat.hip", "ingest.hip", "bedfa.hip", "dispatch.hip", "gather.hip", "cohort.hip", "genotype_edit.hip", "motif.hip", "motif_emit.hip", "repeat.hip", "repeat_emit.hip", "unitalign.hip", "unitalign_emit.hip", "unitparse.hip", "unitparse_emit.hip", "tract.hip", "tract_emit.hip", "locus.hip", "locus_emit.hip", "unitset.hip", "unitset_emit.hip", "spread.hip", "spread_emit.hip"]
# host-only sources (no device code; each also builds alone, without the rest of the library): the BAM + BAI writer and merge
HOST_SOURCES = ["bam_sink.cpp"]
# -ffp-contract=off: the reference's clustering decisions are FP64 comparisons made without FMA
# contraction; fused operations are written explicitly where glibc uses them.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result"]


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: cannot build libotter_gpu.so (there is no CPU fallback)")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "otter_gpu.h")]
    return any(os.path.getmtime(d) > t for d in deps if os.path.isfile(d))


TOOL_SRC = os.path.join(HERE, "..", "tools", "otter_assemble.cpp")
TOOL = os.path.join(HERE, "..", "tools", "otter_assemble")
TOOLS = [(TOOL_SRC, TOOL), (os.path.join(HERE, "..", "tools", "otter_compare.cpp"), os.path.join(HERE, "..", "tools", "otter_compare")),
         (os.path.join(HERE, "..", "tools", "otter_vcf2mat.cpp"), os.path.join(HERE, "..", "tools", "otter_vcf2mat")),
         (os.path.join(HERE, "..", "tools", "otter_cohort.cpp"), os.path.join(HERE, "..", "tools", "otter_cohort")),
         (os.path.join(HERE, "..", "tools", "otter_merge.cpp"), os.path.join(HERE, "..", "tools", "otter_merge")),
         (os.path.join(HERE, "..", "tools", "otter_motifs.cpp"), os.path.join(HERE, "..", "tools", "otter_motifs")),
         (os.path.join(HERE, "..", "tools", "otter_repeats.cpp"), os.path.join(HERE, "..", "tools", "otter_repeats")),
         (os.path.join(HERE, "..", "tools", "otter_copies.cpp"), os.path.join(HERE, "..", "tools", "otter_copies")),
         (os.path.join(HERE, "..", "tools", "otter_unitparse.cpp"), os.path.join(HERE, "..", "tools", "otter_unitparse")),
         (os.path.join(HERE, "..", "tools", "otter_tracts.cpp"), os.path.join(HERE, "..", "tools", "otter_tracts")),
         (os.path.join(HERE, "..", "tools", "otter_loci.cpp"), os.path.join(HERE, "..", "tools", "otter_loci")),
         (os.path.join(HERE, "..", "tools", "otter_units.cpp"), os.path.join(HERE, "..", "tools", "otter_units")),
         (os.path.join(HERE, "..", "tools", "otter_spread.cpp"), os.path.join(HERE, "..", "tools", "otter_spread"))]


def build_tool(force=False):
    """the command-line hosts of the dispatcher (plain C++ over the C-ABI); each rebuilt when its source or the library is newer"""
    for src, exe in TOOLS:
        if not os.path.exists(src) or not os.path.exists(LIB):
            continue
        if not force and os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(src), os.path.getmtime(LIB), os.path.getmtime(os.path.join(HERE, "..", "include", "otter_gpu.h"))):
            continue
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src, "-L" + HERE, "-lotter_gpu", "-Wl,-rpath," + HERE, "-Wl,-rpath,/opt/rocm/lib"])


def build(force=False, verbose=False, jobs=4):
    if not force and not needs_build():
        build_tool()
        return LIB
    cc = hipcc()
    objs = []
    procs = []
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    for src in SOURCES + HOST_SOURCES:
        path = os.path.join(CSRC, src)
        obj = os.path.join(CSRC, "build", os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))] + [os.path.join(HERE, "..", "include", "otter_gpu.h")]
        if (not force) and os.path.exists(obj) and os.path.getmtime(obj) > max([os.path.getmtime(path)] + [os.path.getmtime(h) for h in headers]):
            continue
        cmd = [cc] + (FLAGS if src in SOURCES else FLAGS[1:]) + os.environ.get("OTG_EXTRA_HIPCC_FLAGS", "").split() + ["-c", path, "-o", obj]      # (measurement builds: -DOTG_REG_TIMING, ...)
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        if len(procs) >= jobs:
            _drain(procs)
    _drain(procs)
    cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-lz", "-pthread", "-ldl"]      # zlib: BGZF blocks of the BAM ingest; threads: its region slices
    subprocess.check_call(cmd)
    build_tool(force=True)
    return LIB


def _drain(procs):
    while procs:
        src, p = procs.pop(0)
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, out.decode(errors="replace")))
        if out.strip():
            sys.stderr.write(out.decode(errors="replace"))


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
