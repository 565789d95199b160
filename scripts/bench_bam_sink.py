"""Wall time of otg_assemble_files on the 10 000-locus fixture of scripts/bench_e2e.py with the collecting writer (SAM text into memory) and
with the BAM sink (otg_bam_sink_write as the writer: BAM + BAI on disk) deflating on 1 and on 16 host threads.  Per leg one untimed
warm-up, then three rounds taken in turn; prints median (min - max) per leg and the size of what was written.
usage: python scripts/bench_bam_sink.py [regions=10000] [reads=30] [ingest threads=16]"""
import os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import otter_amd
from otter_amd import bamwrite

R = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
D = int(sys.argv[2]) if len(sys.argv) > 2 else 30
T = int(sys.argv[3]) if len(sys.argv) > 3 else 16
tmp = tempfile.mkdtemp()
t0 = time.perf_counter()
fx = bamwrite.make_tr_fixture(tmp, R, depth=D, len_range=(1000, 5000), seed=7)
print("fixture: %d regions, %d records, BAM %.1f MB (%.1f s to build)" % (R, fx["n_records"], os.path.getsize(fx["bam"]) / 1e6, time.perf_counter() - t0), flush=True)
out = os.path.join(tmp, "alleles.bam")


def run(sink_threads):
    """one job; sink_threads None = the collecting writer"""
    t = time.perf_counter()
    text, st = otter_amd.assemble_files(fx["bam"], fx["bed"], read_group="s1", offset_l=1, offset_r=1, mapq=10, threads=T,
                                        bam_out=out if sink_threads is not None else None, bam_threads=sink_threads)
    return time.perf_counter() - t, len(text), st


legs = [("collecting writer", None), ("sink, 1 thread", 1), ("sink, 16 threads", 16)]
walls = {name: [] for name, _ in legs}
for name, k in legs:
    run(k)
for rnd in range(3):
    for name, k in legs:
        w, n, st = run(k)
        walls[name].append(w)
        print("round %d %-18s %.3f s; %s; stage busy ms: ingest %.0f, hot path %.0f, emit %.0f" % (
            rnd, name, w, "%.1f MB of SAM text" % (n / 1e6) if k is None else "%.1f MB BAM + %.0f KB BAI" % (os.path.getsize(out) / 1e6, os.path.getsize(out + ".bai") / 1e3),
            st["ms_ingest"], st["ms_hot_path"], st["ms_emit"]), flush=True)
for name, _ in legs:
    w = sorted(walls[name])
    print("%-18s median %.0f ms (%.0f - %.0f)" % (name, 1e3 * w[1], 1e3 * w[0], 1e3 * w[2]))
