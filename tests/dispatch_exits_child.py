"""Child process of tests/test_gpu_dispatch_exits.py: the early exits of one otg_*_files entry point (argv[1]) on fixtures in argv[2].

For every failing writer — the text writer refusing its first call and its second, the warning writer of compare, the allele writer of
cohort — the call must raise OTG_ERR_ARG with the entry point's text, and the same job run again in this process with the collecting
writer must give the bytes of the untouched run: the contexts went back to the pool, no thread or handle leaked into the next job.  Then a
BAM / VCF path that does not exist: the code and text of the opener.  Every fixture has at least three batches, so a prefetch thread
exists when the second call is refused.  assemble / cohort run on two shards of device 0 with one region per batch: 11 and 12 (cohort:
6 and 6) batches per shard against an ordered output that holds back 3, and the writer that refuses a later call first sits on it for
SHARD_FILL_S seconds — by then both shards have filled their outputs, their hot-path threads wait in deliver() and their ingest
threads in push(), and that is the state the refusal has to release.
The refusing writers get into the job through _lib._run_files_job's `sink` and `callbacks` parameters (run_with below).
Prints one line per case and "ok" at the end; any failed assertion ends it with a traceback and a non-zero exit."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import otter_amd                                    # noqa: E402
from otter_amd import _lib, abi, bamwrite           # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# what a shard needs to finish the 3 batches its output holds back and one more per hot-path thread: a one-region batch takes
# milliseconds, the two contexts a second shard of the same device creates anew in every job up to a second each
SHARD_FILL_S = 3.0


def refusing_after(n_ok, n_args=3, wait_s=0.0):
    """a writer callback that accepts n_ok calls and refuses every later one, after wait_s seconds"""
    calls = [0]

    def w3(_user, _data, _n):
        calls[0] += 1
        if calls[0] <= n_ok:
            return 0
        time.sleep(wait_s)
        return 1

    def w4(_user, _sample, _data, _n):
        return w3(_user, _data, _n)
    return w3 if n_args == 3 else w4


def run_with(call, sink=None, **field_writers):
    """call() with the text writer replaced by `sink` and the job's further callbacks (by field name) by `field_writers`"""
    orig = _lib._run_files_job

    def patched(fn_name, job, job_type, callbacks=None, _sink=None):
        cbs = dict(callbacks or {})
        for field, fn in field_writers.items():
            cbs[field] = (cbs[field][0], fn)
        return orig(fn_name, job, job_type, cbs or None, sink=sink)
    _lib._run_files_job = patched
    try:
        return call()
    finally:
        _lib._run_files_job = orig


def expect_error(what, call, fn_name, text):
    try:
        call()
    except otter_amd.OtterGpuError as e:
        assert str(e) == "%s failed (%d): %s" % (fn_name, abi.OTG_ERR_ARG, text), (what, str(e))
        print("%-28s -> %s" % (what, e), flush=True)
        return
    raise AssertionError("%s: %s did not fail" % (what, fn_name))


def cases(name, tmp):
    """-> (fn_name, call, {case: kwargs of run_with}, call with a missing input, its error text)"""
    if name in ("assemble", "assemble_fasta_out"):
        fx = bamwrite.make_tr_fixture(tmp, 23, depth=12, len_range=(300, 900), seed=5)
        kw = dict(read_group="s1", offset_l=1, offset_r=1, mapq=10, threads=4, batch_regions=1, devices=[0, 0], is_fasta=name == "assemble_fasta_out")
        missing = os.path.join(tmp, "missing.bam")
        return ("otg_assemble_files", lambda: otter_amd.assemble_files(fx["bam"], fx["bed"], **kw),
                {"the writer failed": [dict(sink=refusing_after(0)), dict(sink=refusing_after(1, wait_s=SHARD_FILL_S))]},
                lambda: otter_amd.assemble_files(missing, fx["bed"], **kw), "otg_bam_open(%s): cannot open" % missing)
    if name in ("genotype", "genotype_table"):
        g = json.load(open(os.path.join(GOLDEN, "genotype_ref.json")))
        bed = os.path.join(tmp, "g.bed")
        with open(bed, "w") as f:
            f.write("".join("%s\t%d\t%d\n" % tuple(r) for r in g["regions"]))
        assert len(g["regions"]) >= 9
        fasta = os.path.join(GOLDEN, "genotype_small.fa") if name == "genotype" else None
        kw = dict(fasta=fasta, threads=3, batch_regions=3)
        missing = os.path.join(tmp, "missing.bam")
        return ("otg_genotype_files", lambda: otter_amd.genotype_files(os.path.join(GOLDEN, "genotype_small.bam"), bed, **kw),
                {"the writer failed": [dict(sink=refusing_after(0)), dict(sink=refusing_after(1))]},
                lambda: otter_amd.genotype_files(missing, bed, **kw), "otg_bam_open(%s): cannot open" % missing)
    if name == "cohort":
        import cohort_helpers
        fx = cohort_helpers.golden_fixture(tmp)
        kw = dict(batch_regions=1, devices=[0, 0], threads=3, alleles=True)
        missing = os.path.join(tmp, "missing.bam")
        return ("otg_cohort_files", lambda: otter_amd.cohort_files(fx["bams"], fx["names"], fx["bed"], fx["fasta"], **kw),
                {"the writer failed": [dict(sink=refusing_after(0)), dict(sink=refusing_after(1, wait_s=SHARD_FILL_S))],
                 "the allele writer failed": [dict(allele_write=refusing_after(0, 4)), dict(allele_write=refusing_after(len(fx["bams"]), 4, wait_s=SHARD_FILL_S))]},
                lambda: otter_amd.cohort_files(fx["bams"][:1] + [missing] + fx["bams"][2:], fx["names"], fx["bed"], fx["fasta"], **kw),
                "otg_bam_open(%s): cannot open" % missing)
    if name == "compare":
        import pathlib
        import test_gpu_compare
        bed, tb, qb, _lines = test_gpu_compare._fixture(pathlib.Path(tmp))
        kw = dict(threads=2, batch_regions=7)
        missing = os.path.join(tmp, "missing.bam")
        return ("otg_compare_files", lambda: otter_amd.compare_files(tb, qb, bed, **kw),
                {"the writer failed": [dict(sink=refusing_after(0)), dict(sink=refusing_after(1))],
                 "the warning writer failed": [dict(warn=refusing_after(0)), dict(warn=refusing_after(1))]},
                lambda: otter_amd.compare_files(tb, missing, bed, **kw), "otg_bam_open(%s): cannot open" % missing)
    if name == "vcf2mat":
        bed = os.path.join(tmp, "t.bed")
        with open(bed, "w") as f:
            f.write("chr1\t100\t200\n")
        vcf = os.path.join(GOLDEN, "vcf2mat_small.vcf.gz")
        kw = dict(k=3, threads=2, batch_alleles=3)
        missing = os.path.join(tmp, "missing.vcf.gz")
        return ("otg_vcf2mat_files", lambda: otter_amd.vcf2mat_files(vcf, bed, **kw),
                {"the writer failed": [dict(sink=refusing_after(0)), dict(sink=refusing_after(1))]},
                lambda: otter_amd.vcf2mat_files(missing, bed, **kw), "otg_vcf_open: cannot open %s" % missing)
    raise SystemExit("unknown entry point " + name)


def main():
    name, tmp = sys.argv[1], sys.argv[2]
    fn_name, call, failing, call_missing, missing_text = cases(name, tmp)
    t0 = time.time()
    good = call()
    print("%s: untouched run %.2f s, %d bytes" % (name, time.time() - t0, len(good[0])), flush=True)
    assert len(good[0]) > 0

    def same_as_good(got):
        # everything but the statistics (whose times differ from run to run): the text and what the further writers collected
        return [x for x in got if not isinstance(x, dict)] == [x for x in good if not isinstance(x, dict)]
    good_writer_only = len(sys.argv) > 3 and sys.argv[3] == "--good-writer"      # the same runs with no refusal: what the parent's time limit is sized by
    for text, variants in failing.items():
        for i, kw in enumerate(variants):
            what = "%s, %s call" % (text, ("first", "a later")[i])
            if good_writer_only:
                assert same_as_good(call())
            else:
                expect_error(what, lambda: run_with(call, **kw), fn_name, "%s: %s" % (fn_name, text))
            assert same_as_good(call()), "the run after '%s' differs from the untouched one" % what
    expect_error("missing input", call_missing, fn_name, missing_text)
    assert same_as_good(call())
    print("%s: child %.2f s" % (name, time.time() - t0), flush=True)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
