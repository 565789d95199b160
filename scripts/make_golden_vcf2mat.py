"""Writes the `otter vcf2mat` golden fixtures: tests/golden/vcf2mat_small.vcf.gz (a synthetic VCF with every case of the contract, see
tests/vcf2mat_fixtures.py) and the rows the reference's own seq2kcounts / KmerEncoding / KUSAGE::hsdiv give for it at k = 3 and k = 6
(tests/golden/vcf2mat_small_k{3,6}.txt.gz), through tests/vcf2mat_ref.cpp built against oracle/_ref/libotter_ref_io.so.  Run in the build
container (needs the reference for `make -C oracle`)."""
import gzip
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vcf2mat_fixtures as F  # noqa: E402


def main():
    vcf = os.path.join(F.GOLDEN, "vcf2mat_small.vcf.gz")
    F.write_golden_vcf(vcf, F.golden_lines(np.random.default_rng(2024)))
    with tempfile.TemporaryDirectory() as tmp:
        exe = F.build_driver(tmp, with_ref=True)
        assert exe is not None, "oracle/_ref/libotter_ref_io.so or the reference headers are missing"
        for k in (3, 6):
            txt = F.driver_text(exe, k, vcf)
            out = os.path.join(F.GOLDEN, "vcf2mat_small_k%d.txt.gz" % k)
            with gzip.GzipFile(out, "wb", mtime=0) as f:
                f.write(txt)
            print(out, len(txt), os.path.getsize(out))


if __name__ == "__main__":
    main()
