"""Writes tests/golden/cohort_small_k3.mat: the rows `otter vcf2mat -k 3` prints for the committed joint VCF tests/golden/cohort_small.vcf, by
the reference's own seq2kcounts / KmerEncoding / KUSAGE::hsdiv through tests/vcf2mat_ref.cpp built against oracle/_ref/libotter_ref_io.so
(no device code of the product).  Run in the build container (needs the reference for `make -C oracle`)."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vcf2mat_fixtures as F  # noqa: E402
import cohort_helpers as H  # noqa: E402
import cohort_matrix_helpers as M  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = F.build_driver(tmp, with_ref=True)
        assert exe is not None, "oracle/_ref/libotter_ref_io.so or the reference headers are missing"
        txt = F.driver_text(exe, M.GOLDEN_MAT_K, H.GOLDEN_VCF)
    with open(M.GOLDEN_MAT, "wb") as f:
        f.write(txt)
    print(M.GOLDEN_MAT, txt.count(b"\n"), "rows,", len(txt), "bytes")


if __name__ == "__main__":
    main()
