"""otter_amd — MI355X-native drop-in for otter's per-region alignment / clustering / consensus hot path.

The product is libotter_gpu.so (hand-written HIP for gfx950 behind the C-ABI of include/otter_gpu.h);
this package is the thin host-side mirror used by tests and bench.py.  No CPU fallback exists."""
from . import abi, synth  # noqa: F401
from ._lib import Context, Comm, OtterGpuError, device_count, load, LIB_PATH, EXPORTS, emit_alleles, emit_sam_header, Bam  # noqa: F401
from ._lib import Fasta, parse_bed_file, bed_tuples, emit_reads, assemble_files, assemble_files_release, assemble_batch_plan, genotype_files, wgat  # noqa: F401
from ._lib import emit_vcf_header, emit_vcf_lines, emit_genotype_lengths, genotype_blocks, compare_emit, compare_files  # noqa: F401
from ._lib import vcf_read_alleles, vcf2mat_emit, vcf2mat_files, cohort_files, BamSink, merge_bams  # noqa: F401
from ._lib import exp_host, exp_probe  # noqa: F401
from .abi import default_params  # noqa: F401
from ._lib import motif_emit, motifs_files  # noqa: F401
from ._lib import repeat_emit, repeats_files  # noqa: F401
from ._lib import parse_bed_units, unitalign_emit, copies_files  # noqa: F401
from ._lib import tract_emit, tracts_files  # noqa: F401
from ._lib import unitparse_emit, unitparse_files  # noqa: F401
from ._lib import locus_emit, loci_files  # noqa: F401
from ._lib import unitset_emit, units_files  # noqa: F401
from ._lib import spread_emit, spread_files  # noqa: F401
