// otter_merge — per-sample allele BAMs into the one `otter genotype` / `otter compare` read, through the C-ABI alone (include/otter_gpu.h,
// otg_bam_merge): the `samtools merge -pco` step of the reference's workflow.  Host C++ only; no device is needed.
//   otter_merge [-t threads] [-l level] OUT.bam IN.bam [IN.bam ...]
// Writes OUT.bam and OUT.bam.bai.  The inputs are coordinate-sorted BAMs with the same targets (what `otter_assemble --bam` and
// `otter_cohort --alleles-bam` write); a sample given twice, differing `@PG ID:otter OF:` offsets or target lists are refused.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../include/otter_gpu.h"

int main(int argc, char** argv)
{
  int threads = 1, level = -1;
  std::vector<const char*> paths;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> const char* { if (i + 1 >= argc) { fprintf(stderr, "[ERROR] %s needs a value\n", a.c_str()); exit(1); } return argv[++i]; };
    if (a == "-t" || a == "--threads") threads = atoi(val());
    else if (a == "-l" || a == "--level") level = atoi(val());
    else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "[ERROR] unknown option %s\n", a.c_str()); return 1; }
    else paths.push_back(argv[i]);
  }
  if (paths.size() < 2) { fprintf(stderr, "usage: otter_merge [-t threads] [-l level] <OUT.bam> <IN.bam> [<IN.bam> ...]\n"); return 1; }
  uint64_t n = 0;
  const int rc = otg_bam_merge(paths.data() + 1, (uint32_t)paths.size() - 1, paths[0], threads, level, &n);
  if (rc != OTG_OK) { fprintf(stderr, "[ERROR] otter_merge failed (%d): %s\n", rc, otg_last_error(nullptr)); return 1; }
  fprintf(stderr, "otter_merge: %llu records from %zu files in %s\n", (unsigned long long)n, paths.size() - 1, paths[0]);
  return 0;
}
