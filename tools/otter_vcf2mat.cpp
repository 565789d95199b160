// otter_vcf2mat — `otter vcf2mat` over the C-ABI (src/command_vcf2mat.cpp): [parameters] <VCF[.GZ]>
//   -b, --bed <file>          BED-formatted file of target regions (required; parsed and unused, as in the reference)
//   -k, --kmer-size <k>       k-mer size, 1..12 (default 3; the reference accepts up to 32)
//   -t, --threads <n>         host threads of the row formatting (default 1)
//       --batch <n>           alleles per device batch (default: sized from k)
// One row per allele to stdout, in file order.
#include "../include/otter_gpu.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int to_stream(void* user, const char* data, uint64_t len)
{
  return fwrite(data, 1, (size_t)len, (FILE*)user) == (size_t)len ? 0 : 1;
}

static void usage(const char* argv0)
{
  fprintf(stdout, "Usage: %s [parameters] <VCF[.GZ]>\n  -b, --bed <file>          BED-formatted file of target regions.\n"
                  "  -k, --kmer-size <k>       Kmer-size to use (default 3, at most %d).\n  -t, --threads <n>         Total threads to use (default 1).\n"
                  "      --batch <n>           Alleles per device batch (default: sized from k).\n", argv0, OTG_KMER_MAX);
}

// a whole decimal integer, as cxxopts parses an int option
static bool parse_int(const std::string& s, long long* v)
{
  if (s.empty()) return false;
  char* end = nullptr;
  *v = strtoll(s.c_str(), &end, 10);
  return *end == '\0';
}

int main(int argc, char** argv)
{
  std::string bed, ks = "3", ts = "1", bs = "0";
  bool have_bed = false;
  std::vector<std::string> inputs;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto value = [&](const char* s, const char* l, std::string& out) {
      if ((s && a == s) || a == l) {
        if (i + 1 >= argc) { fprintf(stdout, "Error parsing options: Option '%s' is missing an argument\n", l + 2); usage(argv[0]); exit(1); }
        out = argv[++i]; return true;
      }
      const std::string lp = std::string(l) + "=";
      if (a.compare(0, lp.size(), lp) == 0) { out = a.substr(lp.size()); return true; }
      return false;
    };
    if (value("-b", "--bed", bed)) { have_bed = true; continue; }
    if (value("-k", "--kmer-size", ks)) continue;
    if (value("-t", "--threads", ts)) continue;
    if (value(nullptr, "--batch", bs)) continue;
    inputs.push_back(a);
  }
  if (inputs.empty()) { usage(argv[0]); return 0; }
  long long k = 0, t = 0, b = 0;
  if (!parse_int(ks, &k) || !parse_int(ts, &t) || !parse_int(bs, &b) || b < 0) {
    fprintf(stdout, "Error parsing options: invalid integer argument\n"); usage(argv[0]); return 1;
  }
  if (!have_bed) { fprintf(stdout, "Error parsing options: Option 'bed' has no value\n"); usage(argv[0]); return 1; }
  if (k < 1 || k > OTG_KMER_MAX) {
    fprintf(stderr, "[ERROR] invalid '--kmer-size' (%lld). Needs to be 1 <= x <= %d.\n", k, OTG_KMER_MAX);
    return 1;
  }
  otg_vcf2mat_job job;
  memset(&job, 0, sizeof(job));
  job.vcf_path = inputs[0].c_str(); job.bed_path = bed.c_str();
  job.k = (int32_t)k; job.threads = t < 1 ? 1 : (int32_t)t; job.device = 0; job.batch_alleles = (uint32_t)b;
  otg_job_stats st;
  const int rc = otg_vcf2mat_files(&job, to_stream, stdout, &st);
  fflush(stdout);
  if (rc != OTG_OK) { fprintf(stderr, "otter_vcf2mat: %s\n", otg_last_error(nullptr)); return 1; }
  return 0;
}
