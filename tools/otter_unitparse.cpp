// otter_unitparse — the joint parse of the alleles of a VCF against the unit sets of a tandem-repeat catalogue over the C-ABI:
// [parameters] <VCF[.GZ]>
//   -b, --bed <file>          BED-formatted catalogue (required); column 4 carries the units: CAG, CAG,CCG or ID=HTT;MOTIFS=CAG,CCG;...
//   -t, --threads <n>         host threads of the row formatting (default 1)
//       --batch <n>           alleles per device batch (default 65536)
// One row per allele to stdout, in file order: region, allele index, length, units, edits, switches, unit bases, identity, copies per unit,
// structure, e.g. (CAG)20~1(CCG)7.
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
  fprintf(stdout, "Usage: %s [parameters] <VCF[.GZ]>\n  -b, --bed <file>          BED-formatted catalogue; column 4 carries the repeat units of a region.\n"
                  "  -t, --threads <n>         Total threads to use (default 1).\n"
                  "      --batch <n>           Alleles per device batch (default 65536).\n", argv0);
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
  std::string bed, ts = "1", bs = "0";
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
    if (value("-t", "--threads", ts)) continue;
    if (value(nullptr, "--batch", bs)) continue;
    inputs.push_back(a);
  }
  if (inputs.empty()) { usage(argv[0]); return 0; }
  long long t = 0, b = 0;
  if (!parse_int(ts, &t) || !parse_int(bs, &b) || b < 0) {
    fprintf(stdout, "Error parsing options: invalid integer argument\n"); usage(argv[0]); return 1;
  }
  if (!have_bed) { fprintf(stdout, "Error parsing options: Option 'bed' has no value\n"); usage(argv[0]); return 1; }
  otg_unitparse_job job;
  memset(&job, 0, sizeof(job));
  job.vcf_path = inputs[0].c_str(); job.bed_path = bed.c_str();
  job.threads = t < 1 ? 1 : (int32_t)t; job.device = 0;
  job.batch_alleles = b > 0xffffffffLL ? 0xffffffffu : (uint32_t)b;
  otg_job_stats st;
  const int rc = otg_unitparse_files(&job, to_stream, stdout, &st);
  fflush(stdout);
  if (rc != OTG_OK) { fprintf(stderr, "otter_unitparse: %s\n", otg_last_error(nullptr)); return 1; }
  return 0;
}
