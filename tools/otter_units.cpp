// otter_units — the repeat units of the regions of a VCF, discovered from the repeat structure of their alleles, over the C-ABI:
// [parameters] <VCF[.GZ]>
//   -b, --bed <file>          BED-formatted file of target regions (required; gives the first three columns)
//   -p, --max-period <n>      longest repeat unit looked for, 1..4096 (default 256; units over 256 bases are not candidates)
//       --min-copies <n>      fewest whole copies of a repeat segment, 2..1024 (default 2)
//       --min-span <n>        fewest bases of a repeat segment, 2..65535 (default 12)
//       --min-bases <n>       fewest bases of a unit's segments in a region, 1..16777216 (default 12)
//       --min-share <n>       fewest bases as a share of the region's largest unit, per mille, 0..1000 (default 50)
//       --redundant <n>       edits per 1000 bases of a unit written twice that a higher-ranked unit still explains, 0..1000 (default 100)
//   -t, --threads <n>         host threads of the row formatting (default 1)
//       --batch <n>           alleles per device batch (default 65536)
// One catalogue line per VCF record to stdout, in file order: chrom, start, end, MOTIFS=..;BASES=..;SEGMENTS=..;ALLELES=n ("." without a
// set).  The output is a catalogue BED for otter_copies, otter_tracts, otter_unitparse and otter_loci.
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
                  "  -p, --max-period <n>      Longest repeat unit to look for (default 256, at most %d).\n"
                  "      --min-copies <n>      Fewest whole copies of a repeat segment (default 2).\n"
                  "      --min-span <n>        Fewest bases of a repeat segment (default 12).\n"
                  "      --min-bases <n>       Fewest bases of a unit's segments in a region (default 12).\n"
                  "      --min-share <n>       Fewest bases as a share of the region's largest unit, per mille (default 50).\n"
                  "      --redundant <n>       Edits per 1000 bases of a doubled unit that a higher-ranked unit explains (default 100).\n"
                  "  -t, --threads <n>         Total threads to use (default 1).\n"
                  "      --batch <n>           Alleles per device batch (default 65536).\n", argv0, OTG_REPEAT_MAX_PERIOD);
}

// a whole decimal integer, as cxxopts parses an int option
static bool parse_int(const std::string& s, long long* v)
{
  if (s.empty()) return false;
  char* end = nullptr;
  *v = strtoll(s.c_str(), &end, 10);
  return *end == '\0';
}

static bool in_range(const char* name, long long v, long long lo, long long hi)
{
  if (v >= lo && v <= hi) return true;
  fprintf(stderr, "[ERROR] invalid '%s' (%lld). Needs to be %lld <= x <= %lld.\n", name, v, lo, hi);
  return false;
}

int main(int argc, char** argv)
{
  std::string bed, ps = "256", cs = "2", ss = "12", mb = "12", sh = "50", rd = "100", ts = "1", bs = "0";
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
    if (value("-p", "--max-period", ps)) continue;
    if (value(nullptr, "--min-copies", cs)) continue;
    if (value(nullptr, "--min-span", ss)) continue;
    if (value(nullptr, "--min-bases", mb)) continue;
    if (value(nullptr, "--min-share", sh)) continue;
    if (value(nullptr, "--redundant", rd)) continue;
    if (value("-t", "--threads", ts)) continue;
    if (value(nullptr, "--batch", bs)) continue;
    inputs.push_back(a);
  }
  if (inputs.empty()) { usage(argv[0]); return 0; }
  long long p = 0, c = 0, s = 0, m = 0, h = 0, r = 0, t = 0, b = 0;
  if (!parse_int(ps, &p) || !parse_int(cs, &c) || !parse_int(ss, &s) || !parse_int(mb, &m) || !parse_int(sh, &h) || !parse_int(rd, &r) || !parse_int(ts, &t) ||
      !parse_int(bs, &b) || b < 0) {
    fprintf(stdout, "Error parsing options: invalid integer argument\n"); usage(argv[0]); return 1;
  }
  if (!have_bed) { fprintf(stdout, "Error parsing options: Option 'bed' has no value\n"); usage(argv[0]); return 1; }
  if (!in_range("--max-period", p, 1, OTG_REPEAT_MAX_PERIOD) || !in_range("--min-copies", c, 2, 1024) || !in_range("--min-span", s, 2, 65535) ||
      !in_range("--min-bases", m, 1, 1 << 24) || !in_range("--min-share", h, 0, 1000) || !in_range("--redundant", r, 0, 1000))
    return 1;
  otg_units_job job;
  memset(&job, 0, sizeof(job));
  job.vcf_path = inputs[0].c_str(); job.bed_path = bed.c_str();
  job.max_period = (uint32_t)p; job.min_copies = (uint32_t)c; job.min_span = (uint32_t)s;
  job.min_bases = (uint32_t)m; job.min_share = (uint32_t)h; job.redundant = (uint32_t)r;
  job.threads = t < 1 ? 1 : (int32_t)t; job.device = 0;
  job.batch_alleles = b > 0xffffffffLL ? 0xffffffffu : (uint32_t)b;
  otg_job_stats st;
  const int rc = otg_units_files(&job, to_stream, stdout, &st);
  fflush(stdout);
  if (rc != OTG_OK) { fprintf(stderr, "otter_units: %s\n", otg_last_error(nullptr)); return 1; }
  return 0;
}
