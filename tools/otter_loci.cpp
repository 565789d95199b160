// otter_loci — the joint parse of the repeat inside every allele of a VCF against the unit sets of a tandem-repeat catalogue over the C-ABI:
// [parameters] <VCF[.GZ]>
//   -b, --bed <file>          BED-formatted catalogue (required); column 4 carries the units: CAG, CAG,CCG or ID=HTT;MOTIFS=CAG,CCG;...
//       --scores <m,x,g>      match, mismatch and indel scores of the local alignment, 1..16, 1..64, 1..64 (default 2,7,7)
//       --min-score <n>       the lowest score that counts as a tract, 0..16777216 (default 24)
//       --discover            a region without units in the catalogue (a three-column BED has none) gets the unit set discovered from its
//                             alleles, in one pass: repeat structure, discovery, locus mode; the catalogue's units are kept where it has some
//   -p <n>                    with --discover: longest repeat unit looked for, 1..4096 (default 256)
//       --min-copies <n>      with --discover: fewest whole copies of a repeat segment, 2..1024 (default 2)
//       --min-span <n>        with --discover: fewest bases of a repeat segment, 2..65535 (default 12)
//       --min-bases <n>       with --discover: fewest bases of a unit's segments in a region, 1..16777216 (default 12)
//       --min-share <n>       with --discover: fewest bases as a share of the region's largest unit, per mille, 0..1000 (default 50)
//       --redundant <n>       with --discover: edits per 1000 bases of a doubled unit that a higher-ranked unit explains, 0..1000 (default 100)
//   -t, --threads <n>         host threads of the row formatting (default 1)
//       --batch <n>           alleles per device batch (default 65536)
// One row per allele to stdout, in file order: region, allele index, length, units, tract begin, tract end, score, edits, switches, unit
// bases, identity, copies per unit, structure.  Flank bases around the tract count for nothing; otter_unitparse parses the whole allele.
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
  fprintf(stdout, "Usage: %s [parameters] <VCF[.GZ]>\n  -b, --bed <file>          BED-formatted catalogue; column 4 carries the repeat units.\n"
                  "      --scores <m,x,g>      Match, mismatch and indel scores of the local alignment (default 2,7,7).\n"
                  "      --min-score <n>       Lowest score that counts as a tract (default 24).\n"
                  "      --discover            Discover the units of regions the catalogue has none for from their alleles.\n"
                  "  -p <n>                    With --discover: longest repeat unit to look for (default 256, at most %d).\n"
                  "      --min-copies <n>      With --discover: fewest whole copies of a repeat segment (default 2).\n"
                  "      --min-span <n>        With --discover: fewest bases of a repeat segment (default 12).\n"
                  "      --min-bases <n>       With --discover: fewest bases of a unit's segments in a region (default 12).\n"
                  "      --min-share <n>       With --discover: fewest bases as a share of the region's largest unit, per mille (default 50).\n"
                  "      --redundant <n>       With --discover: edits per 1000 bases of a doubled unit that a higher-ranked unit explains (default 100).\n"
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
  std::string bed, cs = "2,7,7", ms = "24", ts = "1", bs = "0", ps = "256", ks = "2", ss = "12", mb = "12", sh = "50", rd = "100";
  bool have_bed = false, discover = false, discover_switch = false;
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
    if (value(nullptr, "--scores", cs)) continue;
    if (value(nullptr, "--min-score", ms)) continue;
    if (value("-t", "--threads", ts)) continue;
    if (value(nullptr, "--batch", bs)) continue;
    if (a == "--discover") { discover = true; continue; }
    if (value("-p", "--max-period", ps) || value(nullptr, "--min-copies", ks) || value(nullptr, "--min-span", ss) || value(nullptr, "--min-bases", mb) ||
        value(nullptr, "--min-share", sh) || value(nullptr, "--redundant", rd)) { discover_switch = true; continue; }
    inputs.push_back(a);
  }
  if (inputs.empty()) { usage(argv[0]); return 0; }
  long long m = 0, t = 0, b = 0, sc[3] = {0, 0, 0};
  // the three scores: whole integers between two commas
  const size_t c1 = cs.find(','), c2 = c1 == std::string::npos ? c1 : cs.find(',', c1 + 1);
  const bool scores_ok = c2 != std::string::npos && parse_int(cs.substr(0, c1), &sc[0]) && parse_int(cs.substr(c1 + 1, c2 - c1 - 1), &sc[1]) &&
                         parse_int(cs.substr(c2 + 1), &sc[2]);
  if (!parse_int(ms, &m) || !parse_int(ts, &t) || !parse_int(bs, &b) || b < 0 || !scores_ok) {
    fprintf(stdout, "Error parsing options: invalid integer argument\n"); usage(argv[0]); return 1;
  }
  if (!have_bed) { fprintf(stdout, "Error parsing options: Option 'bed' has no value\n"); usage(argv[0]); return 1; }
  long long dp = 0, dk = 0, ds = 0, dm = 0, dh = 0, dr = 0;
  if (!parse_int(ps, &dp) || !parse_int(ks, &dk) || !parse_int(ss, &ds) || !parse_int(mb, &dm) || !parse_int(sh, &dh) || !parse_int(rd, &dr)) {
    fprintf(stdout, "Error parsing options: invalid integer argument\n"); usage(argv[0]); return 1;
  }
  if (discover_switch && !discover) { fprintf(stdout, "Error parsing options: a discovery parameter needs '--discover'\n"); usage(argv[0]); return 1; }
  if (sc[0] < 1 || sc[0] > 16 || sc[1] < 1 || sc[1] > 64 || sc[2] < 1 || sc[2] > 64) {
    fprintf(stderr, "[ERROR] invalid '--scores' (%lld,%lld,%lld). Needs to be 1 <= match <= 16, 1 <= mismatch <= 64, 1 <= indel <= 64.\n", sc[0], sc[1], sc[2]);
    return 1;
  }
  if (m < 0 || m > (1 << 24)) {
    fprintf(stderr, "[ERROR] invalid '--min-score' (%lld). Needs to be 0 <= x <= %d.\n", m, 1 << 24);
    return 1;
  }
  otg_loci_job job;
  memset(&job, 0, sizeof(job));
  job.vcf_path = inputs[0].c_str(); job.bed_path = bed.c_str();
  job.threads = t < 1 ? 1 : (int32_t)t; job.device = 0;
  job.match = (uint32_t)sc[0]; job.mismatch = (uint32_t)sc[1]; job.indel = (uint32_t)sc[2]; job.min_score = (uint32_t)m;
  job.batch_alleles = b > 0xffffffffLL ? 0xffffffffu : (uint32_t)b;
  otg_job_stats st;
  int rc;
  if (discover) {
    if (!in_range("-p", dp, 1, OTG_REPEAT_MAX_PERIOD) || !in_range("--min-copies", dk, 2, 1024) || !in_range("--min-span", ds, 2, 65535) ||
        !in_range("--min-bases", dm, 1, 1 << 24) || !in_range("--min-share", dh, 0, 1000) || !in_range("--redundant", dr, 0, 1000))
      return 1;
    otg_units_job dj;                                               // (its paths are ignored)
    memset(&dj, 0, sizeof(dj));
    dj.max_period = (uint32_t)dp; dj.min_copies = (uint32_t)dk; dj.min_span = (uint32_t)ds;
    dj.min_bases = (uint32_t)dm; dj.min_share = (uint32_t)dh; dj.redundant = (uint32_t)dr;
    rc = otg_units_loci_files(&job, &dj, to_stream, stdout, &st);
  } else
    rc = otg_loci_files(&job, to_stream, stdout, &st);
  fflush(stdout);
  if (rc != OTG_OK) { fprintf(stderr, "otter_loci: %s\n", otg_last_error(nullptr)); return 1; }
  return 0;
}
