// otter_compare — `otter compare` over the C-ABI (src/command_compare.cpp): [parameters] <BAM> <BAM>
//   -b, --bed <file>          BED-formatted file of target regions (required)
//   -R, --sample-name <name>  parsed and unused, as in the reference
//   -t, --threads <n>         host threads of the ingest (default 1)
//   --wfa-heuristic none|wfadaptive[:min_wavefront_length,max_distance_threshold,steps]
//                             heuristic of the edit alignments, as otter_assemble's option of that name (default none = exact; wfadaptive = 10,50,1)
// The first BAM holds the truth alleles, the second the assembled ones.  Records go to stdout in BED order, warnings to stderr.
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
  fprintf(stdout, "Usage: %s [parameters] <BAM> <BAM>\n  -b, --bed <file>          BED-formatted file of target regions.\n"
                  "  -R, --sample-name <name>  Sample name.\n  -t, --threads <n>         Total number of threads (default 1).\n"
                  "  --wfa-heuristic <h>       none | wfadaptive[:min_wavefront_length,max_distance_threshold,steps] (default none).\n", argv0);
}

int main(int argc, char** argv)
{
  std::string bed, sample;
  int threads = 1;
  int heuristic = OTG_HEURISTIC_NONE, heur_p[3] = {10, 50, 1};
  std::vector<std::string> inputs;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto value = [&](const char* s, const char* l, std::string& out) {
      if (a == s || a == l) { if (i + 1 >= argc) { fprintf(stderr, "[ERROR] %s needs a value\n", l); exit(1); } out = argv[++i]; return true; }
      const std::string lp = std::string(l) + "=";
      if (a.compare(0, lp.size(), lp) == 0) { out = a.substr(lp.size()); return true; }
      return false;
    };
    std::string t;
    if (value("-b", "--bed", bed)) continue;
    if (value("-R", "--sample-name", sample)) continue;
    if (value("-t", "--threads", t)) { threads = atoi(t.c_str()); continue; }
    std::string h;
    if (value("--wfa-heuristic", "--wfa-heuristic", h)) {
      if (h == "none") heuristic = OTG_HEURISTIC_NONE;
      else if (h.rfind("wfadaptive", 0) == 0 && (h.size() == 10 || h[10] == ':')) {
        heuristic = OTG_HEURISTIC_WFADAPTIVE;
        if (h.size() > 10) {
          std::vector<std::string> v(1);
          for (char c : h.substr(11)) { if (c == ',') v.emplace_back(); else v.back() += c; }
          if (v.size() != 3) { fprintf(stderr, "[ERROR] --wfa-heuristic wfadaptive:<min_wavefront_length>,<max_distance_threshold>,<steps>\n"); return 1; }
          for (int q = 0; q < 3; ++q) heur_p[q] = atoi(v[q].c_str());
        }
      } else { fprintf(stderr, "[ERROR] --wfa-heuristic none | wfadaptive[:a,b,c]\n"); return 1; }
      continue;
    }
    inputs.push_back(a);
  }
  if (inputs.size() < 2) { usage(argv[0]); return 0; }
  if (bed.empty()) { fprintf(stderr, "[ERROR] '--bed' parameter required\n"); usage(argv[0]); return 1; }
  otg_compare_job job;
  memset(&job, 0, sizeof(job));
  job.truth_bam_path = inputs[0].c_str(); job.query_bam_path = inputs[1].c_str(); job.bed_path = bed.c_str();
  job.threads = threads < 1 ? 1 : threads; job.device = 0; job.batch_regions = 0;
  job.warn = to_stream; job.warn_user = stderr;
  job.heuristic = heuristic; job.heur_min_wavefront_length = heur_p[0]; job.heur_max_distance_threshold = heur_p[1]; job.heur_steps_between_cutoffs = heur_p[2];
  otg_job_stats st;
  const int rc = otg_compare_files(&job, to_stream, stdout, &st);
  fflush(stdout);
  if (rc != OTG_OK) { fprintf(stderr, "otter_compare: %s\n", otg_last_error(nullptr)); return 1; }
  return 0;
}
