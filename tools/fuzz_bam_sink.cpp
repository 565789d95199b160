// fuzz_bam_sink — drives otg_bam_sink_* and otg_bam_merge (otter_amd/csrc/bam_sink.cpp, linked alone: no HIP, no library) over damaged
// input; built with -fsanitize=address,undefined (tests/test_bam_sink_sanitized.py).  Exit code 0 = every call came back with OTG_OK or
// an error code and the sanitizers saw nothing; a sanitizer report aborts the process.
//   fuzz_bam_sink <clean.sam> <scratch directory> [<clean.bam> <possibly damaged .bam> ...]
// The SAM text is fed to sinks as it is and under seeded mutations (byte flips, truncated lines, 20-digit numbers, tabs removed), in pieces
// of random sizes; every BAM after the first is merged with the first.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/otter_gpu.h"

static int feed(const std::string& text, const std::string& out, int sort, int threads, std::mt19937& rng, unsigned long long* records)
{
  otg_bam_sink* s = nullptr;
  otg_bam_sink_opts o; memset(&o, 0, sizeof o);
  o.sort = sort; o.threads = threads; o.level = 1;
  int rc = otg_bam_sink_open(out.c_str(), &o, &s);
  if (rc != OTG_OK) return rc;
  size_t at = 0;
  int wrc = OTG_OK;
  while (at < text.size()) {
    const size_t k = std::min<size_t>(text.size() - at, 1 + rng() % 5000);
    const int r = otg_bam_sink_write(s, text.data() + at, k);
    if (r != OTG_OK && wrc == OTG_OK) { wrc = r; if (!otg_bam_sink_error(s)[0]) { fprintf(stderr, "a refusal without a text\n"); exit(3); } }
    if (wrc != OTG_OK && r == OTG_OK) { fprintf(stderr, "a write after a refusal was accepted\n"); exit(3); }
    at += k;
  }
  uint64_t n = 0;
  if (rng() % 7 == 0) { otg_bam_sink_abort(s); return wrc; }
  rc = otg_bam_sink_close(s, &n);
  if (wrc != OTG_OK && rc == OTG_OK) { fprintf(stderr, "close after a refusal returned OTG_OK\n"); exit(3); }
  *records += n;
  return rc;
}

int main(int argc, char** argv)
{
  if (argc < 3) return 2;
  std::string clean;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) clean.append(buf, k);
    fclose(f);
  }
  const std::string dir = argv[2];
  std::mt19937 rng(20240917u);
  int errors = 0, calls = 0;
  unsigned long long records = 0;
  if (feed(clean, dir + "/clean.bam", 0, 2, rng, &records) != OTG_OK) { fprintf(stderr, "the clean text was refused\n"); return 3; }
  std::vector<size_t> line_start = {0};
  for (size_t i = 0; i + 1 < clean.size(); ++i) if (clean[i] == '\n') line_start.push_back(i + 1);
  for (int kind = 0; kind < 5; ++kind)
    for (int trial = 0; trial < 12; ++trial) {
      std::string t = clean;
      const int n_mut = 1 + (int)(rng() % 6);
      for (int m = 0; m < n_mut; ++m) {
        const size_t ls = line_start[rng() % line_start.size()];
        size_t le = t.find('\n', std::min(ls, t.size()));
        if (le == std::string::npos) le = t.size();
        if (ls >= le) continue;
        const size_t at = ls + rng() % (le - ls);
        if (kind == 0) t[at] = (char)(t[at] ^ (1 << (rng() % 8)));                              // a flipped bit
        else if (kind == 1) t[at] = (char)(rng() % 256);                                        // any byte
        else if (kind == 2) t.erase(at, (le - at) + (rng() % 2));                               // a truncated line (with or without its newline)
        else if (kind == 3) {                                                                   // a 20-digit number in place of a number
          size_t a = at;
          while (a < le && !(t[a] >= '0' && t[a] <= '9')) ++a;
          size_t b = a;
          while (b < le && t[b] >= '0' && t[b] <= '9') ++b;
          if (a < b) t.replace(a, b - a, (rng() % 2) ? "98765432109876543210" : "-9876543210987654321");
        } else {                                                                                 // a tab removed
          const size_t tab = t.find('\t', at);
          if (tab != std::string::npos && tab < le) t.erase(tab, 1);
        }
        if (kind == 2 || kind == 3 || kind == 4) {                                              // offsets moved: find the lines again
          line_start.assign(1, 0);
          for (size_t i = 0; i + 1 < t.size(); ++i) if (t[i] == '\n') line_start.push_back(i + 1);
        }
      }
      ++calls;
      if (feed(t, dir + "/mut.bam", trial % 2, 1 + trial % 3, rng, &records) != OTG_OK) ++errors;
      line_start.assign(1, 0);
      for (size_t i = 0; i + 1 < clean.size(); ++i) if (clean[i] == '\n') line_start.push_back(i + 1);
    }
  int merge_errors = 0, merges = 0;
  for (int i = 4; i < argc; ++i) {
    const char* in[2] = {argv[3], argv[i]};
    uint64_t n = 0;
    ++merges;
    if (otg_bam_merge(in, 2, (dir + "/merged.bam").c_str(), 1 + i % 3, 1, &n) != OTG_OK) ++merge_errors;
    const char* rev[2] = {argv[i], argv[3]};
    if (otg_bam_merge(rev, 2, (dir + "/merged.bam").c_str(), 1, -1, &n) != OTG_OK) ++merge_errors;
  }
  printf("done: %d of %d mutated texts refused, %llu records written; %d of %d merges refused\n", errors, calls, records, merge_errors, 2 * merges);
  return 0;
}
