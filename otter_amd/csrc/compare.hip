// compare.hip — `otter compare` region logic (src/compare.cpp:50-66,106-146): host code, no device work.
//
// Per BED region: the truth alleles (exactly two, or the region is skipped), the query alleles (one is duplicated), every
// truth x query pair aligned end-to-end with the longer sequence as the pattern (ties: the query), the pairs sorted by
// (edit, ops) with std::sort and the reference's comparator, then the best pair and the best pair disjoint from it printed.
#include "otg_common.hpp"
#include "otg_compare.hpp"
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace {

struct DistEdge {            // DistCompare (src/compare.cpp:17-24)
  int i, j;
  double edit, ops;
};

void put_g(std::string& out, double x)
{
  char b[64];
  snprintf(b, sizeof(b), "%g", x);         // ostream's default for a double: %g, 6 significant digits
  out += b;
}

} // namespace

bool otg_compare_special(const uint8_t* s, uint32_t sl, const uint8_t* q, uint32_t ql, double* edit, double* ops)
{
  // get_distances (src/compare.cpp:56-57): equal alleles and the "N" / "NDNNN" placeholders are not aligned
  auto is = [](const uint8_t* x, uint32_t l, const char* w) { const size_t n = strlen(w); return l == n && memcmp(x, w, n) == 0; };
  const bool eq = sl == ql && (sl == 0 || memcmp(s, q, sl) == 0);
  const size_t qs = ql;
  if (eq || (is(s, sl, "N") && is(q, ql, "NDNNN")) || (is(q, ql, "N") && is(s, sl, "NDNNN"))) { *edit = 0; *ops = (double)qs; return true; }
  if (is(s, sl, "N") || is(q, ql, "N") || is(s, sl, "NDNNN") || is(q, ql, "NDNNN")) { *edit = (double)(size_t)(qs - 1); *ops = (double)qs; return true; }
  return false;
}

uint32_t otg_compare_n_pairs(uint32_t n_truth, uint32_t n_query)
{
  if (n_truth != 2 || n_query == 0) return 0;
  return 2u * (n_query == 1 ? 2u : n_query);
}

extern "C" int otg_compare_emit(const otg_bed* beds, const char* chr_arena, uint32_t n_regions,
                                const uint32_t* truth_first, const otg_allele* truth, const uint8_t* truth_seqs,
                                const uint32_t* span_first, const int32_t* spannings,
                                const uint32_t* query_first, const otg_allele* query, const uint8_t* query_seqs,
                                const uint64_t* pair_first, const double* pair_edit, const double* pair_ops,
                                char* out, uint64_t out_capacity, uint64_t* out_len,
                                char* warn, uint64_t warn_capacity, uint64_t* warn_len, otg_compare_counts* counts)
{
  if ((n_regions && (!beds || !chr_arena || !truth_first || !span_first || !query_first || !pair_first)) || !out_len)
    return otg_fail(nullptr, OTG_ERR_ARG, "otg_compare_emit: null argument");
  std::string text, wtext;
  otg_compare_counts cnt{};
  std::vector<DistEdge> edges;
  for (uint32_t r = 0; r < n_regions; ++r) {
    const std::string region = std::string(chr_arena + beds[r].chr_off, beds[r].chr_len) + ":" + std::to_string((uint32_t)beds[r].start) + "-" +
                               std::to_string((uint32_t)beds[r].end);          // BED::toScString
    const uint32_t nt = truth_first[r + 1] - truth_first[r], nq0 = query_first[r + 1] - query_first[r];
    const uint32_t np = otg_compare_n_pairs(nt, nq0);
    // src/compare.cpp:107-110, in that order
    const char* skip = nullptr;
    if (nt > 2) { skip = "WARNING: skipping region due to multiple expected alignments (>2) for region: "; ++cnt.skip_many_truth; }
    else if (nt == 1) { skip = "WARNING: skipping region due to single expected alignment for region: "; ++cnt.skip_one_truth; }
    else if (nt == 0) { skip = "WARNING: skipping region due no expected alignments for region: "; ++cnt.skip_no_truth; }
    else if (nq0 == 0) { skip = "WARNING: skipping region due no query alleles for region: "; ++cnt.skip_no_query; }
    if (skip) { wtext += skip; wtext += region; wtext += '\n'; continue; }
    if (pair_first[r + 1] - pair_first[r] != np || !pair_edit || !pair_ops)
      return otg_fail(nullptr, OTG_ERR_ARG, "otg_compare_emit: region %u needs %u pairs, pair_first gives %llu", r, np,
                      (unsigned long long)(pair_first[r + 1] - pair_first[r]));
    ++cnt.n_compared;
    // the query list with its first allele duplicated when it is the only one (src/compare.cpp:106)
    const uint32_t nq = nq0 == 1 ? 2 : nq0;
    auto qa = [&](uint32_t j) -> const otg_allele& { return query[query_first[r] + (nq0 == 1 ? 0 : j)]; };
    edges.clear();
    uint64_t p = pair_first[r];
    for (uint32_t i = 0; i < nt; ++i) {
      const otg_allele& ta = truth[truth_first[r] + i];
      for (uint32_t j = 0; j < nq; ++j, ++p) {
        const otg_allele& qq = qa(j);
        DistEdge e{(int)i, (int)j, pair_edit[p], pair_ops[p]};
        otg_compare_special(truth_seqs + ta.seq_off, ta.seq_len, query_seqs + qq.seq_off, qq.seq_len, &e.edit, &e.ops);
        edges.push_back(e);
      }
    }
    // src/compare.cpp:114-117: std::sort itself (not stable above 16 elements, so the library's own sort decides ties)
    std::sort(edges.begin(), edges.end(), [](const DistEdge& x, const DistEdge& y) {
      if (x.edit == y.edit) return x.ops < y.ops;
      else return x.edit < y.edit;
    });
    uint32_t e1 = 1;
    const DistEdge& e0 = edges.front();
    for (; e1 < edges.size(); ++e1)
      if (edges[e1].i != e0.i && edges[e1].j != e0.j) break;
    for (uint32_t idx : {0u, e1}) {
      const DistEdge& m = edges[idx];
      const int32_t ns = (int32_t)(span_first[r + 1] - span_first[r]);
      // reference_spannings[min_edge.i] (src/compare.cpp:142); an index past the pushed values reads outside the vector there: -1 here
      const int32_t sp = m.i < ns ? spannings[span_first[r] + (uint32_t)m.i] : -1;
      text += region; text += '\t';
      text += std::to_string(truth[truth_first[r] + (uint32_t)m.i].seq_len); text += '\t';
      text += std::to_string(qa((uint32_t)m.j).seq_len); text += '\t';
      text += std::to_string(sp); text += '\t';
      put_g(text, m.edit); text += '\t';
      put_g(text, m.ops); text += '\n';
    }
  }
  if (counts) *counts = cnt;
  *out_len = text.size();                                          // (here as well: the sizing call learns it even where the warnings do not fit)
  if (warn_len) {
    *warn_len = wtext.size();
    if (wtext.size() > warn_capacity || (!warn && !wtext.empty())) return otg_fail(nullptr, OTG_ERR_CAPACITY, "otg_compare_emit: warning buffer too small");
    if (!wtext.empty()) memcpy(warn, wtext.data(), wtext.size());
  }
  return otg_text_out("otg_compare_emit", text, out, out_capacity, out_len);
}
