// spread_emit.hip — the host side of the spread operator: the row text (otg_spread_emit).  No device work; the kernels are spread.hip.
#include "otg_common.hpp"
#include "otg_spread.hpp"
#include <string>

void otg_spread_rows(std::string& o, const otg_bed* beds, const char* chr_arena, uint32_t n_regions, const otg_region_result* regions, const otg_allele* alleles,
                     const uint32_t* region_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                     const otg_spread* records, const uint64_t* spread_unit_off, const otg_spread_unit* units)
{
  char b[256];
  std::string name;
  for (uint32_t r = 0; r < n_regions; ++r) {
    const otg_region_result& R = regions[r];
    if (R.n_alleles == 0) continue;
    name.clear();
    otg_region_name(name, chr_arena + beds[r].chr_off, beds[r].chr_len, beds[r].start, beds[r].end);
    const uint32_t s = region_set[r];
    const uint64_t u0 = s == OTG_SPREAD_NONE ? 0 : set_first[s], K = s == OTG_SPREAD_NONE ? 0 : set_first[s + 1] - u0;
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      const otg_spread& S = records[a];
      o += name;
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%d\t%u\t", alleles[a].label, alleles[a].seq_len));
      if (K == 0) o += '.';
      for (uint64_t k = 0; k < K; ++k) {
        if (k) o += ',';
        o.append((const char*)unit_arena + unit_off[u0 + k], unit_len[u0 + k]);
      }
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%llu\t%llu\t", S.n_reads, S.n_called, S.ref_bases, S.q[0], S.q[1], S.q[2], S.q[3],
                                   S.q[4], S.n_below, S.n_above, (unsigned long long)S.sum_below, (unsigned long long)S.sum_above));
      if (K == 0) o += '.';
      for (uint64_t k = 0; k < K; ++k) {
        const otg_spread_unit& U = units[spread_unit_off[a] + k];
        const double p = (double)unit_len[u0 + k];
        if (k) o += ',';
        o.append((const char*)unit_arena + unit_off[u0 + k], unit_len[u0 + k]);
        o.append(b, (size_t)snprintf(b, sizeof b, ":%.2f:%.2f/%.2f/%.2f/%.2f/%.2f", (double)U.ref_bases / p, (double)U.q[0] / p, (double)U.q[1] / p, (double)U.q[2] / p,
                                     (double)U.q[3] / p, (double)U.q[4] / p));
      }
      o += '\n';
    }
  }
}

extern "C" int otg_spread_emit(const otg_bed* beds, const char* chr_arena, uint32_t n_regions, const otg_region_result* regions, const otg_allele* alleles,
                               const uint32_t* region_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                               const otg_spread* records, const uint64_t* spread_unit_off, const otg_spread_unit* units, char* out, uint64_t out_capacity,
                               uint64_t* out_len)
{
  const char* who = "otg_spread_emit";
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL out_len", who);
  if (n_regions && (!beds || !chr_arena || !regions || !region_set)) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL argument", who);
  for (uint32_t r = 0; r < n_regions; ++r) {
    if (regions[r].n_alleles == 0) continue;
    if (!alleles || !records) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL argument", who);
    const uint32_t s = region_set[r];
    if (s == OTG_SPREAD_NONE) continue;
    if (!set_first || !unit_arena || !unit_off || !unit_len || !spread_unit_off || !units) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL argument", who);
    const uint64_t K = set_first[s + 1] - set_first[s];
    if (set_first[s + 1] <= set_first[s]) return otg_fail(nullptr, OTG_ERR_ARG, "%s: set %u of region %u is empty", who, s, r);
    for (uint64_t k = set_first[s]; k < set_first[s + 1]; ++k)
      if (unit_len[k] == 0u) return otg_fail(nullptr, OTG_ERR_ARG, "%s: region %u has an empty unit", who, r);
    for (uint32_t i = 0; i < regions[r].n_alleles; ++i) {
      const uint64_t a = (uint64_t)regions[r].first_allele + i;
      if (spread_unit_off[a + 1] - spread_unit_off[a] != K)
        return otg_fail(nullptr, OTG_ERR_ARG, "%s: allele %u of region %u has %llu unit records, its set has %llu units", who, i, r,
                        (unsigned long long)(spread_unit_off[a + 1] - spread_unit_off[a]), (unsigned long long)K);
    }
  }
  std::string text;
  otg_spread_rows(text, beds, chr_arena, n_regions, regions, alleles, region_set, set_first, unit_arena, unit_off, unit_len, records, spread_unit_off, units);
  return otg_text_out(who, text, out, out_capacity, out_len);
}
