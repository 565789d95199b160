// unitparse_emit.hip — the host side of the joint unit parse: the row text (otg_unitparse_emit).  No device work; the kernels are unitparse.hip.
#include "otg_common.hpp"
#include "otg_unitparse.hpp"
#include <algorithm>
#include <string>

void otg_unitparse_counts(std::string& o, uint64_t K, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len, const otg_unitparse_seg* segs,
                          uint64_t n_segs)
{
  char b[64];
  uint64_t per_unit[OTG_UNITPARSE_MAX_UNITS];
  for (uint64_t k = 0; k < K; ++k) per_unit[k] = 0;
  for (uint64_t g = 0; g < n_segs; ++g) per_unit[segs[g].unit] += segs[g].unit_bases;
  for (uint64_t k = 0; k < K; ++k) o.append(b, (size_t)snprintf(b, sizeof b, "%s%.2f", k ? "," : "", (double)per_unit[k] / (double)unit_len[k]));
  o += '\t';
  if (n_segs == 0) o += '.';
  for (uint64_t g = 0; g < n_segs; ++g) {
    const otg_unitparse_seg& G = segs[g];
    const uint32_t p = unit_len[G.unit];
    o += '(';
    o.append((const char*)unit_arena + unit_off[G.unit], p);
    o += ')';
    if (G.unit_bases % p == 0u) o.append(b, (size_t)snprintf(b, sizeof b, "%u", G.unit_bases / p));
    else o.append(b, (size_t)snprintf(b, sizeof b, "%.2f", (double)G.unit_bases / (double)p));
    if (G.edits) o.append(b, (size_t)snprintf(b, sizeof b, "~%u", G.edits));
  }
}

void otg_unitparse_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                        const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                        const otg_unitparse_sum* sums, const uint64_t* seg_off, const otg_unitparse_seg* segs)
{
  char b[128];
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_vcf_record& R = records[r];
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      const uint32_t q = allele_set[a];
      const uint64_t u0 = q == OTG_UNITPARSE_NO_SET ? 0 : set_first[q], K = q == OTG_UNITPARSE_NO_SET ? 0 : set_first[q + 1] - u0;
      const uint32_t L = seq_len[a];
      o.append(region_arena + R.region_off, R.region_len);
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t", i, L));
      if (K == 0) {
        o += ".\t0\t0\t0\t0.0000\t.\t.\n";
        continue;
      }
      const otg_unitparse_sum& A = sums[a];
      for (uint64_t k = 0; k < K; ++k) {
        if (k) o += ',';
        o.append((const char*)unit_arena + unit_off[u0 + k], unit_len[u0 + k]);
      }
      const uint32_t span = std::max(L, A.unit_bases);
      const double identity = A.flags == 0u && span ? 1.0 - (double)A.edits / (double)span : 0.0;
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%u\t%.4f\t", A.edits, A.switches, A.unit_bases, identity));
      otg_unitparse_counts(o, K, unit_arena, unit_off + u0, unit_len + u0, segs + seg_off[a], seg_off[a + 1] - seg_off[a]);
      o += '\n';
    }
  }
}

int otg_unitparse_rows_check(const char* who, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                             const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                             const void* sums, const uint64_t* seg_off, const otg_unitparse_seg* segs)
{
  if (n_records && (!records || !region_arena || !seq_len || !allele_set)) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL argument", who);
  for (uint32_t r = 0; r < n_records; ++r)
    for (uint32_t i = 0; i < records[r].n_alleles; ++i) {
      const uint64_t a = (uint64_t)records[r].first_allele + i;
      const uint32_t q = allele_set[a];
      if (q == OTG_UNITPARSE_NO_SET) continue;
      if (!set_first) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL argument", who);
      if (set_first[q + 1] <= set_first[q]) return otg_fail(nullptr, OTG_ERR_ARG, "%s: set %u of allele %u of record %u is empty", who, q, i, r);
      const uint64_t K = set_first[q + 1] - set_first[q];
      if (K > OTG_UNITPARSE_MAX_UNITS) return otg_fail(nullptr, OTG_ERR_ARG, "%s: allele %u of record %u has %llu units, at most %d", who, i, r,
                                                       (unsigned long long)K, OTG_UNITPARSE_MAX_UNITS);
      if (!unit_arena || !unit_off || !unit_len || !sums || !seg_off) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL argument", who);
      for (uint64_t k = set_first[q]; k < set_first[q + 1]; ++k)
        if (unit_len[k] == 0u) return otg_fail(nullptr, OTG_ERR_ARG, "%s: allele %u of record %u has an empty unit", who, i, r);
      if (seg_off[a + 1] < seg_off[a]) return otg_fail(nullptr, OTG_ERR_ARG, "%s: seg_off decreases at allele %u of record %u", who, i, r);
      if (seg_off[a + 1] > seg_off[a] && !segs) return otg_fail(nullptr, OTG_ERR_ARG, "%s: NULL argument", who);
      for (uint64_t g = seg_off[a]; g < seg_off[a + 1]; ++g)
        if (segs[g].unit >= K) return otg_fail(nullptr, OTG_ERR_ARG, "%s: segment %llu of allele %u of record %u names unit %u of %llu", who,
                                               (unsigned long long)(g - seg_off[a]), i, r, segs[g].unit, (unsigned long long)K);
    }
  return OTG_OK;
}

extern "C" int otg_unitparse_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                                  const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                                  const otg_unitparse_sum* sums, const uint64_t* seg_off, const otg_unitparse_seg* segs, char* out, uint64_t out_capacity,
                                  uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitparse_emit: NULL out_len");
  if (int rc = otg_unitparse_rows_check("otg_unitparse_emit", records, n_records, region_arena, seq_len, allele_set, set_first, unit_arena, unit_off, unit_len, sums, seg_off,
                                        segs))
    return rc;
  std::string text;
  otg_unitparse_rows(text, records, n_records, region_arena, seq_len, allele_set, set_first, unit_arena, unit_off, unit_len, sums, seg_off, segs);
  return otg_text_out("otg_unitparse_emit", text, out, out_capacity, out_len);
}
