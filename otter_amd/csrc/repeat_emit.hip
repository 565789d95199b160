// repeat_emit.hip — the host side of the repeat structure: the row text (otg_repeat_emit).  No device work; the kernels are repeat.hip.
#include "otg_common.hpp"
#include "otg_repeat.hpp"
#include "otg_repeat_core.hpp"
#include <string>

void otg_repeat_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint8_t* seq_arena,
                     const uint64_t* seq_off, const uint32_t* seq_len, const otg_repeat_sum* sums, const uint64_t* seg_off, const otg_repeat_seg* segs)
{
  char b[96];
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_vcf_record& R = records[r];
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      const uint8_t* s = seq_arena + seq_off[a];
      o.append(region_arena + R.region_off, R.region_len);
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%u\t%u\t", i, seq_len[a], sums[a].n_repeats, sums[a].covered));
      if (seg_off[a + 1] == seg_off[a]) o += '.';
      for (uint64_t g = seg_off[a]; g < seg_off[a + 1]; ++g) {
        const otg_repeat_seg& S = segs[g];
        if (S.period) {
          o += '(';
          for (uint32_t j = 0; j < S.period; ++j) o += "ACGTN"[otg_motif_core::mo_code(s[S.begin + j])];
          o.append(b, (size_t)snprintf(b, sizeof b, ")%u", S.copies));
        } else if (S.length <= OTG_REPEAT_TEXT_LITERAL) o.append((const char*)s + S.begin, S.length);
        else o.append(b, (size_t)snprintf(b, sizeof b, "[%u]", S.length));
      }
      o += '\n';
    }
  }
}

extern "C" int otg_repeat_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint8_t* seq_arena, const uint64_t* seq_off,
                               const uint32_t* seq_len, const otg_repeat_sum* sums, const uint64_t* seg_off, const otg_repeat_seg* segs, char* out,
                               uint64_t out_capacity, uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_repeat_emit: NULL out_len");
  if (n_records && (!records || !region_arena || !seq_off || !seq_len || !sums || !seg_off)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_repeat_emit: NULL argument");
  for (uint32_t r = 0; r < n_records; ++r)
    for (uint32_t i = 0; i < records[r].n_alleles; ++i) {
      const uint64_t a = (uint64_t)records[r].first_allele + i;
      if (seg_off[a + 1] < seg_off[a] || (seg_off[a + 1] > seg_off[a] && (!segs || !seq_arena)))
        return otg_fail(nullptr, OTG_ERR_ARG, "otg_repeat_emit: allele %u of record %u has segments and no segment or sequence array, or descending offsets", i, r);
      for (uint64_t g = seg_off[a]; g < seg_off[a + 1]; ++g)
        if (segs[g].begin > seq_len[a] || segs[g].length > seq_len[a] - segs[g].begin || segs[g].period > segs[g].length)
          return otg_fail(nullptr, OTG_ERR_ARG, "otg_repeat_emit: segment %llu of allele %u of record %u (begin %u, period %u, length %u) lies outside the allele of %u bases",
                          (unsigned long long)(g - seg_off[a]), i, r, segs[g].begin, segs[g].period, segs[g].length, seq_len[a]);
    }
  std::string text;
  otg_repeat_rows(text, records, n_records, region_arena, seq_arena, seq_off, seq_len, sums, seg_off, segs);
  return otg_text_out("otg_repeat_emit", text, out, out_capacity, out_len);
}
