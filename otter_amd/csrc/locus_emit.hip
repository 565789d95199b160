// locus_emit.hip — the host side of the locus mode: the row text (otg_locus_emit).  No device work; the kernels are locus.hip.
#include "otg_common.hpp"
#include "otg_locus.hpp"
#include "otg_unitparse.hpp"
#include <algorithm>
#include <string>

void otg_locus_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                    const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                    const otg_locus* loci, const uint64_t* seg_off, const otg_unitparse_seg* segs)
{
  char b[160];
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_vcf_record& R = records[r];
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      const uint32_t q = allele_set[a];
      const uint64_t u0 = q == OTG_UNITPARSE_NO_SET ? 0 : set_first[q], K = q == OTG_UNITPARSE_NO_SET ? 0 : set_first[q + 1] - u0;
      o.append(region_arena + R.region_off, R.region_len);
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t", i, seq_len[a]));
      if (K == 0) {
        o += ".\t0\t0\t0\t0\t0\t0\t0.0000\t.\t.\n";
        continue;
      }
      const otg_locus& A = loci[a];
      for (uint64_t k = 0; k < K; ++k) {
        if (k) o += ',';
        o.append((const char*)unit_arena + unit_off[u0 + k], unit_len[u0 + k]);
      }
      const uint32_t span = std::max(A.end - A.begin, A.unit_bases);
      const double identity = A.flags == 0u && span ? 1.0 - (double)A.edits / (double)span : 0.0;
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%u\t%u\t%u\t%u\t%.4f\t", A.begin, A.end, A.score, A.edits, A.switches, A.unit_bases, identity));
      otg_unitparse_counts(o, K, unit_arena, unit_off + u0, unit_len + u0, segs + seg_off[a], seg_off[a + 1] - seg_off[a]);
      o += '\n';
    }
  }
}

extern "C" int otg_locus_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len, const uint32_t* allele_set,
                              const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len, const otg_locus* loci,
                              const uint64_t* seg_off, const otg_unitparse_seg* segs, char* out, uint64_t out_capacity, uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_locus_emit: NULL out_len");
  if (int rc = otg_unitparse_rows_check("otg_locus_emit", records, n_records, region_arena, seq_len, allele_set, set_first, unit_arena, unit_off, unit_len, loci, seg_off, segs))
    return rc;
  std::string text;
  otg_locus_rows(text, records, n_records, region_arena, seq_len, allele_set, set_first, unit_arena, unit_off, unit_len, loci, seg_off, segs);
  return otg_text_out("otg_locus_emit", text, out, out_capacity, out_len);
}
