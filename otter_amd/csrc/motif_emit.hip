// motif_emit.hip — the host side of the motif annotation: the row text (otg_motif_emit).  No device work; the kernels are motif.hip.
#include "otg_common.hpp"
#include "otg_motif.hpp"
#include <string>

void otg_motif_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                    const otg_motif* motifs, const uint8_t* units, uint32_t unit_stride)
{
  char b[96];
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_vcf_record& R = records[r];
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      const otg_motif& M = motifs[a];
      o.append(region_arena + R.region_off, R.region_len);
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%u\t", i, seq_len[a], M.period));
      if (M.period) o.append((const char*)units + a * unit_stride, M.period);
      else o += '.';
      const double copies = M.period ? (double)seq_len[a] / (double)M.period : 0.0;
      const double purity = M.period ? (double)M.matches / (double)M.compared : 0.0;
      o.append(b, (size_t)snprintf(b, sizeof b, "\t%.2f\t%.4f\n", copies, purity));
    }
  }
}

extern "C" int otg_motif_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                              const otg_motif* motifs, const uint8_t* units, uint32_t unit_stride, char* out, uint64_t out_capacity, uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_motif_emit: NULL out_len");
  if (n_records && (!records || !region_arena || !seq_len || !motifs || !units)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_motif_emit: NULL argument");
  for (uint32_t r = 0; r < n_records; ++r)
    for (uint32_t i = 0; i < records[r].n_alleles; ++i)
      if (motifs[(uint64_t)records[r].first_allele + i].period > unit_stride)
        return otg_fail(nullptr, OTG_ERR_ARG, "otg_motif_emit: allele %u of record %u has period %u, unit_stride is %u", i, r,
                        motifs[(uint64_t)records[r].first_allele + i].period, unit_stride);
  std::string text;
  otg_motif_rows(text, records, n_records, region_arena, seq_len, motifs, units, unit_stride);
  return otg_text_out("otg_motif_emit", text, out, out_capacity, out_len);
}
