// unitalign_emit.hip — the host side of the unit alignment: the row text (otg_unitalign_emit).  No device work; the kernels are unitalign.hip.
#include "otg_common.hpp"
#include "otg_unitalign.hpp"
#include <algorithm>
#include <string>

void otg_unitalign_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                        const uint64_t* task_first, const uint8_t* task_source, const uint8_t* unit_arena, const uint64_t* task_unit_off,
                        const uint32_t* task_unit_len, const otg_unitalign* aligned)
{
  char b[96];
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_vcf_record& R = records[r];
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      for (uint64_t t = task_first[a]; t < task_first[a + 1]; ++t) {
        const otg_unitalign& A = aligned[t];
        const uint32_t p = task_unit_len[t], L = seq_len[a];
        o.append(region_arena + R.region_off, R.region_len);
        o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%s\t", i, L, task_source[t] == OTG_UNITALIGN_SOURCE_BED ? "bed" : "motif"));
        if (p) o.append((const char*)unit_arena + task_unit_off[t], p);
        else o += '.';
        const uint32_t span = std::max(L, A.unit_bases);
        const bool counted = p != 0u && A.flags == 0u;
        const double copies = counted ? (double)A.unit_bases / (double)p : 0.0;
        const double identity = counted && span ? 1.0 - (double)A.edits / (double)span : 0.0;
        o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%.2f\t%.4f\n", A.edits, A.unit_bases, copies, identity));
      }
    }
  }
}

extern "C" int otg_unitalign_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                                  const uint64_t* task_first, const uint8_t* task_source, const uint8_t* unit_arena, const uint64_t* task_unit_off,
                                  const uint32_t* task_unit_len, const otg_unitalign* aligned, char* out, uint64_t out_capacity, uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitalign_emit: NULL out_len");
  if (n_records && (!records || !region_arena || !seq_len || !task_first)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitalign_emit: NULL argument");
  for (uint32_t r = 0; r < n_records; ++r)
    for (uint32_t i = 0; i < records[r].n_alleles; ++i) {
      const uint64_t a = (uint64_t)records[r].first_allele + i;
      if (task_first[a + 1] < task_first[a]) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitalign_emit: task_first decreases at allele %u of record %u", i, r);
      if (task_first[a + 1] > task_first[a] && (!task_source || !task_unit_off || !task_unit_len || !aligned || !unit_arena))
        return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitalign_emit: NULL argument");
    }
  std::string text;
  otg_unitalign_rows(text, records, n_records, region_arena, seq_len, task_first, task_source, unit_arena, task_unit_off, task_unit_len, aligned);
  return otg_text_out("otg_unitalign_emit", text, out, out_capacity, out_len);
}
