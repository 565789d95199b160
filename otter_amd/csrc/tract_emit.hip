// tract_emit.hip — the host side of the tract mode: the row text (otg_tract_emit).  No device work; the kernels are tract.hip.
#include "otg_common.hpp"
#include "otg_tract.hpp"
#include <algorithm>
#include <string>

void otg_tract_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                    const uint64_t* task_first, const uint8_t* task_source, const uint8_t* unit_arena, const uint64_t* task_unit_off,
                    const uint32_t* task_unit_len, const otg_tract* tracts)
{
  char b[160];
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_vcf_record& R = records[r];
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      for (uint64_t t = task_first[a]; t < task_first[a + 1]; ++t) {
        const otg_tract& A = tracts[t];
        const uint32_t p = task_unit_len[t];
        o.append(region_arena + R.region_off, R.region_len);
        o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%s\t", i, seq_len[a], task_source[t] == OTG_UNITALIGN_SOURCE_BED ? "bed" : "motif"));
        if (p) o.append((const char*)unit_arena + task_unit_off[t], p);
        else o += '.';
        const uint32_t span = std::max(A.end - A.begin, A.unit_bases);
        const bool counted = p != 0u && A.flags == 0u;
        const double copies = counted ? (double)A.unit_bases / (double)p : 0.0;
        const double identity = counted && span ? 1.0 - (double)A.edits / (double)span : 0.0;
        o.append(b, (size_t)snprintf(b, sizeof b, "\t%u\t%u\t%u\t%u\t%u\t%.2f\t%.4f\n", A.begin, A.end, A.score, A.edits, A.unit_bases, copies, identity));
      }
    }
  }
}

extern "C" int otg_tract_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len, const uint64_t* task_first,
                              const uint8_t* task_source, const uint8_t* unit_arena, const uint64_t* task_unit_off, const uint32_t* task_unit_len,
                              const otg_tract* tracts, char* out, uint64_t out_capacity, uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_tract_emit: NULL out_len");
  if (n_records && (!records || !region_arena || !seq_len || !task_first)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_tract_emit: NULL argument");
  for (uint32_t r = 0; r < n_records; ++r)
    for (uint32_t i = 0; i < records[r].n_alleles; ++i) {
      const uint64_t a = (uint64_t)records[r].first_allele + i;
      if (task_first[a + 1] < task_first[a]) return otg_fail(nullptr, OTG_ERR_ARG, "otg_tract_emit: task_first decreases at allele %u of record %u", i, r);
      if (task_first[a + 1] > task_first[a] && (!task_source || !task_unit_off || !task_unit_len || !tracts || !unit_arena))
        return otg_fail(nullptr, OTG_ERR_ARG, "otg_tract_emit: NULL argument");
    }
  std::string text;
  otg_tract_rows(text, records, n_records, region_arena, seq_len, task_first, task_source, unit_arena, task_unit_off, task_unit_len, tracts);
  return otg_text_out("otg_tract_emit", text, out, out_capacity, out_len);
}
