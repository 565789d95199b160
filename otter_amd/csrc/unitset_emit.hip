// unitset_emit.hip — the host side of the unit-set discovery: the catalogue text (otg_unitset_emit).  No device work; the kernels are
// unitset.hip.
#include "otg_common.hpp"
#include "otg_unitset.hpp"
#include <string>
#include <unordered_map>
#include <vector>

void otg_unitset_lines(std::string& o, const otg_vcf_record* records, uint32_t n_records, const uint32_t* rec_bed, const otg_bed* beds, const char* chr_arena,
                       const uint64_t* set_first, const otg_unitset_unit* units, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len)
{
  char num[32];
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_bed& bed = beds[rec_bed[r]];
    o.append(chr_arena + bed.chr_off, bed.chr_len);
    o.append(num, (size_t)snprintf(num, sizeof num, "\t%u\t%u\t", (uint32_t)bed.start, (uint32_t)bed.end));
    const uint64_t k0 = set_first[r], K = set_first[r + 1] - k0;
    if (K == 0) {
      o += ".\n";
      continue;
    }
    o += "MOTIFS=";
    for (uint64_t k = 0; k < K; ++k) {
      if (k) o += ',';
      o.append((const char*)unit_arena + unit_off[k0 + k], unit_len[k0 + k]);
    }
    o += ";BASES=";
    for (uint64_t k = 0; k < K; ++k) o.append(num, (size_t)snprintf(num, sizeof num, "%s%llu", k ? "," : "", (unsigned long long)units[k0 + k].weight));
    o += ";SEGMENTS=";
    for (uint64_t k = 0; k < K; ++k) o.append(num, (size_t)snprintf(num, sizeof num, "%s%u", k ? "," : "", units[k0 + k].segments));
    o.append(num, (size_t)snprintf(num, sizeof num, ";ALLELES=%u\n", records[r].n_alleles));
  }
}

extern "C" int otg_unitset_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const otg_bed* beds, const char* chr_arena,
                                uint32_t n_beds, const otg_unitset* sets, const uint64_t* set_first, const otg_unitset_unit* units, const uint8_t* unit_arena,
                                const uint64_t* unit_off, const uint32_t* unit_len, char* out, uint64_t out_capacity, uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_emit: NULL out_len");
  if (n_records && (!records || !region_arena || !sets || !set_first || (n_beds && (!beds || !chr_arena))))
    return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_emit: NULL argument");
  // the first BED record of a region string wins, as in the catalogue lookup of otg_copies_files
  std::unordered_map<std::string, uint32_t> by_region;
  std::string name;
  for (uint32_t b = 0; b < n_beds; ++b) {
    name.clear();
    otg_region_name(name, chr_arena + beds[b].chr_off, beds[b].chr_len, beds[b].start, beds[b].end);
    by_region.emplace(name, b);
  }
  std::vector<uint32_t> rec_bed(n_records);
  for (uint32_t r = 0; r < n_records; ++r) {
    name.assign(region_arena + records[r].region_off, records[r].region_len);
    const auto it = by_region.find(name);
    if (it == by_region.end()) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_emit: no BED record for the region %s", name.c_str());
    rec_bed[r] = it->second;
    const uint64_t K = set_first[r + 1] - set_first[r];
    if (set_first[r + 1] < set_first[r] || K != sets[r].n_units)
      return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_emit: set %u has %u units, set_first gives it %llu", r, sets[r].n_units, (unsigned long long)K);
    if (K && (!units || !unit_arena || !unit_off || !unit_len)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_unitset_emit: NULL argument");
  }
  std::string text;
  otg_unitset_lines(text, records, n_records, rec_bed.data(), beds, chr_arena, set_first, units, unit_arena, unit_off, unit_len);
  return otg_text_out("otg_unitset_emit", text, out, out_capacity, out_len);
}
