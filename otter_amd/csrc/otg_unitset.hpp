// otg_unitset.hpp — the catalogue text of `otter_units`, shared by unitset_emit.hip and the dispatcher.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the catalogue lines of records[0 .. n_records) to o (the text of otg_unitset_emit): record r is group r (sets[r], set_first[r]),
// its first three columns those of beds[rec_bed[r]]
void otg_unitset_lines(std::string& o, const otg_vcf_record* records, uint32_t n_records, const uint32_t* rec_bed, const otg_bed* beds, const char* chr_arena,
                       const uint64_t* set_first, const otg_unitset_unit* units, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len);
