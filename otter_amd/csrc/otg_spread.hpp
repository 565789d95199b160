// otg_spread.hpp — the row text of the spread operator (spread_emit.hip).
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the rows of regions[0 .. n_regions) to o (the text of otg_spread_emit): region r's alleles are regions[r].first_allele .. + n_alleles
void otg_spread_rows(std::string& o, const otg_bed* beds, const char* chr_arena, uint32_t n_regions, const otg_region_result* regions, const otg_allele* alleles,
                     const uint32_t* region_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                     const otg_spread* records, const uint64_t* spread_unit_off, const otg_spread_unit* units);
