// otg_tract.hpp — the row text of `otter_tracts`, shared by tract_emit.hip and the dispatcher.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the rows of records[0 .. n_records) to o (the text of otg_tract_emit)
void otg_tract_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                    const uint64_t* task_first, const uint8_t* task_source, const uint8_t* unit_arena, const uint64_t* task_unit_off,
                    const uint32_t* task_unit_len, const otg_tract* tracts);
