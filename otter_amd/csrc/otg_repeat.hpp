// otg_repeat.hpp — the row text of `otter_repeats`, shared by repeat_emit.hip and the dispatcher.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the rows of records[0 .. n_records) to o (the text of otg_repeat_emit); every segment lies inside its allele
void otg_repeat_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint8_t* seq_arena,
                     const uint64_t* seq_off, const uint32_t* seq_len, const otg_repeat_sum* sums, const uint64_t* seg_off, const otg_repeat_seg* segs);
