// otg_locus.hpp — the row text of `otter_loci`, shared by locus_emit.hip and the dispatcher.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the rows of records[0 .. n_records) to o (the text of otg_locus_emit)
void otg_locus_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                    const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                    const otg_locus* loci, const uint64_t* seg_off, const otg_unitparse_seg* segs);
