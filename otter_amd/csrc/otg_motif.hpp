// otg_motif.hpp — the row text of `otter_motifs`, shared by motif_emit.hip and the dispatcher.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the rows of records[0 .. n_records) to o (the text of otg_motif_emit)
void otg_motif_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                    const otg_motif* motifs, const uint8_t* units, uint32_t unit_stride);
