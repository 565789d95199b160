// otg_vcf2mat.hpp — the row text of `otter vcf2mat`, shared by vcf2mat.hip and the dispatcher.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the rows of records[0 .. n_records) to o (the text of otg_vcf2mat_emit).  first_index: the allele number of the first row of records[0],
// above 0 for a record whose earlier alleles went out with another call (the cohort matrix walks its rows in ranges, dispatch.hip)
void otg_vcf2mat_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                      int32_t k, const double* usage, const double* gc, const double* hsd, uint32_t first_index = 0);
