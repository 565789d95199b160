// otg_unitparse.hpp — the row text of `otter_unitparse`, shared by unitparse_emit.hip, locus_emit.hip and the dispatcher.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/otter_gpu.h"

// appends the rows of records[0 .. n_records) to o (the text of otg_unitparse_emit)
void otg_unitparse_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                        const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                        const otg_unitparse_sum* sums, const uint64_t* seg_off, const otg_unitparse_seg* segs);
// appends "counts \t structure" of one allele: K units (unit k = unit_len[k] bytes at unit_arena + unit_off[k]) and its n_segs segments
void otg_unitparse_counts(std::string& o, uint64_t K, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len, const otg_unitparse_seg* segs,
                          uint64_t n_segs);
// the refusals of an emit entry `who` over such rows: NULL arguments, empty or oversized sets, decreasing offsets, a segment outside its set
int otg_unitparse_rows_check(const char* who, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                             const uint32_t* allele_set, const uint64_t* set_first, const uint8_t* unit_arena, const uint64_t* unit_off, const uint32_t* unit_len,
                             const void* sums, const uint64_t* seg_off, const otg_unitparse_seg* segs);
