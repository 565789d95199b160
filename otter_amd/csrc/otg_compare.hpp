// otg_compare.hpp — pieces of the `otter compare` region logic shared by compare.hip and the dispatcher.
#pragma once
#include <cstdint>

// get_distances' pairs that are not aligned (src/compare.cpp:56-57): true with their (edit, ops) when (truth s, query q) is one of them
bool otg_compare_special(const uint8_t* s, uint32_t sl, const uint8_t* q, uint32_t ql, double* edit, double* ops);
// pairs of a region otg_compare_emit expects (0 for a skipped region)
uint32_t otg_compare_n_pairs(uint32_t n_truth, uint32_t n_query);
