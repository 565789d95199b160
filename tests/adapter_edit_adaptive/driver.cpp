// Calls the operator-level adapter the way compare.cpp would against a WFA2-lib whose aligners run wfadaptive (src/compare.cpp:59-61,95): one
// WFAlignerEdit(Alignment, MemoryMed), setHeuristicWFadaptive(argv[1], argv[2], argv[3]), alignEnd2End with the longer sequence first, then
// getAlignmentScore() and getAlignmentCigar(); after the last pair, setHeuristicNone() on the SAME object and every pair once more.
// stdin: "<pattern> <text>" per line ("-" = empty); stdout: "<status> <score> <op string or ->" per pair, the adaptive lines first, then the
// exact ones.  Built by tests/test_gpu_compare_adaptive.py with g++ against libotter_gpu.so.
#include "bindings/cpp/WFAligner.hpp"

#include <cstdlib>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

int main(int argc, char** argv)
{
  if (argc != 4) { std::cerr << "usage: driver <min_wavefront_length> <max_distance_threshold> <steps_between_cutoffs>\n"; return 2; }
  wfa::WFAlignerEdit aligner(wfa::WFAligner::Alignment, wfa::WFAligner::MemoryMed);
  aligner.setHeuristicWFadaptive(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]));
  std::vector<std::pair<std::string, std::string>> pairs;
  std::string p, t;
  while (std::cin >> p >> t) {
    if (p == "-") p.clear();
    if (t == "-") t.clear();
    pairs.emplace_back(p, t);
  }
  for (int round = 0; round < 2; ++round) {
    if (round == 1) aligner.setHeuristicNone();
    for (auto& pr : pairs) {
      const int st = aligner.alignEnd2End(pr.first, pr.second);
      if (st != 0) { std::cerr << "adapter: " << aligner.strError() << "\n"; return 3; }
      const std::string cigar = aligner.getAlignmentCigar();
      std::cout << st << " " << aligner.getAlignmentScore() << " " << (cigar.empty() ? "-" : cigar) << "\n";
    }
  }
  return 0;
}
