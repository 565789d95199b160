// Calls the operator-level adapter the way compare.cpp does (src/compare.cpp:59-61,95): one WFAlignerEdit(Alignment, MemoryMed), alignEnd2End
// with the longer sequence first, then getAlignmentScore() and getAlignmentCigar().  stdin: "<pattern> <text>" per line ("-" = empty);
// stdout: "<status> <score> <op string or ->".  Built by tests/test_gpu_compare.py with g++ against libotter_gpu.so.
#include "bindings/cpp/WFAligner.hpp"

#include <iostream>
#include <string>

int main()
{
  wfa::WFAlignerEdit aligner(wfa::WFAligner::Alignment, wfa::WFAligner::MemoryMed);
  std::string p, t;
  while (std::cin >> p >> t) {
    if (p == "-") p.clear();
    if (t == "-") t.clear();
    const int st = aligner.alignEnd2End(p, t);
    if (st != 0) { std::cerr << "adapter: " << aligner.strError() << "\n"; return 3; }
    const std::string cigar = aligner.getAlignmentCigar();
    std::cout << st << " " << aligner.getAlignmentScore() << " " << (cigar.empty() ? "-" : cigar) << "\n";
  }
  return 0;
}
