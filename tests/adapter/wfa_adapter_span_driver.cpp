// Calls WFAlignerEdit(Alignment) of the operator-level adapter (include/wfa_adapter/bindings/cpp/WFAligner.hpp) on pairs read from stdin,
// one per line:
//   <pattern> <text> <endsfree 0|1> <pbf> <pef> <tbf> <tef>      ("-" = empty sequence)
// and prints per pair:  <status> <score> <op string or ->
// With arguments `wfadaptive <min_wavefront_length> <max_distance_threshold> <steps>` the aligner first gets setHeuristicWFadaptive, with
// `none` setHeuristicNone.  Built by tests/test_wfa_adapter_span.py with g++ against libotter_gpu.so; the test compares every line with
// the CPU restatement of the ends-free edit alignment.
#include "bindings/cpp/WFAligner.hpp"

#include <cstdlib>
#include <iostream>
#include <string>

int main(int argc, char** argv)
{
  wfa::WFAlignerEdit aligner(wfa::WFAligner::Alignment, wfa::WFAligner::MemoryMed);
  if (argc >= 5 && std::string(argv[1]) == "wfadaptive") aligner.setHeuristicWFadaptive(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
  else if (argc >= 2 && std::string(argv[1]) == "none") aligner.setHeuristicNone();
  std::string p, t;
  int ef, pbf, pef, tbf, tef;
  while (std::cin >> p >> t >> ef >> pbf >> pef >> tbf >> tef) {
    if (p == "-") p.clear();
    if (t == "-") t.clear();
    const int st = ef ? aligner.alignEndsFree(p, pbf, pef, t, tbf, tef) : aligner.alignEnd2End(p, t);
    if (st != 0) { std::cerr << "adapter: " << aligner.strError() << "\n"; return 3; }
    const std::string cigar = aligner.getAlignmentCigar();
    std::cout << st << " " << aligner.getAlignmentScore() << " " << (cigar.empty() ? "-" : cigar) << "\n";
  }
  return 0;
}
