// vcf2mat_ref.cpp — test infrastructure: `otter vcf2mat` (src/vcf2mat.cpp:16-77) restated on the CPU, one thread.
//   vcf2mat_ref text K VCF            the rows, as the reference prints them, to stdout
//   vcf2mat_ref values K VCF OUT      per allele the doubles gc, hsd and the 4^K+1 frequencies, binary, to OUT
// The VCF is read through zlib's gz* reader (plain, gzip, BGZF); a last line without '\n' is read too.  Built plainly, the k-mer counts,
// KUSAGE and hsdiv are restated here (the CPU baseline of scripts/bench_vcf2mat.py and the GPU tests' restatement).  Built with
// -DOTG_REF_ANSEQS against the reference's headers and oracle/_ref/libotter_ref_io.so, they are the reference's own seq2kcounts,
// KmerEncoding and KUSAGE::hsdiv; only the line loop below is restated then.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <zlib.h>
#ifdef OTG_REF_ANSEQS
#include "anseqs.hpp"
#endif

namespace {

#ifndef OTG_REF_ANSEQS
struct KmerEncoding {
  uint8_t nt2encoding[256];
  KmerEncoding()
  {
    for (int i = 0; i < 256; ++i) nt2encoding[i] = 4;
    nt2encoding['A'] = nt2encoding['a'] = 0; nt2encoding['C'] = nt2encoding['c'] = 1;
    nt2encoding['G'] = nt2encoding['g'] = 2; nt2encoding['T'] = nt2encoding['t'] = 3;
  }
};

// a window of k bytes -> its base-4 code (first base most significant), 4^k when a byte is outside ACGTacgt
void seq2kcounts(const uint32_t& k, const KmerEncoding& enc, const std::string& seq, std::vector<double>& counts)
{
  const uint32_t nb = 1u << (2 * k);
  counts.assign(nb + 1, 0.0);
  if (seq.size() < k) return;
  for (size_t j = 0; j + k <= seq.size(); ++j) {
    uint64_t idx = 0;
    bool ok = true;
    for (uint32_t h = 0; h < k; ++h) {
      const uint8_t e = enc.nt2encoding[(uint8_t)seq[j + h]];
      if (e == 4) { ok = false; break; }
      idx = 4 * idx + e;
    }
    counts[ok ? idx : nb] += 1;
  }
}

struct KUSAGE {
  std::vector<double> vec;
  explicit KUSAGE(const std::vector<double>& c) : vec(c.size(), 0)
  {
    int total = 0;                                   // an int sum of the counts
    for (double x : c) total += x;
    for (size_t i = 0; i < vec.size(); ++i) vec[i] = c[i] / total;
  }
  double hsdiv() const
  {
    double acc = 0;
    for (double v : vec) if (v > 0) acc += v * std::log(v);
    acc = -1 * acc;
    return std::pow(M_E, acc);
  }
};
#endif

void split(const std::string& s, char d, std::vector<std::string>& out)
{
  std::string v;
  std::istringstream is(s);
  while (std::getline(is, v, d)) out.emplace_back(v);
}

void parse_alleles(const std::string& line, std::string& region, std::vector<std::string>& alleles)
{
  std::string col;
  std::istringstream is(line);
  int index = 0;
  while (std::getline(is, col, '\t')) {
    if (index == 2) region = col;
    else if (index == 3) alleles.emplace_back(col);
    else if (index == 4 && col != ".") {
      if (col == "<DEL>") alleles.emplace_back("N"); else split(col, ',', alleles);
    }
    ++index;
  }
}

double gc_content(const KmerEncoding& enc, const std::string& seq)
{
  double gc = 0;
  for (char c : seq) { const uint8_t e = enc.nt2encoding[(uint8_t)c]; if (e == 1 || e == 2) gc += 1; }
  return gc / seq.size();
}

} // namespace

int main(int argc, char** argv)
{
  if (argc < 4) { fprintf(stderr, "usage: %s text|values K VCF [OUT]\n", argv[0]); return 2; }
  const std::string mode = argv[1];
  const uint32_t k = (uint32_t)atoi(argv[2]);
  gzFile f = gzopen(argv[3], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }
  FILE* vout = nullptr;
  if (mode == "values") { if (argc < 5 || !(vout = fopen(argv[4], "wb"))) return 1; }
  std::string data;
  {
    std::vector<char> buf(1 << 20);
    int n;
    while ((n = gzread(f, buf.data(), (unsigned)buf.size())) > 0) data.append(buf.data(), (size_t)n);
    gzclose(f);
    if (n < 0) return 1;
  }
  KmerEncoding encoding;
  std::ostream& os = std::cout;
  size_t p = 0;
  while (p < data.size()) {
    size_t e = data.find('\n', p);
    if (e == std::string::npos) e = data.size();
    const std::string line = data.substr(p, e - p);
    p = e + 1;
    if (!line.empty() && line.front() == '#') continue;
    std::vector<std::string> alleles;
    std::string region;
    parse_alleles(line, region, alleles);
    for (uint32_t i = 0; i < alleles.size(); ++i) {
      std::vector<double> kcounts;
      seq2kcounts(k, encoding, alleles[i], kcounts);
      KUSAGE kusage(kcounts);
      const double gc = gc_content(encoding, alleles[i]), hsd = kusage.hsdiv();
      if (vout) {
        fwrite(&gc, 8, 1, vout); fwrite(&hsd, 8, 1, vout);
        fwrite(kusage.vec.data(), 8, kusage.vec.size(), vout);
        continue;
      }
      os << region << '\t' << i << '\t' << gc << '\t' << alleles[i].size() << '\t' << hsd;
      for (const auto& ku : kusage.vec) os << '\t' << ku;
      os << '\n';
    }
  }
  if (vout) fclose(vout);
  os.flush();
  return 0;
}
