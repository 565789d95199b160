// vcf2mat.hip — the host side of `otter vcf2mat` (src/vcf2mat.cpp:16-77, src/angzipiter.hpp): the VCF reader, parse_alleles and the row
// text.  No device work; the k-mer usage itself is kmer_usage.hip.
#include "otg_common.hpp"
#include "otg_vcf2mat.hpp"
#include <cmath>
#include <string>
#include <vector>
#include <zlib.h>

struct otg_vcf {
  gzFile f = nullptr;
  std::vector<char> buf;
  size_t pos = 0, end = 0;
  bool eof = false;
  // a parsed record that did not fit the caller's buffers: returned first by the next call
  bool pending = false;
  std::string region;
  std::vector<std::string> alleles;
  uint64_t pending_bytes = 0;
};

namespace {

constexpr size_t VCF_CHUNK = 1 << 20;

// the next line without its '\n' (GZIPiter::next); a last line without '\n' is returned too.  false at the end of the file.
int next_line(otg_vcf* v, std::string& line, bool* got, uint64_t* bytes)
{
  line.clear();
  *got = false;
  for (;;) {
    if (v->pos < v->end) {
      const char* p = v->buf.data() + v->pos;
      const char* nl = (const char*)memchr(p, '\n', v->end - v->pos);
      if (nl) {
        line.append(p, nl);
        *bytes += (uint64_t)(nl - p) + 1;
        v->pos += (size_t)(nl - p) + 1;
        *got = true;
        return OTG_OK;
      }
      line.append(p, v->end - v->pos);
      *bytes += v->end - v->pos;
      v->pos = v->end;
      *got = true;          // a partial line: more may follow
    }
    if (v->eof) return OTG_OK;
    const int n = gzread(v->f, v->buf.data(), (unsigned)v->buf.size());
    if (n < 0) { int e = 0; const char* m = gzerror(v->f, &e); return otg_fail(nullptr, OTG_ERR_ARG, "VCF read error: %s", m ? m : "?"); }
    v->pos = 0; v->end = (size_t)n;
    if (n == 0) v->eof = true;
  }
}

// std::getline(stream, field, delim) over the whole string: an empty trailing field is not produced
template <class F>
void split_getline(const char* p, size_t n, char delim, F f)
{
  size_t i = 0;
  while (i < n) {
    const char* q = (const char*)memchr(p + i, delim, n - i);
    const size_t j = q ? (size_t)(q - p) : n;
    f(p + i, j - i);
    i = j + 1;
  }
}

// parse_alleles (src/vcf2mat.cpp:23-36)
void parse_alleles(const std::string& line, std::string& region, std::vector<std::string>& alleles)
{
  region.clear();
  alleles.clear();
  int index = 0;
  split_getline(line.data(), line.size(), '\t', [&](const char* c, size_t n) {
    if (index == 2) region.assign(c, n);
    else if (index == 3) alleles.emplace_back(c, n);
    else if (index == 4 && !(n == 1 && c[0] == '.')) {
      if (n == 5 && memcmp(c, "<DEL>", 5) == 0) alleles.emplace_back("N");
      else split_getline(c, n, ',', [&](const char* a, size_t m) { alleles.emplace_back(a, m); });
    }
    ++index;
  });
}

void put_dbl(std::string& o, double v)
{
  if (std::isnan(v)) { o += "-nan"; return; }           // the reference's 0/0 is x86-64's default NaN, negative
  if (v == 0.0 && !std::signbit(v)) { o += '0'; return; }
  if (v == 1.0) { o += '1'; return; }
  char b[48];
  const int n = snprintf(b, sizeof b, "%g", v);         // ostream's default for a double
  o.append(b, (size_t)n);
}

void put_u64(std::string& o, uint64_t v)
{
  char b[24];
  int n = 0;
  do { b[23 - n++] = (char)('0' + v % 10); v /= 10; } while (v);
  o.append(b + 24 - n, (size_t)n);
}

} // namespace

void otg_vcf2mat_rows(std::string& o, const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len,
                      int32_t k, const double* usage, const double* gc, const double* hsd, uint32_t first_index)
{
  const uint64_t bins = (1ull << (2 * k)) + 1;
  for (uint32_t r = 0; r < n_records; ++r) {
    const otg_vcf_record& R = records[r];
    const uint64_t i0 = r == 0 ? first_index : 0u;
    for (uint32_t i = 0; i < R.n_alleles; ++i) {
      const uint64_t a = (uint64_t)R.first_allele + i;
      o.append(region_arena + R.region_off, R.region_len);
      o += '\t'; put_u64(o, i0 + i);
      o += '\t'; put_dbl(o, gc[a]);
      o += '\t'; put_u64(o, seq_len[a]);
      o += '\t'; put_dbl(o, hsd[a]);
      const double* row = usage + a * bins;
      for (uint64_t b = 0; b < bins; ++b) { o += '\t'; put_dbl(o, row[b]); }
      o += '\n';
    }
  }
}

extern "C" {

int otg_vcf_open(const char* path, otg_vcf** out)
{
  if (!path || !out) return otg_fail(nullptr, OTG_ERR_ARG, "otg_vcf_open: NULL argument");
  *out = nullptr;
  gzFile f = gzopen(path, "rb");
  if (!f) return otg_fail(nullptr, OTG_ERR_ARG, "otg_vcf_open: cannot open %s", path);
  otg_vcf* v = new otg_vcf();
  v->f = f;
  v->buf.resize(VCF_CHUNK);
  *out = v;
  return OTG_OK;
}

void otg_vcf_close(otg_vcf* v)
{
  if (!v) return;
  if (v->f) gzclose(v->f);
  delete v;
}

int otg_vcf_read_alleles(otg_vcf* v, otg_vcf_record* records, uint32_t records_capacity, uint32_t* n_records,
                         char* region_arena, uint64_t region_capacity, uint64_t* region_used,
                         uint64_t* seq_off, uint32_t* seq_len, uint32_t alleles_capacity, uint32_t* n_alleles,
                         uint8_t* seq_arena, uint64_t arena_capacity, uint64_t* arena_used, uint64_t* bytes_in)
{
  if (!v || !n_records || !region_used || !n_alleles || !arena_used) return otg_fail(nullptr, OTG_ERR_ARG, "otg_vcf_read_alleles: NULL argument");
  *n_records = 0; *region_used = 0; *n_alleles = 0; *arena_used = 0;
  std::string line;
  uint64_t consumed = 0;
  int rc = OTG_OK;
  for (;;) {
    if (!v->pending) {
      bool got = false;
      rc = next_line(v, line, &got, &consumed);
      if (rc != OTG_OK || !got) break;
      if (!line.empty() && line[0] == '#') continue;
      parse_alleles(line, v->region, v->alleles);
      if (v->alleles.empty()) continue;                 // empty line, fewer than 4 columns: nothing printed
      v->pending = true;
      v->pending_bytes = 0;
    }
    uint64_t need = 0;
    for (const auto& a : v->alleles) need += a.size();
    const uint32_t na = (uint32_t)v->alleles.size();
    const bool fits = *n_records < records_capacity && records && region_arena && seq_off && seq_len && seq_arena &&
                      *region_used + v->region.size() <= region_capacity && (uint64_t)*n_alleles + na <= alleles_capacity &&
                      *arena_used + need <= arena_capacity;
    if (!fits) {
      if (*n_records == 0) {                            // the record alone: report its needs, keep it for the next call
        *region_used = v->region.size(); *n_alleles = na; *arena_used = need;
        rc = otg_fail(nullptr, OTG_ERR_CAPACITY, "otg_vcf_read_alleles: a record needs %u alleles, %llu sequence bytes", na, (unsigned long long)need);
      }
      break;
    }
    otg_vcf_record& R = records[(*n_records)++];
    R.region_off = *region_used; R.region_len = (uint32_t)v->region.size(); R.first_allele = *n_alleles; R.n_alleles = na; R.reserved = 0;
    if (!v->region.empty()) memcpy(region_arena + *region_used, v->region.data(), v->region.size());
    *region_used += v->region.size();
    for (const auto& a : v->alleles) {
      seq_off[*n_alleles] = *arena_used; seq_len[*n_alleles] = (uint32_t)a.size();
      if (!a.empty()) memcpy(seq_arena + *arena_used, a.data(), a.size());
      *arena_used += a.size();
      ++*n_alleles;
    }
    v->pending = false;
  }
  if (bytes_in) *bytes_in += consumed;
  return rc;
}

int otg_vcf2mat_emit(const otg_vcf_record* records, uint32_t n_records, const char* region_arena, const uint32_t* seq_len, int32_t k,
                     const double* usage, const double* gc, const double* hsd, char* out, uint64_t out_capacity, uint64_t* out_len)
{
  if (!out_len) return otg_fail(nullptr, OTG_ERR_ARG, "otg_vcf2mat_emit: NULL out_len");
  if (k < 1 || k > OTG_KMER_MAX) return otg_fail(nullptr, OTG_ERR_ARG, "otg_vcf2mat_emit: k = %d outside 1..%d", k, OTG_KMER_MAX);
  if (n_records && (!records || !region_arena || !seq_len || !usage || !gc || !hsd)) return otg_fail(nullptr, OTG_ERR_ARG, "otg_vcf2mat_emit: NULL argument");
  std::string text;
  otg_vcf2mat_rows(text, records, n_records, region_arena, seq_len, k, usage, gc, hsd);
  return otg_text_out("otg_vcf2mat_emit", text, out, out_capacity, out_len);
}

} // extern "C"
