// bam_sink.cpp — SAM text in, coordinate-sorted BAM + BAI out (otg_bam_sink_*), and the k-way merge of such BAMs (otg_bam_merge).
// Host code that needs only include/otter_gpu.h, zlib and threads: no HIP, nothing else of the library, so that a stand-alone program can
// link this file alone (tools/fuzz_bam_sink.cpp does, under the sanitizers).  Written from the SAM/BAM specification (records, BGZF
// framing, the binning index with its 16-kb linear index); the record rules follow what the reference's vendored converter makes of the
// same line (sam_parse1, src/sam.c:504-668).
#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <queue>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include <zlib.h>
#include "../../include/otter_gpu.h"

// otg_api.hip defines this hook (it stores the text otg_last_error(NULL) returns); a program that links this file alone has none
extern "C" __attribute__((weak)) void otg_set_global_error(const char* msg);

namespace {

constexpr size_t BGZF_INPUT = 0xff00;                 // input bytes per block
constexpr int64_t BAI_MAX_END = (int64_t)1 << 29;     // the binning scheme covers [0, 2^29)
const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
const char HD_LINE[] = "@HD\tVN:1.6\tSO:coordinate\n";

thread_local std::string g_io_err;
int io_fail(int code, const char* fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_io_err = buf;
  if (otg_set_global_error) otg_set_global_error(buf);
  return code;
}

void put32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
void set32(uint8_t* p, uint32_t x) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(x >> (8 * i)); }
uint32_t get32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// bin of [beg, end) in the 5-level scheme of the SAM specification (§5.3); beg may be -1 (the converter bins unmapped records too)
int reg2bin(int64_t beg, int64_t end)
{
  --end;
  if (beg >> 14 == end >> 14) return (int)(4681 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (int)(585 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (int)(73 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (int)(9 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (int)(1 + (beg >> 26));
  return 0;
}

// ---------------------------------------------------------------- BGZF out
// The uncompressed stream is cut every 0xff00 bytes and at flush_block(); every block is deflated on its own, so the file depends on
// neither the number of threads nor the pieces write() was called with.  Offsets are handed out in uncompressed bytes; voffset()
// translates them once the blocks in front of them have been written.
struct BgzfWriter {
  FILE* f = nullptr;
  int threads = 1, level = -1;
  std::vector<uint8_t> cur;
  std::vector<std::vector<uint8_t>> pending;
  uint64_t upos = 0, u_written = 0, fpos = 0;
  std::vector<uint64_t> blk_u, blk_f;             // uncompressed / file offset of every block written
  bool io_error = false;

  static void deflate_block(z_stream* zs, const std::vector<uint8_t>& in, std::vector<uint8_t>& out)
  {
    out.resize(18 + 65536);
    size_t clen = 0;
    bool ok = false;
    if (zs && deflateReset(zs) == Z_OK) {
      zs->next_in = const_cast<Bytef*>(in.data()); zs->avail_in = (uInt)in.size();
      zs->next_out = out.data() + 18; zs->avail_out = 65536 - 26;
      if (deflate(zs, Z_FINISH) == Z_STREAM_END) { ok = true; clen = 65536 - 26 - zs->avail_out; }
    }
    if (!ok) {                                    // does not shrink (or no deflate state): one stored block, len + 5 bytes
      uint8_t* p = out.data() + 18;
      p[0] = 1; p[1] = (uint8_t)in.size(); p[2] = (uint8_t)(in.size() >> 8); p[3] = (uint8_t)~p[1]; p[4] = (uint8_t)~p[2];
      if (!in.empty()) memcpy(p + 5, in.data(), in.size());
      clen = in.size() + 5;
    }
    const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(out.data(), head, 16);
    const size_t total = 18 + clen + 8;
    out[16] = (uint8_t)(total - 1); out[17] = (uint8_t)((total - 1) >> 8);
    set32(out.data() + 18 + clen, (uint32_t)crc32(crc32(0L, Z_NULL, 0), in.data(), (uInt)in.size()));
    set32(out.data() + 22 + clen, (uint32_t)in.size());
    out.resize(total);
  }

  void compress_pending()
  {
    const size_t n = pending.size();
    if (!n) return;
    std::vector<std::vector<uint8_t>> outs(n);
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)threads, n));
    auto work = [&](size_t t) {
      z_stream zs; memset(&zs, 0, sizeof zs);
      const bool have = deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK;
      for (size_t i = t; i < n; i += nt) deflate_block(have ? &zs : nullptr, pending[i], outs[i]);
      if (have) deflateEnd(&zs);
    };
    if (nt == 1) work(0);
    else {
      std::vector<std::thread> th;
      for (size_t t = 1; t < nt; ++t) th.emplace_back(work, t);
      work(0);
      for (auto& x : th) x.join();
    }
    for (size_t i = 0; i < n; ++i) {
      blk_u.push_back(u_written); blk_f.push_back(fpos);
      if (!io_error && fwrite(outs[i].data(), 1, outs[i].size(), f) != outs[i].size()) io_error = true;
      u_written += pending[i].size(); fpos += outs[i].size();
    }
    pending.clear();
  }

  void close_block()
  {
    pending.emplace_back(std::move(cur));
    cur.clear();
    if (pending.size() >= (size_t)std::max(1, threads) * 4) compress_pending();
  }

  void write(const uint8_t* p, size_t n)
  {
    upos += n;
    while (n) {
      if (cur.capacity() < BGZF_INPUT) cur.reserve(BGZF_INPUT);
      const size_t k = std::min(n, BGZF_INPUT - cur.size());
      cur.insert(cur.end(), p, p + k);
      p += k; n -= k;
      if (cur.size() == BGZF_INPUT) close_block();
    }
  }
  void flush_block() { if (!cur.empty()) close_block(); }

  bool finish()
  {
    flush_block();
    compress_pending();
    blk_u.push_back(u_written); blk_f.push_back(fpos);           // the EOF block: where an offset at the very end points
    if (!io_error && fwrite(EOF_BLOCK, 1, sizeof EOF_BLOCK, f) != sizeof EOF_BLOCK) io_error = true;
    if (fclose(f) != 0) io_error = true;
    f = nullptr;
    return !io_error;
  }

  // after finish(): virtual offset of uncompressed offset u; the end of a block is the start of the next one
  uint64_t voffset(uint64_t u) const
  {
    const size_t b = (size_t)(std::upper_bound(blk_u.begin(), blk_u.end(), u) - blk_u.begin()) - 1;
    return blk_f[b] << 16 | (u - blk_u[b]);
  }
};

// ---------------------------------------------------------------- BAI
struct IndexBuilder {
  struct Target {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;     // chunks in uncompressed offsets until save()
    std::vector<uint64_t> linear;                                             // UINT64_MAX: no record overlaps the window yet
  };
  std::vector<Target> t;
  void push(int32_t tid, int64_t pos, int64_t end, uint64_t ub, uint64_t ue)
  {
    if (tid < 0 || (size_t)tid >= t.size() || pos < 0) return;
    Target& T = t[(size_t)tid];
    auto& ch = T.bins[(uint32_t)reg2bin(pos, end)];
    if (!ch.empty() && ch.back().second == ub) ch.back().second = ue; else ch.emplace_back(ub, ue);
    const size_t w1 = (size_t)((end - 1) >> 14);
    if (T.linear.size() <= w1) T.linear.resize(w1 + 1, UINT64_MAX);
    for (size_t w = (size_t)(pos >> 14); w <= w1; ++w) if (T.linear[w] == UINT64_MAX) T.linear[w] = ub;
  }
  bool save(const std::string& path, const BgzfWriter& w) const
  {
    std::vector<uint8_t> o = {'B', 'A', 'I', 1};
    auto put64 = [&](uint64_t x) { put32(o, (uint32_t)x); put32(o, (uint32_t)(x >> 32)); };
    put32(o, (uint32_t)t.size());
    for (const Target& T : t) {
      put32(o, (uint32_t)T.bins.size());
      for (const auto& kv : T.bins) {
        put32(o, kv.first); put32(o, (uint32_t)kv.second.size());
        for (const auto& c : kv.second) { put64(w.voffset(c.first)); put64(w.voffset(c.second)); }
      }
      put32(o, (uint32_t)T.linear.size());
      uint64_t last = 0;                           // a window without a record takes the previous offset
      for (uint64_t u : T.linear) { if (u != UINT64_MAX) last = w.voffset(u); put64(last); }
    }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    return (fclose(f) == 0) && ok;
  }
};

void bam_header_bytes(const std::string& text, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, std::vector<uint8_t>& o)
{
  o = {'B', 'A', 'M', 1};
  put32(o, (uint32_t)text.size());
  o.insert(o.end(), text.begin(), text.end());
  put32(o, (uint32_t)names.size());
  for (size_t i = 0; i < names.size(); ++i) {
    put32(o, (uint32_t)names[i].size() + 1);
    o.insert(o.end(), names[i].begin(), names[i].end());
    o.push_back(0);
    put32(o, lens[i]);
  }
}

// the value of field `key` ("SN:", "ID:", ...) of a tab-separated header line; false when absent
bool header_field(const std::string& line, const char* key, std::string& out)
{
  size_t a = line.find('\t');
  while (a != std::string::npos) {
    const size_t b = line.find('\t', a + 1);
    if (line.compare(a + 1, 3, key) == 0) { out = line.substr(a + 4, b == std::string::npos ? b : b - a - 4); return true; }
    a = b;
  }
  return false;
}

bool whole_long(const char* s, size_t n, int base, long* v)
{
  if (n == 0) return false;
  char* e = nullptr;
  errno = 0;
  *v = strtol(s, &e, base);
  return errno == 0 && e == s + n;
}

uint64_t sort_key(int32_t tid, int32_t pos) { return (uint64_t)(uint32_t)tid << 32 | (uint32_t)(pos + 1); }   // tid -1 (unmapped) sorts last

}  // namespace

// ---------------------------------------------------------------- the sink
struct otg_bam_sink {
  std::string path, err;
  int sort = 0, code = OTG_OK;             // code: what the refusal or the failed write returned

  bool failed = false, started = false;
  BgzfWriter w;
  IndexBuilder idx;
  std::string carry;                       // an unfinished line
  std::vector<char> line;                  // the line being parsed: mutable, NUL-terminated
  uint64_t lineno = 0, n_records = 0;
  std::string header;                      // the input's header lines, @HD dropped
  std::vector<std::string> tnames;
  std::vector<uint32_t> tlens;
  std::unordered_map<std::string, int32_t> name2tid;
  uint8_t nt16[256];
  int8_t cigar_op[256];
  uint64_t last_key = 0, last_line = 0;
  int32_t last_tid = 0, last_pos = 0;
  std::vector<uint8_t> rec;                // the record being built
  struct Ref { uint64_t key, off; uint32_t len; int32_t end; };
  std::vector<uint8_t> held;               // sort = 1: every record's bytes ...
  std::vector<Ref> refs;                   // ... and where they are
};

namespace {

int sink_fail(otg_bam_sink* s, int code, const char* fmt, ...)
{
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  s->err = buf;
  s->failed = true;
  s->code = code;
  return io_fail(code, "otg_bam_sink %s: %s", s->path.c_str(), buf);
}
#define REFUSE(...) return sink_fail(s, OTG_ERR_ARG, __VA_ARGS__)

int header_line(otg_bam_sink* s, const char* p, size_t n)
{
  const unsigned long long ln = (unsigned long long)s->lineno;
  if (s->started || !s->refs.empty()) REFUSE("line %llu: a header line after the first record", ln);
  const std::string l(p, n);
  if (l.compare(0, 3, "@HD") == 0 && (n == 3 || l[3] == '\t')) return OTG_OK;          // replaced by ours
  if (l.compare(0, 4, "@SQ\t") == 0) {
    std::string sn, lnv;
    long v = 0;
    if (!header_field(l, "SN:", sn) || sn.empty() || !header_field(l, "LN:", lnv) || !whole_long(lnv.c_str(), lnv.size(), 10, &v) || v < 0 || v > INT32_MAX)
      REFUSE("line %llu: an @SQ line without a usable SN: / LN:", ln);
    if (!s->name2tid.emplace(sn, (int32_t)s->tnames.size()).second) REFUSE("line %llu: @SQ SN:%s is given twice", ln, sn.c_str());
    s->tnames.push_back(sn); s->tlens.push_back((uint32_t)v);
  }
  s->header += l;
  s->header += '\n';
  return OTG_OK;
}

void start_output(otg_bam_sink* s)
{
  std::vector<uint8_t> h;
  bam_header_bytes(HD_LINE + s->header, s->tnames, s->tlens, h);
  s->w.write(h.data(), h.size());
  s->w.flush_block();                      // records start on a block boundary
  s->idx.t.resize(s->tnames.size());
  s->started = true;
}

int emit_record(otg_bam_sink* s, const uint8_t* rec, size_t len, int32_t tid, int32_t pos, int32_t end)
{
  if (!s->started) start_output(s);
  const uint64_t ub = s->w.upos;
  s->w.write(rec, len);
  s->idx.push(tid, pos, end, ub, s->w.upos);
  ++s->n_records;
  return s->w.io_error ? sink_fail(s, OTG_ERR_FATAL, "cannot write %s", s->path.c_str()) : OTG_OK;
}

// one alignment line (p[n] == 0, writable): the BAM record the converter makes of it
int record_line(otg_bam_sink* s, char* p, size_t n)
{
  const unsigned long long ln = (unsigned long long)s->lineno;
  std::vector<std::pair<char*, size_t>> f;
  f.reserve(20);
  for (char* a = p;;) {
    char* b = (char*)memchr(a, '\t', (size_t)(p + n - a));
    if (!b) { f.emplace_back(a, (size_t)(p + n - a)); break; }
    *b = 0;
    f.emplace_back(a, (size_t)(b - a));
    a = b + 1;
  }
  if (f.size() < 11) REFUSE("line %llu: %zu fields, a record has at least 11", ln, f.size());
  for (const auto& x : f) if (memchr(x.first, 0, x.second)) REFUSE("line %llu: a NUL byte", ln);
  long v = 0;
  if (f[0].second == 0 || f[0].second > 254) REFUSE("line %llu: QNAME of %zu bytes", ln, f[0].second);
  if (!whole_long(f[1].first, f[1].second, 0, &v) || v < 0 || v > 65535) REFUSE("line %llu: FLAG '%.32s'", ln, f[1].first);
  uint32_t flag = (uint32_t)v;
  int32_t tid = -1;
  if (strcmp(f[2].first, "*") != 0) {
    auto it = s->name2tid.find(std::string(f[2].first, f[2].second));
    if (it == s->name2tid.end()) REFUSE("line %llu: RNAME '%.64s' is not in the @SQ lines", ln, f[2].first);
    tid = it->second;
  }
  if (!whole_long(f[3].first, f[3].second, 10, &v) || v < 0 || v > BAI_MAX_END) REFUSE("line %llu: POS '%.32s'", ln, f[3].first);
  const int32_t pos = (int32_t)v - 1;
  if (pos < 0 && tid >= 0) tid = -1;       // "mapped query cannot have zero coordinate; treated as unmapped"
  if (tid < 0) flag |= 4;
  if (!whole_long(f[4].first, f[4].second, 10, &v) || v < 0 || v > 255) REFUSE("line %llu: MAPQ '%.32s'", ln, f[4].first);
  const uint32_t mapq = (uint32_t)v;

  std::vector<uint8_t>& r = s->rec;
  r.assign(36, 0);
  r.insert(r.end(), f[0].first, f[0].first + f[0].second + 1);           // with its NUL
  uint32_t n_cigar = 0;
  int64_t rlen = 0, qlen = 0;
  if (strcmp(f[5].first, "*") == 0) { flag |= 4; rlen = 1; }             // "mapped query must have a CIGAR; treated as unmapped"
  else {
    if (f[5].second == 0) REFUSE("line %llu: empty CIGAR", ln);
    for (const char* c = f[5].first; *c;) {
      uint64_t len = 0;
      int digits = 0;
      while (*c >= '0' && *c <= '9') { len = len * 10 + (uint64_t)(*c - '0'); if (++digits > 9) break; ++c; }
      const int op = s->cigar_op[(uint8_t)*c];
      if (digits == 0 || digits > 9 || op < 0 || len >= (1u << 28)) REFUSE("line %llu: CIGAR '%.32s'", ln, f[5].first);
      ++c;
      if (++n_cigar > 65535) REFUSE("line %llu: more than 65535 CIGAR operations", ln);
      put32(r, (uint32_t)len << 4 | (uint32_t)op);
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += (int64_t)len;
      if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += (int64_t)len;
      if (rlen > BAI_MAX_END || qlen > INT32_MAX) REFUSE("line %llu: the CIGAR spans more than a BAI index can hold", ln);
    }
  }
  const uint32_t bin = (uint32_t)reg2bin(pos, (int64_t)pos + rlen) & 0xffffu;
  const int64_t end = (int64_t)pos + (rlen > 0 ? rlen : 1);
  if (tid >= 0 && end > BAI_MAX_END) REFUSE("line %llu: the record ends at %lld, past 2^29 (a BAI index cannot hold it)", ln, (long long)end);
  int32_t mtid = -1;
  if (strcmp(f[6].first, "=") == 0) mtid = tid;
  else if (strcmp(f[6].first, "*") != 0) { auto it = s->name2tid.find(std::string(f[6].first, f[6].second)); mtid = it == s->name2tid.end() ? -1 : it->second; }
  if (!whole_long(f[7].first, f[7].second, 10, &v) || v < 0 || v > INT32_MAX) REFUSE("line %llu: PNEXT '%.32s'", ln, f[7].first);
  const int32_t mpos = (int32_t)v - 1;
  if (mpos < 0 && mtid >= 0) mtid = -1;
  if (!whole_long(f[8].first, f[8].second, 10, &v) || v < INT32_MIN || v > INT32_MAX) REFUSE("line %llu: TLEN '%.32s'", ln, f[8].first);
  const int32_t tlen = (int32_t)v;
  uint32_t l_seq = 0;
  if (strcmp(f[9].first, "*") != 0) {
    if (f[9].second > (size_t)INT32_MAX) REFUSE("line %llu: SEQ too long", ln);
    l_seq = (uint32_t)f[9].second;
    if (n_cigar && qlen != (int64_t)l_seq) REFUSE("line %llu: the CIGAR covers %lld bases, SEQ has %u", ln, (long long)qlen, l_seq);
    const uint8_t* q = (const uint8_t*)f[9].first;
    const size_t at = r.size();
    r.resize(at + (l_seq + 1) / 2, 0);
    uint8_t* o = r.data() + at;
    for (uint32_t i = 0; i + 1 < l_seq; i += 2) o[i >> 1] = (uint8_t)(s->nt16[q[i]] << 4 | s->nt16[q[i + 1]]);
    if (l_seq & 1) o[l_seq >> 1] = (uint8_t)(s->nt16[q[l_seq - 1]] << 4);
  }
  if (strcmp(f[10].first, "*") != 0) {
    if (f[10].second != l_seq) REFUSE("line %llu: SEQ has %u bases, QUAL %zu", ln, l_seq, f[10].second);
    const size_t at = r.size();
    r.resize(at + l_seq);
    for (uint32_t i = 0; i < l_seq; ++i) r[at + i] = (uint8_t)(f[10].first[i] - 33);
  } else r.insert(r.end(), l_seq, 0xff);
  for (size_t k = 11; k < f.size(); ++k) {
    char* q = f[k].first;
    const size_t m = f[k].second;
    if (m < 6 || q[2] != ':' || q[4] != ':') REFUSE("line %llu: tag '%.32s' is not XX:T:value", ln, q);
    const char type = q[3];
    const char* val = q + 5;
    r.push_back((uint8_t)q[0]); r.push_back((uint8_t)q[1]);
    if (type == 'A') {
      if (m != 6) REFUSE("line %llu: tag '%.32s': an A value is one character", ln, q);
      r.push_back('A'); r.push_back((uint8_t)val[0]);
    } else if (type == 'i') {
      if (!whole_long(val, m - 5, 10, &v) || v < INT32_MIN || v > (long)UINT32_MAX) REFUSE("line %llu: tag '%.40s' is not a 32-bit integer", ln, q);
      // the smallest of c C s S i I that holds the value
      if (v < 0) {
        if (v >= INT8_MIN) { r.push_back('c'); r.push_back((uint8_t)v); }
        else if (v >= INT16_MIN) { r.push_back('s'); r.push_back((uint8_t)v); r.push_back((uint8_t)(v >> 8)); }
        else { r.push_back('i'); put32(r, (uint32_t)v); }
      } else {
        if (v <= UINT8_MAX) { r.push_back('C'); r.push_back((uint8_t)v); }
        else if (v <= UINT16_MAX) { r.push_back('S'); r.push_back((uint8_t)v); r.push_back((uint8_t)(v >> 8)); }
        else { r.push_back('I'); put32(r, (uint32_t)v); }
      }
    } else if (type == 'f') {
      char* e = nullptr;
      const float x = (float)strtod(val, &e);              // through double, as the converter does
      if (e != val + (m - 5)) REFUSE("line %llu: tag '%.40s' is not a number", ln, q);
      uint32_t bits;
      memcpy(&bits, &x, 4);
      r.push_back('f'); put32(r, bits);
    } else if (type == 'Z') {
      r.push_back('Z');
      r.insert(r.end(), val, val + (m - 5) + 1);
    } else REFUSE("line %llu: tag '%.2s' has type '%c'; A, i, f and Z are written", ln, q, type);
  }
  if (r.size() - 4 > (size_t)INT32_MAX) REFUSE("line %llu: the record is too long", ln);
  set32(&r[0], (uint32_t)(r.size() - 4));
  set32(&r[4], (uint32_t)tid); set32(&r[8], (uint32_t)pos);
  set32(&r[12], bin << 16 | mapq << 8 | (uint32_t)(f[0].second + 1));
  set32(&r[16], flag << 16 | n_cigar);
  set32(&r[20], l_seq); set32(&r[24], (uint32_t)mtid); set32(&r[28], (uint32_t)mpos); set32(&r[32], (uint32_t)tlen);

  const uint64_t key = sort_key(tid, pos);
  if (s->sort) {
    s->refs.push_back({key, (uint64_t)s->held.size(), (uint32_t)r.size(), (int32_t)end});
    s->held.insert(s->held.end(), r.begin(), r.end());
    return OTG_OK;
  }
  if (s->n_records && key < s->last_key)
    REFUSE("line %llu: out of order: target %d position %d comes after target %d position %d of line %llu (sort = 0 takes coordinate-sorted text)", ln, tid,
           pos + 1, s->last_tid, s->last_pos + 1, (unsigned long long)s->last_line);
  s->last_key = key; s->last_tid = tid; s->last_pos = pos; s->last_line = s->lineno;
  return emit_record(s, r.data(), r.size(), tid, pos, (int32_t)end);
}

int one_line(otg_bam_sink* s, const char* p, size_t n)
{
  ++s->lineno;
  if (n == 0) REFUSE("line %llu: an empty line", (unsigned long long)s->lineno);
  if (p[0] == '@') return header_line(s, p, n);
  s->line.assign(p, p + n);
  s->line.push_back(0);
  return record_line(s, s->line.data(), n);
}

void sink_remove(otg_bam_sink* s)
{
  if (s->w.f) { fclose(s->w.f); s->w.f = nullptr; }
  remove(s->path.c_str());
  remove((s->path + ".bai").c_str());
}

}  // namespace

extern "C" {

int otg_bam_sink_open(const char* bam_path, const otg_bam_sink_opts* opts, otg_bam_sink** out)
{
  if (!bam_path || !bam_path[0] || !out) return io_fail(OTG_ERR_ARG, "otg_bam_sink_open: NULL path or handle");
  *out = nullptr;
  const int threads = opts ? opts->threads : 1, level = opts ? opts->level : -1;
  if (level < -1 || level > 9) return io_fail(OTG_ERR_ARG, "otg_bam_sink_open: level %d is not -1 .. 9", level);
  FILE* f = fopen(bam_path, "wb");
  if (!f) return io_fail(OTG_ERR_ARG, "otg_bam_sink_open: cannot write %s: %s", bam_path, strerror(errno));
  otg_bam_sink* s = new otg_bam_sink();
  s->path = bam_path;
  s->sort = opts && opts->sort ? 1 : 0;
  s->w.f = f; s->w.threads = std::max(1, std::min(threads, 256)); s->w.level = level;
  memset(s->nt16, 15, sizeof s->nt16);
  const char* iupac = "=ACMGRSVTWYHKDBN";                               // SAM specification §4.2.3; digits 0-3 read as A C G T
  for (int i = 0; i < 16; ++i) { s->nt16[(uint8_t)iupac[i]] = (uint8_t)i; s->nt16[(uint8_t)tolower(iupac[i])] = (uint8_t)i; }
  for (int i = 0; i < 4; ++i) s->nt16['0' + i] = (uint8_t)(1 << i);
  memset(s->cigar_op, -1, sizeof s->cigar_op);
  const char* ops = "MIDNSHP=X";
  for (int i = 0; i < 9; ++i) s->cigar_op[(uint8_t)ops[i]] = (int8_t)i;
  *out = s;
  return OTG_OK;
}

int otg_bam_sink_write(void* sink, const char* data, uint64_t len)
{
  otg_bam_sink* s = (otg_bam_sink*)sink;
  if (!s) return io_fail(OTG_ERR_ARG, "otg_bam_sink_write: NULL sink");
  if (s->failed) return s->code;
  if (len && !data) return sink_fail(s, OTG_ERR_ARG, "NULL data");
  const char* p = data;
  const char* const e = data + len;
  while (p < e) {
    const char* nl = (const char*)memchr(p, '\n', (size_t)(e - p));
    if (!nl) { s->carry.append(p, (size_t)(e - p)); break; }
    int rc;
    if (s->carry.empty()) rc = one_line(s, p, (size_t)(nl - p));
    else {
      s->carry.append(p, (size_t)(nl - p));
      rc = one_line(s, s->carry.data(), s->carry.size());
      s->carry.clear();
    }
    if (rc != OTG_OK) return rc;
    p = nl + 1;
  }
  return OTG_OK;
}

void otg_bam_sink_abort(otg_bam_sink* s)
{
  if (!s) return;
  sink_remove(s);
  delete s;
}

int otg_bam_sink_close(otg_bam_sink* s, uint64_t* n_records)
{
  if (!s) return io_fail(OTG_ERR_ARG, "otg_bam_sink_close: NULL sink");
  if (n_records) *n_records = 0;
  int rc = OTG_OK;
  if (!s->failed && !s->carry.empty()) {                    // a last line without its newline
    const std::string last = std::move(s->carry);
    s->carry.clear();
    rc = one_line(s, last.data(), last.size());
  }
  if (!s->failed && s->sort) {
    std::stable_sort(s->refs.begin(), s->refs.end(), [](const otg_bam_sink::Ref& a, const otg_bam_sink::Ref& b) { return a.key < b.key; });
    for (const auto& r : s->refs) {
      const uint8_t* p = s->held.data() + r.off;
      if ((rc = emit_record(s, p, r.len, (int32_t)get32(p + 4), (int32_t)get32(p + 8), r.end)) != OTG_OK) break;
    }
  }
  if (!s->failed) {
    if (!s->started) start_output(s);
    if (!s->w.finish()) rc = sink_fail(s, OTG_ERR_FATAL, "cannot write %s", s->path.c_str());
    else if (!s->idx.save(s->path + ".bai", s->w)) rc = sink_fail(s, OTG_ERR_FATAL, "cannot write %s.bai", s->path.c_str());
  }
  if (s->failed) {
    rc = s->code;
    io_fail(rc, "otg_bam_sink %s: %s", s->path.c_str(), s->err.c_str());
    sink_remove(s);
  } else if (n_records) *n_records = s->n_records;
  delete s;
  return rc;
}

const char* otg_bam_sink_error(const otg_bam_sink* s) { return s ? s->err.c_str() : g_io_err.c_str(); }

}  // extern "C"

// ---------------------------------------------------------------- merge
namespace {

struct BgzfReader {
  FILE* f = nullptr;
  std::vector<uint8_t> blk, raw;
  size_t off = 0;
  bool bad = false, eof_block = false;     // eof_block: the last block read was an empty one
  z_stream zs;
  bool have_zs = false;
  ~BgzfReader() { if (f) fclose(f); if (have_zs) inflateEnd(&zs); }
  bool open(const char* path)
  {
    f = fopen(path, "rb");
    if (!f) return false;
    memset(&zs, 0, sizeof zs);
    have_zs = inflateInit2(&zs, -15) == Z_OK;
    return have_zs;
  }
  // the next non-empty block; false at the end of the file or on damage (bad)
  bool fill()
  {
    for (;;) {
      uint8_t h[12];
      const size_t got = fread(h, 1, 12, f);
      if (got == 0) { if (!eof_block) bad = true; return false; }     // the file must end with the empty EOF block: a cut at a block boundary
      if (got != 12 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) { bad = true; return false; }
      const size_t xlen = (size_t)h[10] | (size_t)h[11] << 8;
      raw.resize(xlen);
      if (xlen && fread(raw.data(), 1, xlen, f) != xlen) { bad = true; return false; }
      size_t bsize = 0;
      for (size_t p = 0; p + 4 <= xlen;) {
        const size_t sl = (size_t)raw[p + 2] | (size_t)raw[p + 3] << 8;
        if (raw[p] == 'B' && raw[p + 1] == 'C' && sl == 2 && p + 6 <= xlen) bsize = ((size_t)raw[p + 4] | (size_t)raw[p + 5] << 8) + 1;
        p += 4 + sl;
      }
      if (bsize < 12 + xlen + 8) { bad = true; return false; }
      const size_t clen = bsize - 12 - xlen - 8;
      raw.resize(clen + 8);
      if (fread(raw.data(), 1, clen + 8, f) != clen + 8) { bad = true; return false; }
      blk.resize(65536);
      if (inflateReset(&zs) != Z_OK) { bad = true; return false; }
      zs.next_in = raw.data(); zs.avail_in = (uInt)clen;
      zs.next_out = blk.data(); zs.avail_out = 65536;
      if (inflate(&zs, Z_FINISH) != Z_STREAM_END) { bad = true; return false; }
      const size_t n = 65536 - zs.avail_out;
      if (n != get32(raw.data() + clen + 4) || (uint32_t)crc32(crc32(0L, Z_NULL, 0), blk.data(), (uInt)n) != get32(raw.data() + clen)) { bad = true; return false; }
      blk.resize(n);
      off = 0;
      eof_block = n == 0;
      if (n) return true;
    }
  }
  size_t read(uint8_t* dst, size_t n)
  {
    size_t done = 0;
    while (done < n) {
      if (off == blk.size() && !fill()) break;
      const size_t k = std::min(n - done, blk.size() - off);
      memcpy(dst + done, blk.data() + off, k);
      off += k; done += k;
    }
    return done;
  }
  // n bytes into v, which grows only as the data arrives (a damaged length field must not allocate what it claims)
  bool read_vec(std::vector<uint8_t>& v, size_t at, size_t n)
  {
    while (n) {
      const size_t k = std::min<size_t>(n, 1u << 20);
      v.resize(at + k);
      if (read(v.data() + at, k) != k) return false;
      at += k; n -= k;
    }
    return true;
  }
};

struct MergeInput {
  std::string path;
  BgzfReader r;
  std::vector<std::string> lines;          // header lines
  std::vector<std::string> tnames;
  std::vector<uint32_t> tlens;
  std::vector<uint8_t> rec;                // the current record (with its length field)
  bool have = false;
  uint64_t key = 0;
  int32_t tid = 0, pos = 0, end = 0;
  uint64_t n_read = 0;
};

int read_bam_header(MergeInput& in)
{
  std::vector<uint8_t> b;
  if (!in.r.read_vec(b, 0, 8) || memcmp(b.data(), "BAM\1", 4) != 0) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s is not a BAM file", in.path.c_str());
  const uint32_t l_text = get32(b.data() + 4);
  if (l_text > (1u << 28) || !in.r.read_vec(b, 0, (size_t)l_text + 4)) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: truncated header", in.path.c_str());
  const uint32_t n_ref = get32(b.data() + l_text);
  std::string text((const char*)b.data(), l_text);
  text = text.substr(0, text.find('\0'));
  for (size_t a = 0; a < text.size();) {
    size_t e = text.find('\n', a);
    if (e == std::string::npos) e = text.size();
    if (e > a) in.lines.push_back(text.substr(a, e - a));
    a = e + 1;
  }
  if (n_ref > (1u << 24)) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: %u targets", in.path.c_str(), n_ref);
  for (uint32_t i = 0; i < n_ref; ++i) {
    if (!in.r.read_vec(b, 0, 4)) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: truncated target list", in.path.c_str());
    const uint32_t l_name = get32(b.data());
    if (l_name == 0 || l_name > (1u << 16) || !in.r.read_vec(b, 0, (size_t)l_name + 4)) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: truncated target list", in.path.c_str());
    in.tnames.emplace_back((const char*)b.data(), strnlen((const char*)b.data(), l_name));
    in.tlens.push_back(get32(b.data() + l_name));
  }
  return OTG_OK;
}

// the next record of `in` (have = false at the end); refuses damaged and unsorted input
int next_record(MergeInput& in)
{
  in.have = false;
  uint8_t lb[4] = {0, 0, 0, 0};
  const size_t got = in.r.read(lb, 4);
  if (got == 0 && !in.r.bad) return OTG_OK;
  const uint32_t bl = get32(lb);
  if (got == 0) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s is damaged or truncated after record %llu (a BGZF block does not inflate, or the EOF block is missing)", in.path.c_str(), (unsigned long long)in.n_read);
  if (got != 4 || bl < 32 || bl > (1u << 30)) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: damaged record %llu", in.path.c_str(), (unsigned long long)in.n_read);
  in.rec.resize(4);
  memcpy(in.rec.data(), lb, 4);
  if (!in.r.read_vec(in.rec, 4, bl)) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: truncated record %llu", in.path.c_str(), (unsigned long long)in.n_read);
  const uint8_t* p = in.rec.data() + 4;
  const int32_t tid = (int32_t)get32(p), pos = (int32_t)get32(p + 4);
  const uint32_t l_qname = p[8], n_cigar = get32(p + 12) & 0xffffu;
  if (tid < -1 || tid >= (int32_t)in.tnames.size() || pos < -1 || (int64_t)pos >= BAI_MAX_END || 32 + (uint64_t)l_qname + 4ull * n_cigar > bl)
    return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: damaged record %llu", in.path.c_str(), (unsigned long long)in.n_read);
  int64_t rlen = 0;
  for (uint32_t i = 0; i < n_cigar; ++i) {
    const uint32_t c = get32(p + 32 + l_qname + 4 * i), op = c & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4;
  }
  const int64_t end = (int64_t)pos + (rlen > 0 ? rlen : 1);
  if (tid >= 0 && pos >= 0 && end > BAI_MAX_END) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: record %llu ends past 2^29", in.path.c_str(), (unsigned long long)in.n_read);
  const uint64_t key = sort_key(tid, pos);
  if (in.n_read && key < in.key)
    return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s is not coordinate-sorted (record %llu: target %d position %d after target %d position %d)", in.path.c_str(),
                   (unsigned long long)in.n_read, tid, pos + 1, in.tid, in.pos + 1);
  in.key = key; in.tid = tid; in.pos = pos; in.end = (int32_t)std::min<int64_t>(end, BAI_MAX_END);
  in.have = true;
  ++in.n_read;
  return OTG_OK;
}

}  // namespace

// the merge proper; the caller has checked the arguments and removes the output when this fails
static int merge_into(const char* const* bam_paths, uint32_t n, const char* out_path, int32_t threads, int32_t level, uint64_t* n_records)
{
  std::vector<MergeInput> in(n);
  for (uint32_t i = 0; i < n; ++i) {
    in[i].path = bam_paths[i];
    if (!in[i].r.open(bam_paths[i])) return io_fail(OTG_ERR_ARG, "otg_bam_merge: cannot read %s: %s", bam_paths[i], strerror(errno));
    const int rc = read_bam_header(in[i]);
    if (rc != OTG_OK) return rc;
    if (in[i].tnames != in[0].tnames || in[i].tlens != in[0].tlens)
      return io_fail(OTG_ERR_ARG, "otg_bam_merge: the @SQ list of %s differs from that of %s", bam_paths[i], bam_paths[0]);
  }
  // the header: ours, the first input's @SQ lines, then every other line in input order (verbatim repeats once)
  std::string text = HD_LINE;
  for (const std::string& l : in[0].lines) if (l.compare(0, 4, "@SQ\t") == 0) { text += l; text += '\n'; }
  std::unordered_set<std::string> seen;
  std::unordered_map<std::string, uint32_t> rg_ids;
  std::string otter_of;
  bool have_of = false;
  for (uint32_t i = 0; i < n; ++i)
    for (const std::string& l : in[i].lines) {
      if (l.compare(0, 3, "@HD") == 0 || l.compare(0, 4, "@SQ\t") == 0) continue;
      std::string id;
      if (l.compare(0, 4, "@RG\t") == 0 && header_field(l, "ID:", id)) {
        auto it = rg_ids.emplace(id, i);
        if (!it.second) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: read group ID:%s is already in %s (a sample given twice?)", in[i].path.c_str(), id.c_str(), in[it.first->second].path.c_str());
      }
      if (l.compare(0, 4, "@PG\t") == 0 && header_field(l, "ID:", id) && id == "otter") {
        std::string of;
        header_field(l, "OF:", of);
        if (have_of && of != otter_of) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s: @PG ID:otter has OF:%s, an earlier input OF:%s", in[i].path.c_str(), of.c_str(), otter_of.c_str());
        otter_of = of; have_of = true;
      }
      if (seen.insert(l).second) { text += l; text += '\n'; }
    }
  // inputs that have a record, smallest (target, position) on top; ties: the earlier input
  typedef std::pair<uint64_t, uint32_t> Head;
  std::priority_queue<Head, std::vector<Head>, std::greater<Head>> heap;
  for (uint32_t i = 0; i < n; ++i) {
    const int rc = next_record(in[i]);
    if (rc != OTG_OK) return rc;
    if (in[i].have) heap.emplace(in[i].key, i);
  }

  BgzfWriter w;
  w.f = fopen(out_path, "wb");
  if (!w.f) return io_fail(OTG_ERR_ARG, "otg_bam_merge: cannot write %s: %s", out_path, strerror(errno));
  w.threads = std::max(1, std::min((int)threads, 256)); w.level = level;
  IndexBuilder idx;
  idx.t.resize(in[0].tnames.size());
  std::vector<uint8_t> h;
  bam_header_bytes(text, in[0].tnames, in[0].tlens, h);
  w.write(h.data(), h.size());
  w.flush_block();
  uint64_t count = 0;
  int rc = OTG_OK;
  while (!heap.empty()) {
    MergeInput& m = in[heap.top().second];
    const uint32_t which = heap.top().second;
    heap.pop();
    const uint64_t ub = w.upos;
    w.write(m.rec.data(), m.rec.size());
    idx.push(m.tid, m.pos, m.end, ub, w.upos);
    ++count;
    if (w.io_error) { rc = io_fail(OTG_ERR_FATAL, "otg_bam_merge: cannot write %s", out_path); break; }
    if ((rc = next_record(m)) != OTG_OK) break;
    if (m.have) heap.emplace(m.key, which);
  }
  if (rc == OTG_OK && !w.finish()) rc = io_fail(OTG_ERR_FATAL, "otg_bam_merge: cannot write %s", out_path);
  if (rc == OTG_OK && !idx.save(std::string(out_path) + ".bai", w)) rc = io_fail(OTG_ERR_FATAL, "otg_bam_merge: cannot write %s.bai", out_path);
  if (rc != OTG_OK) {
    if (w.f) { fclose(w.f); w.f = nullptr; }
    return rc;
  }
  if (n_records) *n_records = count;
  return OTG_OK;
}

extern "C" int otg_bam_merge(const char* const* bam_paths, uint32_t n, const char* out_path, int32_t threads, int32_t level, uint64_t* n_records)
{
  if (n_records) *n_records = 0;
  if (!bam_paths || n == 0 || !out_path || !out_path[0]) return io_fail(OTG_ERR_ARG, "otg_bam_merge: no inputs or no output path");
  if (level < -1 || level > 9) return io_fail(OTG_ERR_ARG, "otg_bam_merge: level %d is not -1 .. 9", level);
  for (uint32_t i = 0; i < n; ++i) {
    if (!bam_paths[i]) return io_fail(OTG_ERR_ARG, "otg_bam_merge: input %u is NULL", i);
    if (strcmp(bam_paths[i], out_path) == 0) return io_fail(OTG_ERR_ARG, "otg_bam_merge: %s is both an input and the output", out_path);
  }
  const int rc = merge_into(bam_paths, n, out_path, threads, level, n_records);
  if (rc != OTG_OK) {                       // a refused merge leaves no output behind, not even one from an earlier run
    remove(out_path);
    remove((std::string(out_path) + ".bai").c_str());
  }
  return rc;
}
