// K15 — per-line code of the split of a whole-genome VCF into per-chromosome texts
// (Util/bin/split_vcf_by_chr.py:29-52), shared by the kernels (avdb_splitvcf.hip) and the
// library's host entries (avdb_vcf_split_size_host / avdb_vcf_split_write_host): one
// definition, compiled for both sides, as avdb_expvcf.hpp is.
#pragma once

#include "avdb_lines.hpp"
#include "avdb_vcfline.hpp"

namespace avdb {
namespace splitvcf {

constexpr uint32_t kStreams = AVDB_SPLIT_N_STREAMS;
constexpr uint32_t kMaxLen = 0x7FFFFFFEu;  // a stored length (bit 31 of out_len is the LINE_HOST flag)

// what the size pass knows of one line
struct Line {
  uint32_t code;     // 0..25, or AVDB_SPLIT_NONE: a comment
  uint32_t out_len;  // the stored length + 1 (0: a comment), AVDB_SPLIT_LINE_HOST or-ed in
};

// the index of a key among the labels 1..22, X, Y, M (xstr of the HumanChromosome
// values), 0xFF when it is not exactly one of them
template <class CP>
AVDB_HD uint32_t label_code(CP p, uint32_t n) {
  if (n == 1) {
    const uint32_t c = p[0];
    if (c >= '1' && c <= '9') return c - '1';
    return c == 'X' ? 22u : c == 'Y' ? 23u : c == 'M' ? 24u : 0xFFu;
  }
  if (n == 2) {
    const uint32_t a = p[0], b = p[1];
    if (a == '1' && b >= '0' && b <= '9') return 9 + (b - '0');
    if (a == '2' && b >= '0' && b <= '2') return 19 + (b - '0');
  }
  return 0xFFu;
}

// a last byte after which Python's str.rstrip() may go on, or its decode may raise
AVDB_HD bool is_host_tail(uint32_t c) { return (c >= 0x1Cu && c <= 0x1Fu) || c >= 0x80u; }

// One line (its len bytes, '\n' excluded) by split_vcf_by_chr.py:37-50.  CP: a byte
// pointer in the text's address space (host, global or the LDS stage).
template <class CP>
AVDB_HD Line scan_line(CP line, uint64_t len64, const ChromMapView& cm) {
  uint32_t n = len64 < kMaxLen ? uint32_t(len64) : kMaxLen;  // (lengths are u32: a longer line is cut)
  while (n && is_ws(uint8_t(line[n - 1]))) --n;              // str.rstrip() of ASCII text
  const uint32_t host = n && is_host_tail(line[n - 1]) ? AVDB_SPLIT_LINE_HOST : 0u;
  if (n && line[0] == '#') return Line{AVDB_SPLIT_NONE, host};
  uint32_t k = 0;
  while (k < n && line[k] != '\t') ++k;  // values[0] of line.split('\t')
  bool unused;
  uint32_t c = cm.slot ? uint32_t(chrom_map_code(cm, line, k, &unused)) : label_code(line, k);
  if (c >= AVDB_SPLIT_OTHER) c = AVDB_SPLIT_OTHER;
  return Line{c, (n + 1) | host};
}

// a line's place in the write pass: its stream, or kStreams when it has no output
AVDB_HD uint32_t stream_of(uint32_t code, uint32_t out_len) {
  return code < kStreams && (out_len & ~AVDB_SPLIT_LINE_HOST) ? code : kStreams;
}

}  // namespace splitvcf
}  // namespace avdb
