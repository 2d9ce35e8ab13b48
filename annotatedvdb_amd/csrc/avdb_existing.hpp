// K12 — per-line and per-row code of the --skipExisting key-set build from an
// export of AnnotatedVDB.Variant, shared by the kernels (avdb_existing.hip) and the
// library's host entries (avdb_existing_size_host / avdb_existing_write_host): one
// definition, compiled for both sides, as avdb_cadd.hpp is (line spans: avdb_lines.hpp).
#pragma once

#include "avdb_lines.hpp"

namespace avdb {
namespace exist {

constexpr uint32_t kContigs = 25;   // chromosomes.CHROM_NAMES: 1..22, X, Y, M
constexpr uint32_t kOtherBit = 31;  // the mask bit of every other label

// the .mapping fragment of a row: {'primary_key': '<pk>', 'bin_index': '<bin>'}
// (repr of the one-entry dict ExistingVariants.from_tsv stores, existing.py)
constexpr uint32_t kFragHead = 17;   // {'primary_key': '
constexpr uint32_t kFragMid = 17;    // ', 'bin_index': '
constexpr uint32_t kFragTail = 2;    // '}
constexpr uint32_t kFragFixed = kFragHead + kFragMid + kFragTail;

// what the size pass knows of one line
struct Line {
  uint32_t is_row;   // 1: a row; 0: skipped (short, header, or contig masked out)
  uint32_t key_len, pk_len, frag_len;
  uint32_t flags;    // AVDB_EXIST_*
  uint32_t lone_cr;  // '\r' bytes of the line that no '\n' follows
};

// one row as the write pass reads it: its line's offset in the slab and the lengths
// the size pass wrote (frag_len possibly patched by the caller)
struct Row {
  uint64_t start;
  uint32_t key_len, pk_len, frag_len, flags;
};

// the contig label's bit in the mask: canonical label c -> c, any other -> kOtherBit
template <class CP>
AVDB_HD uint32_t contig_bit(CP p, uint32_t n) {
  if (n == 1) {
    if (p[0] >= '1' && p[0] <= '9') return p[0] - '1';
    if (p[0] == 'X') return 22;
    if (p[0] == 'Y') return 23;
    if (p[0] == 'M') return 24;
  } else if (n == 2 && p[0] >= '1' && p[0] <= '2' && p[1] >= '0' && p[1] <= '9') {
    const uint32_t v = (p[0] - '0') * 10u + (p[1] - '0');
    if (v <= 22) return v - 1;
  }
  return kOtherBit;
}

// a byte Python's repr() of a str does not render as itself inside '...'
AVDB_HD bool repr_escapes(uint32_t c) { return c < 0x20u || c > 0x7Eu || c == '\'' || c == '\\'; }

template <class CP>
AVDB_HD bool is_header(CP p, uint32_t n) {
  const char h[] = "metaseq_id";
  if (n != 10) return false;
  for (uint32_t i = 0; i < 10; ++i)
    if (p[i] != uint8_t(h[i])) return false;
  return true;
}

// from_tsv's rule for one line (its len bytes, '\n' excluded; nl: a '\n' follows).
// CP: a byte pointer in the text's address space (host, global or the LDS stage).
template <class CP>
AVDB_HD Line scan_line(CP line, uint64_t len64, bool nl, uint32_t contig_mask) {
  Line L{0, 0, 0, 0, 0, 0};
  uint32_t n = len64 < 0x7FFFFFFFull ? uint32_t(len64) : 0x7FFFFFFFu;  // (lengths are u32: a longer line is cut)
  if (nl && n && line[n - 1] == '\r') --n;  // "\r\n" is one line end
  uint32_t t[3] = {n, n, n};                // the first three tabs
  uint32_t nt = 0, colon = n;
  bool esc = false;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = line[i];
    if (c == '\t') {
      if (nt < 3) t[nt] = i;
      ++nt;
    } else {
      L.lone_cr += c == '\r';
      if (nt == 0 && c == ':' && colon == n) colon = i;
      if ((nt == 1 || nt == 2) && repr_escapes(c)) esc = true;
    }
  }
  if (nt < 2) return L;  // fewer than 3 fields
  L.key_len = t[0];
  L.pk_len = t[1] - t[0] - 1;
  const uint32_t bin_len = t[2] - t[1] - 1;
  L.frag_len = kFragFixed + L.pk_len + bin_len;
  if (is_header(line, L.key_len)) return L;
  const uint32_t bit = contig_bit(line, colon < L.key_len ? colon : L.key_len);
  if (!((contig_mask >> bit) & 1u)) return L;
  L.is_row = 1;
  L.flags = (esc ? AVDB_EXIST_FRAG_HOST : 0u) | (bit == kOtherBit ? AVDB_EXIST_NONCANON : 0u);
  return L;
}

// ---- the write pass: byte k of a row's three outputs ---------------------------
// T: pos -> the slab's byte at offset pos (0 outside the row's window), so a length
// the caller patched wrongly reads nothing outside the text.
template <class T>
AVDB_HD uint32_t key_byte(const Row& r, uint32_t k, T text) { return text(r.start + k); }

template <class T>
AVDB_HD uint32_t pk_byte(const Row& r, uint32_t k, T text) { return text(r.start + r.key_len + 1 + k); }

template <class T>
AVDB_HD uint32_t frag_byte(const Row& r, uint32_t k, T text) {
  const char head[] = "{'primary_key': '", mid[] = "', 'bin_index': '", tail[] = "'}";
  if (k < kFragHead) return uint8_t(head[k]);
  k -= kFragHead;
  if (k < r.pk_len) return pk_byte(r, k, text);
  k -= r.pk_len;
  if (k < kFragMid) return uint8_t(mid[k]);
  k -= kFragMid;
  const uint32_t bin_len = r.frag_len >= kFragFixed + r.pk_len ? r.frag_len - kFragFixed - r.pk_len : 0u;
  if (k < bin_len) return text(r.start + r.key_len + 1 + r.pk_len + 1 + k);
  k -= bin_len;
  return k < kFragTail ? uint8_t(tail[k]) : uint32_t(' ');
}

}  // namespace exist
}  // namespace avdb
