// K14 — per-line and per-row code of the per-chromosome VCF files written from an export
// of AnnotatedVDB.Variant (record_primary_key<TAB>metaseq_id<TAB>row_algorithm_id), shared
// by the kernels (avdb_expvcf.hip) and the library's host entries
// (avdb_export_vcf_size_host / avdb_export_vcf_write_host): one definition, compiled for
// both sides, as avdb_caddupd.hpp is.
#pragma once

#include "avdb_existing.hpp"

namespace avdb {
namespace expvcf {

constexpr uint32_t kValid = 1, kInvalid = 2;  // a line's class (0: no row)
constexpr uint32_t kVcfFixed = 8;             // a VCF row beside its metaseq id and key: 7 tabs, 3 dots, the LF, less 3 ':'
constexpr uint32_t kNoneLen = 4;              // None: how Python prints a NULL row_algorithm_id

// what the size pass knows of one line
struct Line {
  uint32_t cls;       // kValid (BAD rows included), kInvalid, or 0: no row
  uint32_t filtered;  // 1: its contig's bit is clear in the mask (no row)
  uint32_t pk_len, ms_len, out_len, flags;
  uint32_t lone_cr;
  uint64_t pk_hash;
};

// one row as the write pass reads it
struct Row {
  uint64_t start;  // its line's offset in the slab
  uint32_t pk_len, ms_len, out_len, flags;
};

AVDB_HD uint64_t mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// K6's streaming hash of a byte string (avdb_keyset.hip's Hasher, here for both sides):
// little-endian 8-byte words mixed in as they complete, closed by the length, 0 -> 1
struct Hasher {
  uint64_t h = 0x9E3779B97F4A7C15ull, w = 0;
  uint32_t n = 0;
  AVDB_HD void put(uint32_t c) {
    w |= uint64_t(c & 0xFFu) << (8 * (n & 7));
    if ((++n & 7) == 0) {
      h = mix(h ^ w);
      w = 0;
    }
  }
  AVDB_HD uint64_t done() const {
    const uint64_t x = mix(h ^ w ^ (uint64_t(n) << 56));
    return x ? x : 1ull;
  }
};

template <class CP>
AVDB_HD bool is_header(CP p, uint32_t n) {
  const char h[] = "record_primary_key";
  if (n != 18) return false;
  for (uint32_t i = 0; i < 18; ++i)
    if (p[i] != uint8_t(h[i])) return false;
  return true;
}

// a byte of INVALID_ALLELES = 'I|R|D|N' (export_variant2vcf.py:27)
AVDB_HD bool is_invalid_byte(uint32_t c) { return c == 'I' || c == 'R' || c == 'D' || c == 'N'; }

// row_algorithm_id as text: NULL when absent, empty or \N
template <class CP>
AVDB_HD bool alg_is_null(CP p, uint32_t n) { return n == 0 || (n == 2 && p[0] == '\\' && p[1] == 'N'); }

// One line of the export (its len bytes, '\n' excluded; nl: a '\n' follows) by K13's line
// rule and the classes of export_variant2vcf.py:63-80.  CP: a byte pointer in the text's
// address space (host, global or the LDS stage).
template <class CP>
AVDB_HD Line scan_line(CP line, uint64_t len64, bool nl, uint32_t contig_mask) {
  Line L{0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t n = len64 < 0x7FFFFFFFull ? uint32_t(len64) : 0x7FFFFFFFu;  // (lengths are u32: a longer line is cut)
  if (nl && n && line[n - 1] == '\r') --n;  // "\r\n" is one line end
  uint32_t t[3] = {n, n, n};                // the first three tabs
  uint32_t nt = 0, nc = 0, colon = n;       // the metaseq id's ':' and the first of them
  bool invalid = false;
  Hasher hs;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = line[i];
    if (c == '\t') {
      if (nt < 3) t[nt] = i;
      ++nt;
      continue;
    }
    L.lone_cr += c == '\r';
    if (nt == 0) {
      hs.put(c);
    } else if (nt == 1) {
      if (c == ':') {
        if (!nc) colon = i;
        ++nc;
      }
      invalid |= is_invalid_byte(c);
    }
  }
  if (nt < 1) return L;  // empty, or fewer than two fields
  L.pk_len = t[0];
  if (is_header(line, L.pk_len)) return L;
  const uint32_t m0 = t[0] + 1, m1 = t[1];  // the metaseq id
  L.ms_len = m1 - m0;
  const uint32_t bit = exist::contig_bit(line + m0, (nc ? colon : m1) - m0);
  if (!((contig_mask >> bit) & 1u)) {
    L.filtered = 1;
    return L;
  }
  if (invalid) {  // matches('I|R|D|N', metaseqId), before any other test of the id
    const uint32_t a0 = t[1] + 1, al = nt >= 2 ? t[2] - a0 : 0u;
    L.cls = kInvalid;
    L.out_len = L.pk_len + 1 + (nt < 2 || alg_is_null(line + a0, al) ? kNoneLen : al) + 1;
    return L;
  }
  L.cls = kValid;
  L.pk_hash = hs.done();
  if (nc != 3) {  // chr, pos, ref, alt = metaseqId.split(':') raises
    L.flags = AVDB_EXPVCF_BAD;
    return L;
  }
  L.out_len = L.ms_len + L.pk_len + kVcfFixed;
  return L;
}

// ---- the write pass ----------------------------------------------------------------
// text(pos): the slab's byte at offset pos (0 outside the text); put(k, c): byte k of the
// row, called for k < row.out_len only, so lengths that do not describe the text write
// nothing outside the row's span.

// a VCF row, label<TAB>pos<TAB>pk<TAB>ref<TAB>alt<TAB>.<TAB>.<TAB>.<LF>: the metaseq id with
// its ':' as tabs and the key behind the second.  A BAD or DROPPED row has no bytes; a
// ROW_HOST row's span (the length the caller stored) is filled with spaces for the caller
// to overwrite.
template <class TextAt, class Put>
AVDB_HD void render_vcf_row(const Row& row, TextAt text, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < row.out_len) put_any(k, c);
  };
  if (row.flags & (AVDB_EXPVCF_ROW_HOST | AVDB_EXPVCF_BAD | AVDB_EXPVCF_DROPPED)) {
    for (uint32_t k = 0; k < row.out_len; ++k) put(k, uint32_t(' '));
    return;
  }
  const uint64_t m0 = row.start + row.pk_len + 1;
  uint32_t k = 0, nc = 0;
  for (uint32_t i = 0; i < row.ms_len && k < row.out_len; ++i) {  // (lengths that overrun the row end the walk)
    const uint32_t c = text(m0 + i);
    if (c != ':') {
      put(k++, c);
      continue;
    }
    put(k++, uint32_t('\t'));
    if (++nc == 2) {
      for (uint32_t j = 0; j < row.pk_len && k < row.out_len; ++j) put(k++, text(row.start + j));
      put(k++, uint32_t('\t'));
    }
  }
  for (uint32_t j = 0; j < 3; ++j) {
    put(k++, uint32_t('\t'));
    put(k++, uint32_t('.'));
  }
  put(k++, uint32_t('\n'));
  for (; k < row.out_len; ++k) put(k, uint32_t(' '));  // (a length the caller stored longer)
}

// a row of the invalid file, pk<TAB>alg<LF>; alg: the third field verbatim, or None.  The
// field is found again behind the metaseq id (the row list carries no offset of it); its
// length is what the size pass left of out_len.
template <class TextAt, class Put>
AVDB_HD void render_invalid_row(const Row& row, uint64_t text_bytes, TextAt text, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < row.out_len) put_any(k, c);
  };
  uint32_t k = 0;
  for (uint32_t j = 0; j < row.pk_len && k < row.out_len; ++j) put(k++, text(row.start + j));
  put(k++, uint32_t('\t'));
  uint64_t p = row.start + row.pk_len + 1;  // the metaseq id: to its tab, or the line's end
  while (p < text_bytes && text(p) != '\t' && text(p) != '\n') ++p;
  const uint32_t al = row.out_len >= row.pk_len + 2 ? row.out_len - row.pk_len - 2 : 0u;
  bool null = !(p < text_bytes && text(p) == '\t');
  const uint64_t a0 = p + 1;
  if (!null) {
    uint64_t q = a0;  // the field's own end, one '\r' before the '\n' stripped
    while (q < text_bytes && text(q) != '\t' && text(q) != '\n') ++q;
    if (q > a0 && q < text_bytes && text(q) == '\n' && text(q - 1) == '\r') --q;
    null = q == a0 || (q - a0 == 2 && text(a0) == '\\' && text(a0 + 1) == 'N');
  }
  if (null) {
    const char none[] = "None";
    for (uint32_t j = 0; j < kNoneLen && j < al; ++j) put(k++, uint32_t(uint8_t(none[j])));
  } else {
    for (uint32_t j = 0; j < al; ++j) put(k++, text(a0 + j));
  }
  put(k++, uint32_t('\n'));
  for (; k < row.out_len; ++k) put(k, uint32_t(' '));
}

}  // namespace expvcf
}  // namespace avdb
