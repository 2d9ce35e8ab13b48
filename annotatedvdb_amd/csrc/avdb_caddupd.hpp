// K13 — per-line and per-row code of the CADD update rows rendered from an export of
// AnnotatedVDB.Variant (record_primary_key<TAB>metaseq_id<TAB>cadd_scores), shared by
// the kernels (avdb_caddupd.hip) and the library's host entries
// (avdb_cadd_update_size_host / avdb_cadd_update_write_host): one definition,
// compiled for both sides, as avdb_existing.hpp is.
#pragma once

#include "avdb_cadd.hpp"
#include "avdb_existing.hpp"

namespace avdb {
namespace caddupd {

constexpr uint32_t kChromMax = AVDB_CADDUPD_CHROM_MAX;

// the JSON around the two scores: {"CADD_raw_score": R, "CADD_phred": P}
constexpr uint32_t kJsonHead = 19;  // {"CADD_raw_score":<space>
constexpr uint32_t kJsonMid = 16;   // , "CADD_phred":<space>

struct Tables {
  cadd::View snv, indel;
  uint64_t snv_bytes, indel_bytes;  // the tables' text sizes: a score field ends there at the latest
};

// the caller's chromosome text ('chr' + label), by value in the kernel arguments
struct Chrom {
  uint32_t len;  // 0: none set, the row's own 'chr' + pk label
  uint8_t text[kChromMax];
};

// what the size pass knows of one line
struct Line {
  uint32_t is_row;   // 1: a row (BAD and ROW_HOST rows included)
  uint32_t skipped;  // 1: annotated already, counted `skipped` under skip_existing (no row)
  uint32_t pk_len, kind, out_len, flags;
  int32_t row;       // the matched table row (-1: none)
  uint32_t lone_cr;
};

// one row as the write pass reads it
struct Row {
  uint64_t start;  // its line's offset in the slab
  uint32_t pk_len, kind, out_len, flags;
  int32_t row;
};

// ---- json.dumps(float(text)) as a rewrite of the digits -------------------------
// For every text parse_score accepts — -?digits[.digits], at most 15 significant and
// 22 fractional digits — the shortest digits that round-trip are the text's own with
// the leading and trailing zeros stripped (15 decimal digits always survive a double),
// so repr is a rewrite: with the value 0.d1d2.. x 10^decpt, exponent form d[.ddd]e-XX
// when decpt <= -4, positional form otherwise (decpt <= 15 here), '.0' behind an
// integer, zero as 0.0 / -0.0.  put(k, c): byte k of the result.  Returns its length;
// 0: a text parse_score refuses (the caller's float() and json.dumps).
template <class CP, class Put>
AVDB_HD uint32_t score_text(CP p, uint32_t n, Put put) {
  double unused;
  if (!cadd::parse_score(p, n, &unused)) return 0;
  const uint32_t neg = p[0] == '-';
  uint32_t dot = n;
  for (uint32_t i = neg; i < n; ++i)
    if (p[i] == '.') dot = i;
  const uint32_t P = dot - neg;                         // digits before the point
  const uint32_t L = dot < n ? n - neg - 1 : n - neg;   // all digits
  auto digit = [&](uint32_t j) -> uint32_t { return p[neg + j + (j >= P ? 1u : 0u)]; };
  uint32_t a = L, b = 0;  // first and last non-zero digit
  for (uint32_t j = 0; j < L; ++j)
    if (digit(j) != '0') {
      if (a == L) a = j;
      b = j;
    }
  uint32_t k = 0;
  if (neg) put(k++, uint32_t('-'));
  if (a == L) {
    put(k++, uint32_t('0'));
    put(k++, uint32_t('.'));
    put(k++, uint32_t('0'));
    return k;
  }
  const uint32_t nd = b - a + 1;
  const int32_t decpt = int32_t(P) - int32_t(a);
  if (decpt <= -4) {
    put(k++, digit(a));
    if (nd > 1) {
      put(k++, uint32_t('.'));
      for (uint32_t j = a + 1; j <= b; ++j) put(k++, digit(j));
    }
    const uint32_t e = uint32_t(1 - decpt);  // 5 .. 22
    put(k++, uint32_t('e'));
    put(k++, uint32_t('-'));
    put(k++, '0' + e / 10u);
    put(k++, '0' + e % 10u);
  } else if (decpt <= 0) {
    put(k++, uint32_t('0'));
    put(k++, uint32_t('.'));
    for (int32_t z = decpt; z < 0; ++z) put(k++, uint32_t('0'));
    for (uint32_t j = a; j <= b; ++j) put(k++, digit(j));
  } else {
    const uint32_t ip = uint32_t(decpt);  // digits before the point
    for (uint32_t j = 0; j < ip; ++j) put(k++, j < nd ? digit(a + j) : uint32_t('0'));
    put(k++, uint32_t('.'));
    if (nd <= ip) put(k++, uint32_t('0'));
    for (uint32_t j = ip; j < nd; ++j) put(k++, digit(a + j));
  }
  return k;
}

// the two score fields of table row r: they start behind alt_off + alt_len + 1; the
// first ends at its tab, the second at a tab, the line's end or the text's
AVDB_HD void score_fields(const cadd::View& t, uint64_t text_bytes, uint64_t r, uint64_t* s0, uint32_t* n0,
                          uint64_t* s1, uint32_t* n1) {
  uint64_t p = t.alt_off[r] + t.alt_len[r] + 1;
  if (p > text_bytes) p = text_bytes;
  uint64_t q = p;
  while (q < text_bytes && t.text[q] != '\t' && t.text[q] != '\n') ++q;
  *s0 = p;
  *n0 = uint32_t(q - p < 0x7FFFFFFFull ? q - p : 0u);
  uint64_t u = q < text_bytes && t.text[q] == '\t' ? q + 1 : q;
  uint64_t v = u;
  while (v < text_bytes && t.text[v] != '\t' && t.text[v] != '\n') ++v;
  *s1 = u;
  *n1 = uint32_t(v - u < 0x7FFFFFFFull ? v - u : 0u);
}

// the JSON text of a row matched at table row r; 0: a score the device does not render
template <class Put>
AVDB_HD uint32_t json_text(const cadd::View& t, uint64_t text_bytes, uint64_t r, Put put) {
  const char head[] = "{\"CADD_raw_score\": ", mid[] = ", \"CADD_phred\": ";
  uint64_t s0, s1;
  uint32_t n0, n1;
  score_fields(t, text_bytes, r, &s0, &n0, &s1, &n1);
  uint32_t k = 0;
  for (uint32_t i = 0; i < kJsonHead; ++i) put(k++, uint32_t(uint8_t(head[i])));
  const uint32_t a = score_text(t.text + s0, n0, [&](uint32_t j, uint32_t c) { put(k + j, c); });
  if (!a) return 0;
  k += a;
  for (uint32_t i = 0; i < kJsonMid; ++i) put(k++, uint32_t(uint8_t(mid[i])));
  const uint32_t b = score_text(t.text + s1, n1, [&](uint32_t j, uint32_t c) { put(k + j, c); });
  if (!b) return 0;
  k += b;
  put(k++, uint32_t('}'));
  return k;
}

template <class CP>
AVDB_HD bool is_header(CP p, uint32_t n) {
  const char h[] = "record_primary_key";
  if (n != 18) return false;
  for (uint32_t i = 0; i < 18; ++i)
    if (p[i] != uint8_t(h[i])) return false;
  return true;
}

// the project's contig code of a metaseq id's label (cadd._CODE: 1..22, X, Y, M, and MT as M)
template <class CP>
AVDB_HD uint32_t label_code(CP p, uint32_t n) {
  if (n == 2 && p[0] == 'M' && p[1] == 'T') return 24;
  const uint32_t b = exist::contig_bit(p, n);
  return b == exist::kOtherBit ? cadd::kUnknown : b;
}

// the length of the chrom field: the caller's text, or 'chr' + the pk before its first ':'
AVDB_HD uint32_t chrom_len(const Chrom& ch, uint32_t pk_label_len) { return ch.len ? ch.len : 3u + pk_label_len; }

// One line of the export (its len bytes, '\n' excluded; nl: a '\n' follows) by the rule
// of load_cadd_scores.py:109-120 and cadd_updater.py:187-221.  line: the bytes in
// whatever address space they were staged; gline: the same bytes where the join reads
// the alleles (host or global memory).
template <class CP>
AVDB_HD Line scan_line(CP line, const uint8_t* gline, uint64_t len64, bool nl, uint32_t contig_mask,
                       bool skip_existing, const Chrom& ch, const Tables& T) {
  Line L{0, 0, 0, AVDB_CADD_NONE, 0, 0, -1, 0};
  uint32_t n = len64 < 0x7FFFFFFFull ? uint32_t(len64) : 0x7FFFFFFFu;  // (lengths are u32: a longer line is cut)
  if (nl && n && line[n - 1] == '\r') --n;  // "\r\n" is one line end
  uint32_t t[3] = {n, n, n};                // the first three tabs
  uint32_t col[3] = {n, n, n};              // the first three ':' of the metaseq id
  uint32_t nt = 0, nc = 0, pk_colon = n;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = line[i];
    if (c == '\t') {
      if (nt < 3) t[nt] = i;
      ++nt;
    } else {
      L.lone_cr += c == '\r';
      if (c == ':') {
        if (nt == 0 && pk_colon == n) pk_colon = i;
        if (nt == 1) {
          if (nc < 3) col[nc] = i;
          ++nc;
        }
      }
    }
  }
  if (nt < 1) return L;  // empty, or fewer than two fields
  L.pk_len = t[0];
  if (is_header(line, L.pk_len)) return L;
  const uint32_t m0 = t[0] + 1, m1 = t[1];  // the metaseq id
  const uint32_t lab = (nc ? col[0] : m1) - m0;
  const uint32_t bit = exist::contig_bit(line + m0, lab);
  if (!((contig_mask >> bit) & 1u)) return L;
  if (skip_existing && nt >= 2) {  // cadd_scores: NULL when absent, empty or \N
    const uint32_t s0 = t[1] + 1, sl = t[2] - s0;
    if (!(sl == 0 || (sl == 2 && line[s0] == '\\' && line[s0 + 1] == 'N'))) {
      L.skipped = 1;
      return L;
    }
  }
  L.is_row = 1;
  if (nc != 3) {  // c, p, r, a = m.split(":") raises
    L.flags = AVDB_CADDUPD_BAD;
    return L;
  }
  const uint32_t code = label_code(line + m0, lab);
  const uint32_t p0 = col[0] + 1, p1 = col[1];
  uint64_t pos = 0;
  bool plain = p1 > p0 && p1 - p0 <= 10 && code < cadd::kContigs;
  for (uint32_t i = p0; i < p1 && plain; ++i) {
    plain = cadd::is_digit(line[i]);
    pos = pos * 10u + (line[i] - '0');
  }
  if (!plain || pos > 0xFFFFFFFFull) {
    L.flags = AVDB_CADDUPD_ROW_HOST;
    return L;
  }
  const uint32_t r0 = col[1] + 1, rl = col[2] - r0, a0 = col[2] + 1, al = m1 - a0;
  const bool is_indel = rl > 1 || al > 1;  // cadd_updater.py:189
  const cadd::View& tab = is_indel ? T.indel : T.snv;
  const int64_t r = cadd::match_rows(tab, code, uint32_t(pos), gline + r0, rl, gline + a0, al);
  uint32_t json = 2;  // {}
  if (r >= 0) {
    if (tab.flags[r] & AVDB_CADD_ROW_SCORE_HOST) {
      L.flags = AVDB_CADDUPD_ROW_HOST;
      return L;
    }
    json = json_text(tab, is_indel ? T.indel_bytes : T.snv_bytes, uint64_t(r), [](uint32_t, uint32_t) {});
    if (!json) {  // (a table whose flags do not describe its text)
      L.flags = AVDB_CADDUPD_ROW_HOST;
      return L;
    }
    L.row = int32_t(r);
    L.kind = is_indel ? AVDB_CADD_INDEL : AVDB_CADD_SNV;
  }
  const uint64_t out = uint64_t(L.pk_len) + 1 + chrom_len(ch, pk_colon < L.pk_len ? pk_colon : L.pk_len) + 1 + json + 1;
  if (out > 0xFFFFFFFFull) {
    L.flags = AVDB_CADDUPD_ROW_HOST;
    L.row = -1;
    L.kind = AVDB_CADD_NONE;
    return L;
  }
  L.out_len = uint32_t(out);
  return L;
}

// ---- the write pass: one row's text, pk<TAB>chrom<TAB>json<LF> ---------------------
// text(pos): the slab's byte at offset pos (0 outside the row's window); put(k, c):
// byte k of the row, called for k < row.out_len only, so lengths that do not describe
// the text write nothing outside the row's span.  A BAD row has no bytes; a ROW_HOST
// row's span (the length the caller patched in) is filled with spaces for the caller
// to overwrite.
template <class TextAt, class Put>
AVDB_HD void render_row(const Row& row, const Chrom& ch, const Tables& T, TextAt text, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < row.out_len) put_any(k, c);
  };
  if (row.flags & (AVDB_CADDUPD_ROW_HOST | AVDB_CADDUPD_BAD)) {
    for (uint32_t k = 0; k < row.out_len; ++k) put(k, uint32_t(' '));
    return;
  }
  uint32_t k = 0, colon = row.pk_len;
  for (uint32_t i = 0; i < row.pk_len; ++i) {
    const uint32_t c = text(row.start + i);
    if (c == ':' && colon == row.pk_len) colon = i;
    put(k++, c);
  }
  put(k++, uint32_t('\t'));
  if (ch.len) {
    for (uint32_t i = 0; i < ch.len && i < kChromMax; ++i) put(k++, uint32_t(ch.text[i]));
  } else {
    put(k++, uint32_t('c'));
    put(k++, uint32_t('h'));
    put(k++, uint32_t('r'));
    for (uint32_t i = 0; i < colon; ++i) put(k++, text(row.start + i));
  }
  put(k++, uint32_t('\t'));
  const bool is_indel = row.kind == AVDB_CADD_INDEL;
  const cadd::View& tab = is_indel ? T.indel : T.snv;
  if (row.kind == AVDB_CADD_NONE || row.row < 0 || uint64_t(row.row) >= tab.n_rows) {
    put(k++, uint32_t('{'));
    put(k++, uint32_t('}'));
  } else {
    k += json_text(tab, is_indel ? T.indel_bytes : T.snv_bytes, uint64_t(row.row),
                   [&](uint32_t j, uint32_t c) { put(k + j, c); });
  }
  put(k++, uint32_t('\n'));
  for (; k < row.out_len; ++k) put(k, uint32_t(' '));  // (a length the caller patched longer)
}

}  // namespace caddupd
}  // namespace avdb
