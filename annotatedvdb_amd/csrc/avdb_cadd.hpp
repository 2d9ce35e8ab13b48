// K10 — per-line and per-record arithmetic of the CADD table build and the allele
// join, shared by the kernels (avdb_cadd.hip) and the library's host entries
// (avdb_cadd_table_build_host / avdb_cadd_match_host): one definition, compiled
// for both sides, as avdb_vcfline.hpp and avdb_k5.hpp are (line spans: avdb_lines.hpp).
#pragma once

#include "avdb_lines.hpp"

namespace avdb {
namespace cadd {

constexpr uint32_t kContigs = AVDB_CADD_N_CONTIGS;
constexpr uint32_t kUnknown = 255;
// the longest run of AVDB_CADD_ROW_BAD rows the index pass looks across for a row's
// neighbour: the kBadRun + 1 rows on either side are examined (a longer run of
// unparsable rows is an order violation: the table is not usable)
constexpr uint32_t kBadRun = 64;

struct Cols {  // the table's columns as the build writes them
  uint8_t* chrom;
  uint32_t* pos;
  uint64_t* ref_off;
  uint32_t* ref_len;
  uint64_t* alt_off;
  uint32_t* alt_len;
  double* raw;
  double* phred;
  uint8_t* flags;
};

struct View {  // a built table as the join reads it (n_rows == 0: no table)
  uint64_t n_rows;
  const uint8_t* text;
  const uint8_t* chrom;
  const uint32_t* pos;
  const uint64_t* ref_off;
  const uint32_t* ref_len;
  const uint64_t* alt_off;
  const uint32_t* alt_len;
  const double* raw;
  const double* phred;
  const uint8_t* flags;
  const uint32_t* first_row;
  const uint32_t* end_row;
};

// 10^k, exact in f64 for k <= 22
AVDB_HD double pow10_exact(uint32_t k) {
  constexpr double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                            1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return t[k];
}

AVDB_HD bool is_digit(uint32_t c) { return c - '0' < 10u; }

// -?digits[.digits] with at most 15 significant digits (leading zeros stripped)
// and at most 22 fractional digits: the digits as an integer below 2^53, one
// correctly rounded division by an exact power of ten, then the sign — the value
// Python's float(text) gives, bit for bit (-0.0 included).  Anything else: false.
// CP: a byte pointer in the text's address space (host, global or the LDS stage).
template <class CP>
AVDB_HD bool parse_score(CP p, uint32_t n, double* out) {
  uint32_t i = 0;
  const bool neg = n && p[0] == '-';
  if (neg) i = 1;
  if (i >= n || !is_digit(p[i])) return false;
  uint64_t m = 0;
  uint32_t sig = 0, frac = 0;
  for (; i < n && is_digit(p[i]); ++i) {
    m = m * 10u + (p[i] - '0');
    sig += m != 0;
    if (sig > 15) return false;
  }
  if (i < n) {
    if (p[i] != '.' || i + 1 >= n) return false;
    for (++i; i < n && is_digit(p[i]); ++i) {
      m = m * 10u + (p[i] - '0');
      sig += m != 0;
      if (sig > 15 || ++frac > 22) return false;
    }
    if (i < n) return false;
  }
  const double v = double(m) / pow10_exact(frac);
  *out = neg ? -v : v;
  return true;
}

// CADD's contig labels: 1..22, X, Y and MT (the project's M, cadd_updater.py:171,179)
template <class CP>
AVDB_HD uint32_t contig_code(CP p, uint32_t n) {
  if (n == 1) {
    if (p[0] >= '1' && p[0] <= '9') return p[0] - '1';
    if (p[0] == 'X') return 22;
    if (p[0] == 'Y') return 23;
  } else if (n == 2) {
    if (p[0] == 'M' && p[1] == 'T') return 24;
    if (p[0] >= '1' && p[0] <= '2' && is_digit(p[1])) {
      const uint32_t v = (p[0] - '0') * 10u + (p[1] - '0');
      if (v <= 22) return v - 1;
    }
  }
  return kUnknown;
}

// a data line: not empty and not a '#' header line
AVDB_HD bool is_data_line(const uint8_t* text, uint64_t s, uint64_t e) { return e > s && text[s] != '#'; }

// one data line -> row r.  line: its len bytes (in whatever address space they were
// staged); s: its offset in the slab, which the allele offsets count from.
// Returns the row's flags.
template <class CP>
AVDB_HD uint32_t parse_row(CP line, uint64_t s, uint64_t len, uint64_t r, const Cols& o) {
  uint32_t f[7];  // starts of fields 0..5, then one past the end of field 5 + 1
  uint32_t nf = 1;
  f[0] = 0;
  const uint32_t e = len < 0x7FFFFFFFull ? uint32_t(len) : 0u;  // (no line is that long: BAD)
  for (uint32_t i = 0; i < e && nf < 7; ++i)
    if (line[i] == '\t') f[nf++] = i + 1;
  if (nf < 7) f[nf] = e + 1;  // the last field ends at the line end
  uint32_t flags = 0;
  uint64_t pos = 0;
  if (nf < 6) {
    flags = AVDB_CADD_ROW_BAD;
  } else {
    const uint32_t p0 = f[1], p1 = f[2] - 1;
    if (p0 >= p1) flags = AVDB_CADD_ROW_BAD;
    for (uint32_t i = p0; i < p1 && !flags; ++i) {
      pos = pos * 10u + (line[i] - '0');
      if (!is_digit(line[i]) || pos > 0xFFFFFFFFull) flags = AVDB_CADD_ROW_BAD;
    }
    if (pos == 0) flags = AVDB_CADD_ROW_BAD;
  }
  if (flags) {  // never matches; the index pass gives it its predecessor's pos
    o.chrom[r] = uint8_t(kUnknown);
    o.pos[r] = 0;
    o.ref_off[r] = o.alt_off[r] = s;
    o.ref_len[r] = o.alt_len[r] = 0;
    o.raw[r] = o.phred[r] = 0.0;
    o.flags[r] = uint8_t(flags);
    return flags;
  }
  double raw = 0.0, phred = 0.0;
  if (!parse_score(line + f[4], f[5] - 1 - f[4], &raw)) flags |= AVDB_CADD_ROW_SCORE_HOST;
  if (!parse_score(line + f[5], f[6] - 1 - f[5], &phred)) flags |= AVDB_CADD_ROW_SCORE_HOST;
  o.chrom[r] = uint8_t(contig_code(line, f[1] - 1));
  o.pos[r] = uint32_t(pos);
  o.ref_off[r] = s + f[2];
  o.ref_len[r] = f[3] - 1 - f[2];
  o.alt_off[r] = s + f[3];
  o.alt_len[r] = f[4] - 1 - f[3];
  o.raw[r] = raw;
  o.phred[r] = phred;
  o.flags[r] = uint8_t(flags);
  return flags;
}

// What row i means for the contig index: the start and / or the end of a run of
// its contig, and whether it breaks the order tabix requires.  Neighbours are the
// nearest rows that are not AVDB_CADD_ROW_BAD; a BAD row takes the pos of the row
// before it, so the join's binary search sees one non-decreasing column.
struct IndexEvent {
  uint32_t contig;  // kUnknown: no index entry
  bool start, end, violation;
};

AVDB_HD IndexEvent index_row(const uint8_t* chrom, uint32_t* pos, const uint8_t* flags, uint64_t n, uint64_t i) {
  IndexEvent ev{kUnknown, false, false, false};
  uint64_t p = i;  // nearest good row before i (i: none)
  bool lost = false;
  for (uint32_t k = 0; p == i && k <= kBadRun && k < i; ++k)
    if (!(flags[i - 1 - k] & AVDB_CADD_ROW_BAD)) p = i - 1 - k;
  if (p == i && i > kBadRun) lost = true;
  if (flags[i] & AVDB_CADD_ROW_BAD) {
    if (p != i) pos[i] = pos[p];
    ev.violation = lost;
    return ev;
  }
  uint64_t q = n;  // nearest good row after i (n: none)
  for (uint32_t k = 0; q == n && k <= kBadRun && i + 1 + k < n; ++k)
    if (!(flags[i + 1 + k] & AVDB_CADD_ROW_BAD)) q = i + 1 + k;
  const uint32_t c = chrom[i];
  ev.violation = lost;
  if (c >= kContigs) return ev;
  ev.contig = c;
  ev.start = p == i || chrom[p] != c;
  ev.end = q == n || chrom[q] != c;
  if (!ev.start && pos[i] < pos[p]) ev.violation = true;
  return ev;
}

// ---- the join --------------------------------------------------------------
// n bytes at a and b equal?  8 at a time where both sides reach 8-byte alignment
// together (whole words inside [a, a + n) only); bytewise otherwise.
AVDB_HD bool bytes_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
  uint32_t i = 0;
  if (((reinterpret_cast<uintptr_t>(a) ^ reinterpret_cast<uintptr_t>(b)) & 7) == 0 && n >= 16) {
    const uint32_t head = uint32_t((8 - (reinterpret_cast<uintptr_t>(a) & 7)) & 7);
    for (; i < head; ++i)
      if (a[i] != b[i]) return false;
    for (; i + 8 <= n; i += 8)
      if (*reinterpret_cast<const uint64_t*>(a + i) != *reinterpret_cast<const uint64_t*>(b + i)) return false;
  }
  for (; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

AVDB_HD bool allele_is(const uint8_t* x, uint32_t xl, const uint8_t* y, uint32_t yl) {
  return xl == yl && bytes_equal(x, y, xl);
}

// first row of [lo, hi) with pos >= want
AVDB_HD uint64_t lower_bound(const uint32_t* pos, uint64_t lo, uint64_t hi, uint32_t want) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (pos[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// CADDUpdater.buffer_variant's row test (cadd_updater.py:201-204) over the rows
// at the record's position, first row in file order: -1 when none matches
AVDB_HD int64_t match_rows(const View& t, uint32_t c, uint32_t pos, const uint8_t* ref, uint32_t rl, const uint8_t* alt,
                           uint32_t al) {
  if (!t.n_rows) return -1;
  uint64_t lo = t.first_row[c], hi = t.end_row[c];
  if (hi > t.n_rows) hi = t.n_rows;
  if (lo >= hi) return -1;
  for (uint64_t r = lower_bound(t.pos, lo, hi, pos); r < hi && t.pos[r] == pos; ++r) {
    if (t.flags[r] & AVDB_CADD_ROW_BAD) continue;
    const uint8_t* R = t.text + t.ref_off[r];
    const uint8_t* A = t.text + t.alt_off[r];
    const uint32_t Rl = t.ref_len[r], Al = t.alt_len[r];
    if (!allele_is(ref, rl, R, Rl) && !allele_is(ref, rl, A, Al)) continue;
    if (allele_is(alt, al, R, Rl) || allele_is(alt, al, A, Al)) return int64_t(r);
  }
  return -1;
}

// a caller's table as the join reads it; false: a struct this library cannot read
inline bool table_view(const avdb_cadd_table* t, View* v, const char** err) {
  *v = View{};
  if (!t) return true;
  if (t->struct_size != sizeof(avdb_cadd_table)) { *err = "avdb_cadd_table.struct_size does not match this library"; return false; }
  if (t->n_rows == 0) return true;
  if (t->n_rows >= 0x7FFFFFFFull) { *err = "table of 2^31 rows or more"; return false; }
  if (!t->text || !t->chrom || !t->pos || !t->ref_off || !t->ref_len || !t->alt_off || !t->alt_len || !t->raw ||
      !t->phred || !t->flags || !t->first_row || !t->end_row) {
    *err = "null table column";
    return false;
  }
  *v = View{t->n_rows, t->text,  t->chrom, t->pos,   t->ref_off,   t->ref_len, t->alt_off,
            t->alt_len, t->raw, t->phred, t->flags, t->first_row, t->end_row};
  return true;
}

// one record: *row and the kind; raw / phred written only for a matched record
AVDB_HD uint32_t match_record(const View& snv, const View& indel, uint32_t c, uint32_t pos, const uint8_t* heap,
                              uint64_t heap_bytes, uint64_t off, uint32_t rl, uint32_t al, int32_t* row, double* raw,
                              double* phred) {
  *row = -1;
  if (c >= kContigs) return AVDB_CADD_HOST;
  if (off > heap_bytes || uint64_t(rl) + al > heap_bytes - off) return AVDB_CADD_NONE;  // not inside the heap
  const bool is_indel = rl > 1 || al > 1;  // cadd_updater.py:189
  const View& t = is_indel ? indel : snv;
  const int64_t r = match_rows(t, c, pos, heap + off, rl, heap + off + rl, al);
  if (r < 0) return AVDB_CADD_NONE;
  *row = int32_t(r);
  *raw = t.raw[r];
  *phred = t.phred[r];
  return is_indel ? AVDB_CADD_INDEL : AVDB_CADD_SNV;
}

}  // namespace cadd
}  // namespace avdb
