// K17 — per-line and per-row code of the ADSP QC pVCF pass (Load/bin/update_from_qc_pvcf_file.py),
// shared by the kernels (avdb_qc.hip) and the library's host entries: K17a, the table of the QC
// file's alt alleles (lookup ids chrom:pos:ref:alt, one JSON text per line and whether FILTER is
// PASS), and K17b, the update rows from an export of AnnotatedVDB.Variant
// (record_primary_key<TAB>metaseq_id<TAB>adsp_qc).  One definition, compiled for both sides, as
// avdb_lof.hpp is; the line front (fields, CHROM, POS, ID, REF, ALT, the keys) is K16's.
#pragma once

#include "avdb_fmt.hpp"
#include "avdb_lof.hpp"

namespace avdb {
namespace qc {

constexpr uint32_t kHost = 0xFFFFFFFFu;  // a length no text has: the value is left to the host

// the release key ('--version', lower-cased by the caller), passed to the kernels by value
struct Release {
  uint8_t b[AVDB_QC_RELEASE_MAX];
  uint32_t n;
};

// bytes json.dumps leaves as they are inside a string (it escapes DEL as it does the control bytes)
AVDB_HD bool plain_byte(uint32_t c) { return c >= 0x20u && c < 0x7Fu && c != '\\' && c != '"'; }

// does "Infinity" begin at line[i] (i < n)?  generate_update_values raises for a JSON that holds it
template <class CP>
AVDB_HD bool infinity_at(CP line, uint32_t i, uint32_t n) {
  const char w[] = "Infinity";
  if (n - i < 8) return false;
  for (uint32_t k = 0; k < 8; ++k)
    if (line[i + k] != uint32_t(uint8_t(w[k]))) return false;
  return true;
}

// a release the device can write and compare: 1 .. AVDB_QC_RELEASE_MAX plain bytes
inline bool release_ok(const uint8_t* p, size_t n) {
  if (!p || n == 0 || n > AVDB_QC_RELEASE_MAX) return false;
  for (size_t i = 0; i < n; ++i)
    if (!plain_byte(p[i])) return false;
  return true;
}

// ---- numbers: the signed front of number_plain ------------------------------------------------
// json.dumps(float(text)) of digits with one '.', a text number_plain accepts (at most 15
// significant digits, so repr is a rewrite of them, as caddupd::score_text has it): with the value
// 0.d1d2.. x 10^decpt, exponent form d[.ddd]e-XX / e+XX when decpt - 1 < -4 or >= 16, positional
// form otherwise, '.0' behind an integer, zero as 0.0 / -0.0.  Returns the length.
template <class CP, class Put>
AVDB_HD uint32_t float_json(CP p, uint32_t n, bool neg, Put put) {
  uint32_t dot = n;
  for (uint32_t i = 0; i < n; ++i)
    if (p[i] == '.') dot = i;
  const uint32_t P = dot, L = n - 1;  // digits before the point, all digits
  auto digit = [&](uint32_t j) -> uint32_t { return p[j + (j >= P ? 1u : 0u)]; };
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
  if (decpt <= -4 || decpt > 16) {
    put(k++, digit(a));
    if (nd > 1) {
      put(k++, uint32_t('.'));
      for (uint32_t j = a + 1; j <= b; ++j) put(k++, digit(j));
    }
    const uint32_t e = decpt <= -4 ? uint32_t(1 - decpt) : uint32_t(decpt - 1);  // 5 .. 44, 16 .. 39
    put(k++, uint32_t('e'));
    put(k++, uint32_t(decpt <= -4 ? '-' : '+'));
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

// json.dumps(to_numeric(text)) of one value (an INFO value, FILTER, QUAL or FORMAT) whose bytes are
// all plain_byte: a text with a byte outside lof::numberish, or '.', stays a string (in INFO with
// '#' written as ':'); -?digits is an int, without its leading zeros and, when zero, without its
// sign; -? and a text number_plain accepts is a float.  Everything else needs Python to decide
// ('+', exponents, '_', surrounding space, inf / nan / infinity, more than 15 significant digits,
// a lone '-', the empty text): kHost.  put(k, c): byte k.  Returns the length.
template <class CP, class Put>
AVDB_HD uint32_t value_json(CP p, uint32_t n, bool info, Put put) {
  bool text = false, digits = true;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = p[i];
    text = text || !lof::numberish(c);
    digits = digits && (cadd::is_digit(c) || (i == 0 && c == '-'));
  }
  if (text || (n == 1 && p[0] == '.')) {
    uint32_t k = 0;
    put(k++, uint32_t('"'));
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t c = p[i];
      put(k++, info && c == '#' ? uint32_t(':') : c);
    }
    put(k++, uint32_t('"'));
    return k;
  }
  const uint32_t neg = n && p[0] == '-';
  const uint32_t m = n - neg;
  if (m == 0) return kHost;
  if (digits) {
    if (m > lof::kMaxDigits) return kHost;
    uint32_t d = neg;
    while (d + 1 < n && p[d] == '0') ++d;
    uint32_t k = 0;
    if (neg && p[d] != '0') put(k++, uint32_t('-'));
    for (; d < n; ++d) put(k++, uint32_t(p[d]));
    return k;
  }
  if (m > 40 || !number_plain(p + neg, m)) return kHost;
  return float_json(p + neg, m, neg != 0, put);
}

// ---- K17a: one line of the QC VCF ---------------------------------------------------------
// a line as load_annotation sees it: decoded, rstrip()ped, its first nine fields
struct Parsed {
  lof::Parsed b;  // cls (kComment / kEntry), flags (AVDB_QC_LINE_*), n, the first eight tabs, the key's parts
  uint32_t t8;    // the ninth tab (n where the line has nine fields only)
};

// an INFO key with parse_entry's '#' -> ':' applied
template <class CP>
AVDB_HD uint32_t key_byte(CP line, uint32_t i) {
  const uint32_t c = line[i];
  return c == '#' ? uint32_t(':') : c;
}

// the item that starts at a (a <= fe): its end and its key's end (the first '=', or the item's end)
template <class CP>
AVDB_HD void item_at(CP line, uint32_t a, uint32_t fe, uint32_t* end, uint32_t* key_end) {
  uint32_t b = a, ke = fe + 1;
  while (b < fe && line[b] != ';') {
    if (ke > fe && line[b] == '=') ke = b;
    ++b;
  }
  *end = b;
  *key_end = ke > fe ? b : ke;
}

// does an item before the one at `at` have the key [at, ke)?
template <class CP>
AVDB_HD bool key_before(CP line, uint32_t fs, uint32_t fe, uint32_t at, uint32_t ke) {
  for (uint32_t a = fs; a < at;) {
    uint32_t b, e;
    item_at(line, a, fe, &b, &e);
    if (e - a == ke - at) {
      uint32_t i = 0;
      while (i < ke - at && key_byte(line, a + i) == key_byte(line, at + i)) ++i;
      if (i == ke - at) return true;
    }
    a = b + 1;
  }
  return false;
}

constexpr uint64_t kKeyWork = 1ull << 22;  // bytes of earlier items one line may walk through in repeats_key

// does INFO [fs, fe) repeat a key?  (a dict keeps the first position and the last value: the host's)
// Keys are hashed into 256 bits; only a key whose bit is taken is compared with the items before it.
// That walk is quadratic in the worst case: past kKeyWork bytes of it the answer is "maybe" (true),
// which an INFO of some hundred items does not reach and one of thousands does.
template <class CP>
AVDB_HD bool repeats_key(CP line, uint32_t fs, uint32_t fe) {
  uint64_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, work = 0;
  for (uint32_t a = fs; a <= fe;) {
    uint32_t b, ke;
    item_at(line, a, fe, &b, &ke);
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint32_t i = a; i < ke; ++i) h = (h ^ key_byte(line, i)) * 0x100000001B3ull;
    h ^= h >> 29;
    const uint64_t m = 1ull << (h & 63u);
    const uint32_t w = uint32_t(h >> 6) & 3u;
    const uint64_t cur = w == 0 ? b0 : w == 1 ? b1 : w == 2 ? b2 : b3;
    if (cur & m) {
      work += a - fs;
      if (work > kKeyWork || key_before(line, fs, fe, a, ke)) return true;
    }
    b0 |= w == 0 ? m : 0ull;
    b1 |= w == 1 ? m : 0ull;
    b2 |= w == 2 ? m : 0ull;
    b3 |= w == 3 ? m : 0ull;
    a = b + 1;
  }
  return false;
}

// One line of the VCF (its len bytes, '\n' excluded; nl: a '\n' follows) by the rule of
// load_annotation (update_from_qc_pvcf_file.py:226-258), VcfEntryParser.parse_entry and get_variant.
// with_keys: also look for a repeated INFO key (the size pass; the write pass reads its verdict).
template <class CP>
AVDB_HD Parsed parse_line(CP line, uint64_t len64, bool nl, bool with_keys) {
  Parsed Q{};
  lof::Parsed& P = Q.b;
  uint32_t n = len64 < 0x7FFFFFFFull ? uint32_t(len64) : 0x7FFFFFFFu;  // (lengths are u32: a longer line is cut)
  if (nl && n && line[n - 1] == '\r') --n;                              // "\r\n" is one line end
  while (n && lof::strips(line[n - 1])) --n;                            // line.rstrip()
  P.n = n;
  for (uint32_t i = 0; i < 8; ++i) P.t[i] = n;
  Q.t8 = n;
  if (n && line[0] == '#') {
    P.cls = lof::kComment;
    return Q;
  }
  uint32_t nt = 0;
  bool hi = false, odd = false;  // odd: a byte json.dumps escapes, or "Infinity", in QUAL .. FORMAT
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = line[i];
    if (c == '\t') {
      if (nt < 8) P.t[nt] = i;
      if (nt == 8) Q.t8 = i;
      ++nt;
    } else {
      P.lone_cr += c == '\r';
      hi = hi || c >= 0x80u;
      odd = odd || (nt >= 5 && nt <= 8 && (!plain_byte(c) || (c == 'I' && infinity_at(line, i, n))));
    }
  }
  P.cls = lof::kEntry;
  if (nt < 8) {  // fewer fields than the header: parse_entry raises IndexError
    P.flags = AVDB_QC_LINE_HOST | AVDB_QC_LINE_BAD;
    return Q;
  }
  P.flags = AVDB_QC_LINE_HOST;  // until every check has passed
  if (hi || odd) return Q;
  // CHROM: an optional 'chr' and one of the 25 labels, or MT
  uint32_t cs = 0, cn = P.t[0];
  if (cn == 2 && line[0] == 'M' && line[1] == 'T') {
    cn = 1;
  } else {
    if (cn > 3 && line[0] == 'c' && line[1] == 'h' && line[2] == 'r') {
      cs = 3;
      cn -= 3;
    }
    if (exist::contig_bit(line + cs, cn) == exist::kOtherBit) return Q;
  }
  P.chrom_s = cs;
  P.chrom_n = cn;
  // POS: plain digits
  uint32_t ps = P.t[0] + 1;
  const uint32_t pe = P.t[1];
  if (ps >= pe || pe - ps > lof::kMaxDigits) return Q;
  for (uint32_t i = ps; i < pe; ++i)
    if (!cadd::is_digit(line[i])) return Q;
  while (ps + 1 < pe && line[ps] == '0') ++ps;
  P.pos_s = ps;
  P.pos_n = pe - ps;
  // ID: '.' or a text to_numeric leaves a string (the reference dies in id.startswith otherwise)
  const uint32_t is = P.t[1] + 1, ie = P.t[2];
  bool text_id = false;
  for (uint32_t i = is; i < ie && !text_id; ++i) text_id = !lof::numberish(line[i]);
  if (!text_id && !(ie - is == 1 && line[is] == '.')) return Q;
  // REF and ALT
  const uint32_t rs = P.t[2] + 1, re = P.t[3], as = P.t[3] + 1, ae = P.t[4];
  if (!lof::allele_field_ok(line + rs, re - rs) || !lof::allele_field_ok(line + as, ae - as)) return Q;
  // INFO: a text to_numeric leaves a string (a number has no .replace: parse_entry raises)
  const uint32_t fs = P.t[6] + 1, fe = P.t[7];
  bool text_info = fe - fs == 1 && line[fs] == '.';
  for (uint32_t i = fs; i < fe && !text_info; ++i) text_info = !lof::numberish(line[i]);
  if (!text_info) return Q;
  if (with_keys && repeats_key(line, fs, fe)) return Q;
  const uint32_t ls = P.t[5] + 1;  // FILTER
  const bool pass = P.t[6] - ls == 4 && line[ls] == 'P' && line[ls + 1] == 'A' && line[ls + 2] == 'S' && line[ls + 3] == 'S';
  P.flags = pass ? AVDB_QC_PASS : 0u;
  return Q;
}

// json.dumps({release: {"info": {...}, "filter": v, "qual": v, "format": v}}) of a parsed entry;
// kHost: a value outside the device subset
template <class CP, class Put>
AVDB_HD uint32_t line_json(CP line, const Parsed& Q, const Release& rel, Put put) {
  const lof::Parsed& P = Q.b;
  uint32_t k = 0;
  bool host = false;
  auto lit = [&](const char* s) {
    for (uint32_t i = 0; s[i]; ++i) put(k++, uint32_t(uint8_t(s[i])));
  };
  auto value = [&](uint32_t s, uint32_t e, bool info) {
    const uint32_t a = value_json(line + s, e - s, info, [&](uint32_t j, uint32_t c) { put(k + j, c); });
    host = host || a == kHost;
    k += a == kHost ? 0u : a;
  };
  lit("{\"");
  for (uint32_t i = 0; i < rel.n && i < AVDB_QC_RELEASE_MAX; ++i) put(k++, uint32_t(rel.b[i]));
  lit("\": {\"info\": {");
  const uint32_t fs = P.t[6] + 1, fe = P.t[7];
  for (uint32_t a = fs; a <= fe && !host;) {
    uint32_t b, ke;
    item_at(line, a, fe, &b, &ke);
    if (a != fs) lit(", ");
    put(k++, uint32_t('"'));
    for (uint32_t i = a; i < ke; ++i) put(k++, key_byte(line, i));
    lit("\": ");
    if (ke == b) lit("true");  // a bare flag: [item, True]
    else value(ke + 1, b, true);
    a = b + 1;
  }
  lit("}, \"filter\": ");
  value(P.t[5] + 1, P.t[6], false);
  lit(", \"qual\": ");
  value(P.t[4] + 1, P.t[5], false);
  lit(", \"format\": ");
  value(P.t[7] + 1, Q.t8, false);
  lit("}}");
  return host ? kHost : k;
}

// what the size pass keeps of a parsed line
template <class CP>
AVDB_HD lof::Entry entry_of(CP line, Parsed& Q, const Release& rel) {
  lof::Parsed& P = Q.b;
  lof::Entry E{0, 0, 0, P.flags};
  if (P.cls != lof::kEntry || (P.flags & AVDB_QC_LINE_HOST)) return E;
  const uint32_t json = line_json(line, Q, rel, [](uint32_t, uint32_t) {});
  const uint32_t alts = lof::count_alts(line, P);
  const uint32_t ref_n = P.t[3] - (P.t[2] + 1), alt_field = P.t[4] - (P.t[3] + 1);
  const uint64_t keys = uint64_t(alts) * (P.chrom_n + 1 + P.pos_n + 1 + ref_n + 1) + (alt_field - (alts - 1));
  if (json == kHost || keys > 0xFFFFFFFFull) {
    P.flags = E.flags = AVDB_QC_LINE_HOST;
    return E;
  }
  E.n_alts = alts;
  E.key_bytes = uint32_t(keys);
  E.json_len = json;
  return E;
}

// ---- K17a's write pass: one entry's keys, its rows' columns, its JSON ------------------------
// The keys of entry E through put(k, c), k < E.key_bytes, and the columns of its rows.  A host
// line's span is left blank and its rows all point to the span's start; so is the span of an
// entry whose columns do not describe the text.
template <class Put>
AVDB_HD void render_entry_keys(const uint8_t* text, uint64_t text_bytes, const lof::EntryRow& E, const lof::RowCols& R,
                               Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < E.key_bytes) put_any(k, c);
  };
  auto row = [&](uint32_t a, uint32_t off, uint32_t flags) {
    const uint64_t r = E.first_row + a;
    if (a >= E.alts || r >= R.n_rows) return;
    R.key_off[r] = E.key_base + (off < E.key_bytes ? off : E.key_bytes);
    R.json_off[r] = E.json_base;
    R.json_len[r] = E.json_len;
    R.line_start[r] = E.start;
    R.flags[r] = uint8_t(flags | (a == 0 ? AVDB_QC_ROW_FIRST : 0u));
  };
  bool done = false;
  if (!(E.flags & AVDB_QC_LINE_HOST) && E.start < text_bytes) {
    uint64_t len;
    bool nl;
    lof::line_at(text, text_bytes, E.start, &len, &nl);
    const uint8_t* line = text + E.start;
    const Parsed Q = parse_line(line, len, nl, false);
    if (Q.b.cls == lof::kEntry && !(Q.b.flags & AVDB_QC_LINE_HOST) && lof::count_alts(line, Q.b) == E.alts) {
      uint32_t end = 0;
      lof::entry_keys(line, Q.b, put, [&](uint32_t a, uint32_t off) {
        row(a, off, E.flags & AVDB_QC_PASS);
        end = off;
      });
      for (; end < E.key_bytes; ++end) put(end, uint32_t(' '));
      done = true;
    }
  }
  if (!done) {
    for (uint32_t k = 0; k < E.key_bytes; ++k) put(k, uint32_t(' '));
    for (uint32_t a = 0; a < E.alts; ++a) row(a, 0u, AVDB_QC_LINE_HOST | (E.flags & AVDB_QC_PASS));
  }
}

// the JSON of entry E through put(k, c), k < E.json_len; blank for a host line
template <class Put>
AVDB_HD void render_entry_json(const uint8_t* text, uint64_t text_bytes, const lof::EntryRow& E, const Release& rel,
                               Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < E.json_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(E.flags & AVDB_QC_LINE_HOST) && E.start < text_bytes) {
    uint64_t len;
    bool nl;
    lof::line_at(text, text_bytes, E.start, &len, &nl);
    const uint8_t* line = text + E.start;
    const Parsed Q = parse_line(line, len, nl, false);
    if (Q.b.cls == lof::kEntry && !(Q.b.flags & AVDB_QC_LINE_HOST)) {
      k = line_json(line, Q, rel, put);
      if (k == kHost) k = 0;
    }
  }
  for (; k < E.json_len; ++k) put(k, uint32_t(' '));
}

// ---- K17b: one line of the export ------------------------------------------------------
// the table as K17b reads it (avdb_qc_table): K16b's, the rows' flags and the release
struct Table {
  lof::Table t;
  const uint8_t* row_flags;
  Release rel;
};

struct UpdLine {
  uint32_t is_row;   // 1: a row (BAD and ROW_HOST rows included)
  uint32_t skipped;  // 1: in the table, but has QC values of this release already (no row; `row` is its hit)
  uint32_t missed;   // 1: its id is not in the table, counted `not_in_vcf` (no row)
  uint32_t pk_len, out_len, flags;
  int32_t row;       // the table row (-1: none)
  uint32_t lone_cr, coll;
};

using UpdRow = lof::UpdRow;

enum ColumnQc : uint32_t { kNoQc = 0, kHasQc = 1, kAskHost = 2 };

// The adsp_qc column [s, e) of an export line, the JSONB text as COPY writes it: does a key at depth
// 1 of its object equal the release?  One scan that tracks strings and brace / bracket depth; at
// depth 1 a string followed by ':' is a key.  NULL (absent, empty, \N) has none.  A column with a
// '\' in it or that does not begin with '{' is the host's (json.loads).
template <class CP>
AVDB_HD uint32_t column_has_release(CP line, uint32_t s, uint32_t e, const Release& rel) {
  const uint32_t n = e - s;
  if (n == 0 || (n == 2 && line[s] == '\\' && line[s + 1] == 'N')) return kNoQc;
  if (line[s] != '{') return kAskHost;
  for (uint32_t i = s; i < e; ++i)
    if (line[i] == '\\') return kAskHost;
  uint32_t depth = 0, found = 0;
  for (uint32_t i = s; i < e; ++i) {
    const uint32_t c = line[i];
    if (c == '"') {
      uint32_t j = i + 1;
      bool same = j + rel.n <= e;
      for (uint32_t m = 0; j < e && line[j] != '"'; ++j, ++m) same = same && m < rel.n && line[j] == rel.b[m];
      same = same && j - (i + 1) == rel.n;
      if (depth == 1 && same) {
        uint32_t q = j + 1;
        while (q < e && (line[q] == ' ' || line[q] == '\t' || line[q] == '\n' || line[q] == '\r')) ++q;
        found |= q < e && line[q] == ':';
      }
      i = j;  // the closing quote (or the column's end)
    } else if (c == '{' || c == '[') {
      ++depth;
    } else if (c == '}' || c == ']') {
      depth -= depth ? 1u : 0u;
    }
  }
  return found ? kHasQc : kNoQc;
}

// the bytes of the is_adsp_variant column: true, or \N
AVDB_HD uint32_t flag_len(bool pass) { return pass ? 4u : 2u; }

// One line of the export by K13's conventions (caddupd::scan_line) and the rule of load
// (update_from_qc_pvcf_file.py:45-53) and generate_update_values (:148).
template <class CP>
AVDB_HD UpdLine scan_export_line(CP line, uint64_t len64, bool nl, uint32_t contig_mask, bool update_existing,
                                 const Table& Q) {
  const lof::Table& T = Q.t;
  UpdLine L{0, 0, 0, 0, 0, 0, -1, 0, 0};
  uint32_t n = len64 < 0x7FFFFFFFull ? uint32_t(len64) : 0x7FFFFFFFu;
  if (nl && n && line[n - 1] == '\r') --n;
  uint32_t t[3] = {n, n, n};
  uint32_t nt = 0, nc = 0, col0 = n;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = line[i];
    if (c == '\t') {
      if (nt < 3) t[nt] = i;
      ++nt;
    } else {
      L.lone_cr += c == '\r';
      if (c == ':' && nt == 1) {
        if (!nc) col0 = i;
        ++nc;
      }
    }
  }
  if (nt < 1) return L;
  L.pk_len = t[0];
  if (caddupd::is_header(line, L.pk_len)) return L;
  const uint32_t m0 = t[0] + 1, m1 = t[1];
  const uint32_t lab = (nc ? col0 : m1) - m0;
  const uint32_t bit = exist::contig_bit(line + m0, lab);
  if (!((contig_mask >> bit) & 1u)) return L;
  if (nc != 3) {
    L.is_row = 1;
    L.flags = AVDB_QCUPD_BAD;
    return L;
  }
  const int32_t k = T.n_rows ? keyset::probe_text(T.keys, T.key_off, size_t(T.n_rows), T.tkey, T.tidx, T.mask, line + m0,
                                                  uint64_t(m1 - m0), &L.coll)
                             : -1;
  if (k < 0) {
    L.missed = 1;
    return L;
  }
  const uint64_t row = T.n_rows - 1 - uint64_t(k);
  L.row = int32_t(row);  // (a hit, whether or not a row comes of it)
  uint32_t host = 0;
  if (!update_existing && nt >= 2) {
    const uint32_t has = column_has_release(line, t[1] + 1, t[2], Q.rel);
    if (has == kHasQc) {
      L.skipped = 1;  // generate_update_values: 'update': updateExistingValues or not hasAdspQC
      return L;
    }
    host = has == kAskHost ? AVDB_QCUPD_ROW_HOST : 0u;
  }
  uint64_t js;
  uint32_t jn;
  lof::json_span(T, row, &js, &jn);
  const bool pass = Q.row_flags && (Q.row_flags[row] & AVDB_QC_PASS);
  const uint64_t out = uint64_t(L.pk_len) + 1 + 3 + lab + 1 + flag_len(pass) + 1 + jn + 1;
  L.is_row = 1;
  if (out > 0xFFFFFFFFull) {  // (no such row fits a slab)
    L.flags = AVDB_QCUPD_BAD;
    return L;
  }
  L.flags = host;
  L.out_len = uint32_t(out);
  return L;
}

// one row's text: pk<TAB>chr<label of the metaseq id><TAB>true|\N<TAB>json<LF>.  text(pos): the
// slab's byte at offset pos (0 outside the text); put(k, c) is called for k < row.out_len only.
template <class TextAt, class Put>
AVDB_HD void render_update_row(const UpdRow& row, const Table& Q, TextAt text, Put put_any) {
  const lof::Table& T = Q.t;
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < row.out_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(row.flags & AVDB_QCUPD_BAD) && row.row >= 0 && uint64_t(row.row) < T.n_rows) {
    for (uint32_t i = 0; i < row.pk_len; ++i) put(k++, text(row.start + i));
    put(k++, uint32_t('\t'));
    put(k++, uint32_t('c'));
    put(k++, uint32_t('h'));
    put(k++, uint32_t('r'));
    for (uint64_t p = row.start + row.pk_len + 1; k < row.out_len; ++p) {
      const uint32_t c = text(p);
      if (c == ':' || c == '\t' || c == '\n' || c == 0) break;
      put(k++, c);
    }
    put(k++, uint32_t('\t'));
    const char* f = Q.row_flags && (Q.row_flags[row.row] & AVDB_QC_PASS) ? "true" : "\\N";
    for (uint32_t i = 0; f[i]; ++i) put(k++, uint32_t(uint8_t(f[i])));
    put(k++, uint32_t('\t'));
    uint64_t js;
    uint32_t jn;
    lof::json_span(T, uint64_t(row.row), &js, &jn);
    for (uint32_t j = 0; j < jn; ++j) put(k++, uint32_t(T.json[js + j]));
    put(k++, uint32_t('\n'));
  }
  for (; k < row.out_len; ++k) put(k, uint32_t(' '));
}

}  // namespace qc
}  // namespace avdb
