// K16 — per-line and per-row code of the SnpEff LOF/NMD pass (Load/bin/load_snpeff_lof.py), shared
// by the kernels (avdb_lof.hip) and the library's host entries: K16a, the table of annotated alt
// alleles from the SnpEff VCF (lookup ids chrom:pos:ref:alt and one JSON text per line), and K16b,
// the update rows from an export of AnnotatedVDB.Variant
// (record_primary_key<TAB>metaseq_id<TAB>loss_of_function).  One definition, compiled for both
// sides, as avdb_caddupd.hpp is.
#pragma once

#include "avdb_caddupd.hpp"
#include "avdb_keyset.hpp"

namespace avdb {
namespace lof {

// ---- K16a: one line of the SnpEff VCF --------------------------------------------------
enum LineClass : uint32_t { kComment = 0, kUnannotated = 1, kNoValues = 2, kEntry = 3 };

// a line as load_annotation sees it: decoded, rstrip()ped, its first eight fields
struct Parsed {
  uint32_t cls;     // LineClass
  uint32_t flags;   // AVDB_LOF_LINE_* (an entry's)
  uint32_t n;       // the stripped length
  uint32_t t[8];    // the first eight tabs (n where the line has fewer)
  uint32_t lone_cr;
  uint32_t has_lof, lof_s, lof_e;  // the value of the last LOF= item of INFO
  uint32_t has_nmd, nmd_s, nmd_e;
  uint32_t chrom_s, chrom_n;  // the key's chromosome text: CHROM without 'chr', MT as M
  uint32_t pos_s, pos_n;      // POS without its leading zeros
};

// what the size pass keeps of an entry (a line that yields table rows)
struct Entry {
  uint32_t n_alts, key_bytes, json_len, flags;
};

AVDB_HD bool strips(uint32_t c) {  // ASCII bytes str.rstrip() removes
  return c == ' ' || (c >= 0x09u && c <= 0x0Du) || (c >= 0x1Cu && c <= 0x1Fu);
}

AVDB_HD uint32_t lower(uint32_t c) { return c >= 'A' && c <= 'Z' ? c + 32u : c; }

// is p[0, n), case-insensitively, inf, nan or infinity (what float() takes among letters)
template <class CP>
AVDB_HD bool is_float_word(CP p, uint32_t n) {
  const char* w = n == 3 ? (lower(p[0]) == 'i' ? "inf" : "nan") : n == 8 ? "infinity" : nullptr;
  if (!w) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (lower(p[i]) != uint32_t(uint8_t(w[i]))) return false;
  return true;
}

// a byte that can stand in a text to_numeric turns into a number
AVDB_HD bool numberish(uint32_t c) {
  const uint32_t l = lower(c);
  return (c >= '0' && c <= '9') || c == '_' || c == '.' || c == '+' || c == '-' || strips(c) || l == 'e' || l == 'n' ||
         l == 'a' || l == 'i' || l == 'f' || l == 't' || l == 'y';
}

// REF or the whole ALT field: ASCII letters, ',', '*', '.' only, and no float word
template <class CP>
AVDB_HD bool allele_field_ok(CP p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = p[i], l = lower(c);
    if (!((l >= 'a' && l <= 'z') || c == ',' || c == '*' || c == '.')) return false;
  }
  return !is_float_word(p, n);
}

// the bytes of a LOF / NMD value json.dumps and parse_entry leave as they are
AVDB_HD bool value_byte_ok(uint32_t c) { return c >= 0x20u && c < 0x80u && c != '\\' && c != '#' && c != '"'; }

constexpr uint32_t kMaxDigits = 4000;  // int() of a longer digit string raises

// The JSON of one value, parse_annotation_string's list as json.dumps renders it:
// [{"gene_symbol": s, "gene_id": s, "num_transcripts": int, "fraction_affected_transcripts": float}, ...]
// put(k, c): byte k.  Returns the length; 0: a value outside the device subset.
template <class CP, class Put>
AVDB_HD uint32_t value_json(CP line, uint32_t vs, uint32_t ve, Put put) {
  const char k0[] = "{\"gene_symbol\": \"", k1[] = "\", \"gene_id\": \"", k2[] = "\", \"num_transcripts\": ",
             k3[] = ", \"fraction_affected_transcripts\": ";
  uint32_t k = 0;
  auto lit = [&](const char* s) {
    for (uint32_t i = 0; s[i]; ++i) put(k++, uint32_t(uint8_t(s[i])));
  };
  put(k++, uint32_t('['));
  uint32_t g = vs;
  for (bool first = true;; first = false) {
    uint32_t ge = g;  // the group [g, ge)
    while (ge < ve && line[ge] != ',') ++ge;
    uint32_t ps[4], pe[4], np = 0, at = g;
    for (uint32_t i = g; i <= ge; ++i)
      if (i == ge || line[i] == '|') {
        if (np < 4) {
          ps[np] = at;
          pe[np] = i;
        }
        ++np;
        at = i + 1;
      }
    if (np < 4) return 0;  // values[3] raises IndexError
    if (!first) {
      put(k++, uint32_t(','));
      put(k++, uint32_t(' '));
    }
    for (uint32_t part = 0; part < 2; ++part) {
      lit(part ? k1 : k0);
      for (uint32_t i = ps[part]; i < pe[part]; ++i) {
        const uint32_t c = line[i];
        if (!value_byte_ok(c)) return 0;
        if (c != '(' && c != ')') put(k++, c);
      }
    }
    for (uint32_t part = 2; part < 4; ++part) {  // parentheses at either end only
      while (ps[part] < pe[part] && (line[ps[part]] == '(' || line[ps[part]] == ')')) ++ps[part];
      while (pe[part] > ps[part] && (line[pe[part] - 1] == '(' || line[pe[part] - 1] == ')')) --pe[part];
    }
    lit(k2);
    uint32_t d = ps[2];
    if (d >= pe[2] || pe[2] - d > kMaxDigits) return 0;
    for (uint32_t i = d; i < pe[2]; ++i)
      if (!cadd::is_digit(line[i])) return 0;
    while (d + 1 < pe[2] && line[d] == '0') ++d;
    for (; d < pe[2]; ++d) put(k++, uint32_t(line[d]));
    lit(k3);
    const uint32_t f = caddupd::score_text(line + ps[3], pe[3] - ps[3], [&](uint32_t j, uint32_t c) { put(k + j, c); });
    if (!f) return 0;
    k += f;
    put(k++, uint32_t('}'));
    for (uint32_t i = pe[3]; i < ge; ++i)  // parts beyond the fourth are ignored, their bytes are not
      if (!value_byte_ok(line[i])) return 0;
    if (ge >= ve) break;
    g = ge + 1;
  }
  put(k++, uint32_t(']'));
  return k;
}

// json.dumps({'LOF': [...], 'NMD': [...]}) of a parsed entry; 0: outside the device subset
template <class CP, class Put>
AVDB_HD uint32_t line_json(CP line, const Parsed& P, Put put) {
  uint32_t k = 0;
  auto lit = [&](const char* s) {
    for (uint32_t i = 0; s[i]; ++i) put(k++, uint32_t(uint8_t(s[i])));
  };
  put(k++, uint32_t('{'));
  if (P.has_lof) {
    lit("\"LOF\": ");
    const uint32_t a = value_json(line, P.lof_s, P.lof_e, [&](uint32_t j, uint32_t c) { put(k + j, c); });
    if (!a) return 0;
    k += a;
  }
  if (P.has_nmd) {
    if (P.has_lof) lit(", ");
    lit("\"NMD\": ");
    const uint32_t a = value_json(line, P.nmd_s, P.nmd_e, [&](uint32_t j, uint32_t c) { put(k + j, c); });
    if (!a) return 0;
    k += a;
  }
  put(k++, uint32_t('}'));
  return k;
}

// One line of the VCF (its len bytes, '\n' excluded; nl: a '\n' follows) by the rule of
// load_annotation (load_snpeff_lof.py:250-288), VcfEntryParser.parse_entry and get_variant.
template <class CP>
AVDB_HD Parsed parse_line(CP line, uint64_t len64, bool nl) {
  Parsed P{};
  uint32_t n = len64 < 0x7FFFFFFFull ? uint32_t(len64) : 0x7FFFFFFFu;  // (lengths are u32: a longer line is cut)
  if (nl && n && line[n - 1] == '\r') --n;                              // "\r\n" is one line end
  while (n && strips(line[n - 1])) --n;                                 // line.rstrip()
  P.n = n;
  for (uint32_t i = 0; i < 8; ++i) P.t[i] = n;
  if (n && line[0] == '#') {
    P.cls = kComment;
    return P;
  }
  uint32_t nt = 0;
  bool hi = false, hit = false;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = line[i];
    if (c == '\t') {
      if (nt < 8) P.t[nt] = i;
      ++nt;
    } else if (c == ';') {  // ';LOF=' or ';NMD=' anywhere in the line
      if (i + 4 < n && line[i + 4] == '=') {
        const uint32_t a = line[i + 1], b = line[i + 2], d = line[i + 3];
        hit = hit || (a == 'L' && b == 'O' && d == 'F') || (a == 'N' && b == 'M' && d == 'D');
      }
    } else {
      P.lone_cr += c == '\r';
      hi = hi || c >= 0x80u;
    }
  }
  if (!hit) {
    P.cls = kUnannotated;
    return P;
  }
  P.cls = kEntry;
  if (nt < 7) {  // fewer fields than the header: parse_entry raises IndexError
    P.flags = AVDB_LOF_LINE_HOST | AVDB_LOF_LINE_BAD;
    return P;
  }
  P.flags = AVDB_LOF_LINE_HOST;  // until every check has passed
  if (hi) return P;
  // CHROM: an optional 'chr' and one of the 25 labels, or MT
  uint32_t cs = 0, cn = P.t[0];
  if (cn == 2 && line[0] == 'M' && line[1] == 'T') {
    cn = 1;
  } else {
    if (cn > 3 && line[0] == 'c' && line[1] == 'h' && line[2] == 'r') {
      cs = 3;
      cn -= 3;
    }
    if (exist::contig_bit(line + cs, cn) == exist::kOtherBit) return P;
  }
  P.chrom_s = cs;
  P.chrom_n = cn;
  // POS: plain digits
  uint32_t ps = P.t[0] + 1;
  const uint32_t pe = P.t[1];
  if (ps >= pe || pe - ps > kMaxDigits) return P;
  for (uint32_t i = ps; i < pe; ++i)
    if (!cadd::is_digit(line[i])) return P;
  while (ps + 1 < pe && line[ps] == '0') ++ps;
  P.pos_s = ps;
  P.pos_n = pe - ps;
  // ID: '.' or a text to_numeric leaves a string (the reference dies in id.startswith otherwise)
  const uint32_t is = P.t[1] + 1, ie = P.t[2];
  bool text_id = false;
  for (uint32_t i = is; i < ie && !text_id; ++i) text_id = !numberish(line[i]);
  if (!text_id && !(ie - is == 1 && line[is] == '.')) return P;
  // REF and ALT
  const uint32_t rs = P.t[2] + 1, re = P.t[3], as = P.t[3] + 1, ae = P.t[4];
  if (!allele_field_ok(line + rs, re - rs) || !allele_field_ok(line + as, ae - as)) return P;
  // INFO by key: the last item of a key wins; an item without '=' is a flag (True)
  const uint32_t fs = P.t[6] + 1, fe = P.t[7];
  bool lof_flag = false, nmd_flag = false, any_eq = false;
  for (uint32_t a = fs; a <= fe;) {
    uint32_t b = a;
    while (b < fe && line[b] != ';') {
      any_eq = any_eq || line[b] == '=';
      ++b;
    }
    if (b - a >= 3 && (b - a == 3 || line[a + 3] == '=')) {
      const bool flag = b - a == 3;
      if (line[a] == 'L' && line[a + 1] == 'O' && line[a + 2] == 'F') {
        P.has_lof = 1;
        lof_flag = flag;
        P.lof_s = flag ? b : a + 4;
        P.lof_e = b;
      } else if (line[a] == 'N' && line[a + 1] == 'M' && line[a + 2] == 'D') {
        P.has_nmd = 1;
        nmd_flag = flag;
        P.nmd_s = flag ? b : a + 4;
        P.nmd_e = b;
      }
    }
    a = b + 1;
  }
  if (!P.has_lof && !P.has_nmd) {
    if (!any_eq) return P;  // an INFO that may be a number: parse_entry raises
    P.cls = kNoValues;
    P.flags = 0;
    return P;
  }
  if (lof_flag || nmd_flag) return P;  // parse_annotation_string(True) raises
  P.flags = 0;
  return P;
}

// the alleles of the ALT field: alt.split(',')
template <class CP>
AVDB_HD uint32_t count_alts(CP line, const Parsed& P) {
  uint32_t k = 1;
  for (uint32_t i = P.t[3] + 1; i < P.t[4]; ++i) k += line[i] == ',';
  return k;
}

// what the size pass keeps of a parsed line
template <class CP>
AVDB_HD Entry entry_of(CP line, Parsed& P) {
  Entry E{0, 0, 0, P.flags};
  if (P.cls != kEntry || P.flags) return E;
  const uint32_t json = line_json(line, P, [](uint32_t, uint32_t) {});
  if (!json) {
    P.flags = E.flags = AVDB_LOF_LINE_HOST;
    return E;
  }
  const uint32_t alts = count_alts(line, P);
  const uint32_t ref_n = P.t[3] - (P.t[2] + 1), alt_field = P.t[4] - (P.t[3] + 1);
  const uint64_t keys = uint64_t(alts) * (P.chrom_n + 1 + P.pos_n + 1 + ref_n + 1) + (alt_field - (alts - 1));
  if (keys > 0xFFFFFFFFull) {
    P.flags = E.flags = AVDB_LOF_LINE_HOST;
    return E;
  }
  E.n_alts = alts;
  E.key_bytes = uint32_t(keys);
  E.json_len = json;
  return E;
}

// the keys of an entry, chrom:pos:ref:alt_k back to back: put(k, c) byte k of them; row(a, off):
// key a starts at byte off (called for a = 0 .. n_alts, the last one with the total)
template <class CP, class Put, class RowAt>
AVDB_HD void entry_keys(CP line, const Parsed& P, Put put, RowAt row) {
  uint32_t k = 0, a = 0;
  const uint32_t rs = P.t[2] + 1, re = P.t[3];
  uint32_t as = P.t[3] + 1;
  const uint32_t ae = P.t[4];
  for (;;) {
    row(a++, k);
    for (uint32_t i = 0; i < P.chrom_n; ++i) put(k++, uint32_t(line[P.chrom_s + i]));  // (MT: its first byte)
    put(k++, uint32_t(':'));
    for (uint32_t i = 0; i < P.pos_n; ++i) put(k++, uint32_t(line[P.pos_s + i]));
    put(k++, uint32_t(':'));
    for (uint32_t i = rs; i < re; ++i) put(k++, uint32_t(line[i]));
    put(k++, uint32_t(':'));
    while (as < ae && line[as] != ',') put(k++, uint32_t(line[as++]));
    if (as >= ae) break;
    ++as;
  }
  row(a, k);
}

// ---- K16a's write pass: one entry's keys, its rows' columns, its JSON ------------------------
// an entry as the write pass reads it: the size pass's columns (possibly patched by the caller)
// and where its rows, keys and JSON begin
struct EntryRow {
  uint64_t start;
  uint32_t alts, key_bytes, json_len, flags;
  uint64_t first_row, key_base, json_base;
};

struct RowCols {  // per row, n_rows entries
  uint64_t* key_off;
  uint64_t* json_off;
  uint32_t* json_len;
  uint64_t* line_start;
  uint8_t* flags;
  uint64_t n_rows;
};

// the line that starts at `start`: its length without the '\n', and whether one follows
AVDB_HD void line_at(const uint8_t* text, uint64_t text_bytes, uint64_t start, uint64_t* len, bool* nl) {
  uint64_t e = start < text_bytes ? start : text_bytes;
  while (e < text_bytes && text[e] != '\n') ++e;
  *len = e - (start < text_bytes ? start : text_bytes);
  *nl = e < text_bytes;
}

// The keys of entry E through put(k, c), k < E.key_bytes, and the columns of its rows.  A host
// line's span is left blank and its rows all point to the span's start; so is the span of an
// entry whose columns do not describe the text.
template <class Put>
AVDB_HD void render_entry_keys(const uint8_t* text, uint64_t text_bytes, const EntryRow& E, const RowCols& R,
                               Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < E.key_bytes) put_any(k, c);
  };
  auto row = [&](uint32_t a, uint32_t off, uint32_t host) {
    const uint64_t r = E.first_row + a;
    if (a >= E.alts || r >= R.n_rows) return;
    R.key_off[r] = E.key_base + (off < E.key_bytes ? off : E.key_bytes);
    R.json_off[r] = E.json_base;
    R.json_len[r] = E.json_len;
    R.line_start[r] = E.start;
    R.flags[r] = uint8_t(host | (a == 0 ? AVDB_LOF_ROW_FIRST : 0u));
  };
  bool done = false;
  if (!(E.flags & AVDB_LOF_LINE_HOST) && E.start < text_bytes) {
    uint64_t len;
    bool nl;
    line_at(text, text_bytes, E.start, &len, &nl);
    const uint8_t* line = text + E.start;
    const Parsed P = parse_line(line, len, nl);
    if (P.cls == kEntry && !P.flags && count_alts(line, P) == E.alts) {
      uint32_t end = 0;
      entry_keys(line, P, put, [&](uint32_t a, uint32_t off) {
        row(a, off, 0u);
        end = off;
      });
      for (; end < E.key_bytes; ++end) put(end, uint32_t(' '));
      done = true;
    }
  }
  if (!done) {
    for (uint32_t k = 0; k < E.key_bytes; ++k) put(k, uint32_t(' '));
    for (uint32_t a = 0; a < E.alts; ++a) row(a, 0u, AVDB_LOF_LINE_HOST);
  }
}

// the JSON of entry E through put(k, c), k < E.json_len; blank for a host line
template <class Put>
AVDB_HD void render_entry_json(const uint8_t* text, uint64_t text_bytes, const EntryRow& E, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < E.json_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(E.flags & AVDB_LOF_LINE_HOST) && E.start < text_bytes) {
    uint64_t len;
    bool nl;
    line_at(text, text_bytes, E.start, &len, &nl);
    const uint8_t* line = text + E.start;
    const Parsed P = parse_line(line, len, nl);
    if (P.cls == kEntry && !P.flags) k = line_json(line, P, put);
  }
  for (; k < E.json_len; ++k) put(k, uint32_t(' '));
}

// ---- K16b: one line of the export ------------------------------------------------------
// the table as K16b reads it (avdb_lof_table): the keys in reverse row order, so that K6's
// first-of-equal-keys is the last annotated record of an id
struct Table {
  uint64_t n_rows;
  const uint8_t* keys;
  const uint64_t* key_off;
  const unsigned long long* tkey;
  const uint32_t* tidx;
  uint64_t mask;
  const uint8_t* json;
  uint64_t json_bytes;
  const uint64_t* json_off;
  const uint32_t* json_len;
  uint8_t* hit;
};

struct UpdLine {
  uint32_t is_row;   // 1: a row (BAD rows included)
  uint32_t skipped;  // 1: annotated, but has values already: counted `skipped` (no row; `row` is its hit)
  uint32_t missed;   // 1: its id is not in the table, counted `not_annotated` (no row)
  uint32_t pk_len, out_len, flags;
  int32_t row;       // the table row (-1: none)
  uint32_t lone_cr, coll;
};

struct UpdRow {
  uint64_t start;
  uint32_t pk_len, out_len, flags;
  int32_t row;
};

// the span of table row t's JSON, clamped to the blob
AVDB_HD void json_span(const Table& T, uint64_t t, uint64_t* s, uint32_t* n) {
  uint64_t a = T.json_off[t], l = T.json_len[t];
  if (a > T.json_bytes) a = T.json_bytes;
  if (l > T.json_bytes - a) l = T.json_bytes - a;
  *s = a;
  *n = uint32_t(l);
}

// One line of the export by K13's conventions (caddupd::scan_line) and the rule of
// generate_update_values (load_snpeff_lof.py:136-173).
template <class CP>
AVDB_HD UpdLine scan_export_line(CP line, uint64_t len64, bool nl, uint32_t contig_mask, bool update_existing,
                                 const Table& T) {
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
    L.flags = AVDB_LOFUPD_BAD;
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
  if (!update_existing && nt >= 2) {  // loss_of_function: NULL when absent, empty or \N
    const uint32_t s0 = t[1] + 1, sl = t[2] - s0;
    if (!(sl == 0 || (sl == 2 && line[s0] == '\\' && line[s0 + 1] == 'N'))) {
      L.skipped = 1;  // generate_update_values: existingValues is not None -> {'update': False}
      return L;
    }
  }
  uint64_t js;
  uint32_t jn;
  json_span(T, row, &js, &jn);
  const uint64_t out = uint64_t(L.pk_len) + 1 + 3 + lab + 1 + jn + 1;
  L.is_row = 1;
  if (out > 0xFFFFFFFFull) {  // (no such row fits a slab)
    L.flags = AVDB_LOFUPD_BAD;
    return L;
  }
  L.out_len = uint32_t(out);
  return L;
}

// one row's text: pk<TAB>chr<label of the metaseq id><TAB>json<LF>.  text(pos): the slab's byte
// at offset pos (0 outside the text); put(k, c) is called for k < row.out_len only.
template <class TextAt, class Put>
AVDB_HD void render_update_row(const UpdRow& row, const Table& T, TextAt text, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < row.out_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(row.flags & AVDB_LOFUPD_BAD) && row.row >= 0 && uint64_t(row.row) < T.n_rows) {
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
    uint64_t js;
    uint32_t jn;
    json_span(T, uint64_t(row.row), &js, &jn);
    for (uint32_t j = 0; j < jn; ++j) put(k++, uint32_t(T.json[js + j]));
    put(k++, uint32_t('\n'));
  }
  for (; k < row.out_len; ++k) put(k, uint32_t(' '));
}

}  // namespace lof
}  // namespace avdb
