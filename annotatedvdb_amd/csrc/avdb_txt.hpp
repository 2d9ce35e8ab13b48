// K19 — per-line and per-row code of the generic annotation update
// (Load/bin/update_variant_annotation.py on TextVariantLoader), shared by the kernels
// (avdb_txt.hip) and the library's host entries: a tab-delimited file whose header names the
// columns, one of them `variant`.  K19a, the table of the file's data lines (the looked-up id as
// key, the line's update values rendered once); K19b, the update rows from an export of
// AnnotatedVDB.Variant (record_primary_key<TAB>metaseq_id<TAB>ref_snp_id); K19c, the update rows of
// a file whose `variant` column holds primary keys, which needs neither.  One definition, compiled
// for both sides, as avdb_lof.hpp is.
#pragma once

#include "avdb_lof.hpp"

namespace avdb {
namespace txt {

// what the host read from the header (csv's own parse of it)
struct Shape {
  uint32_t skip_lines;  // the slab's lines up to and including the header
  uint32_t n_fields;    // the header's fields, 2 .. AVDB_TXT_MAX_FIELDS
  uint32_t id_col;      // the field named `variant`: taken out of the tail, the source of the chromosome
  uint32_t key_col;     // the field looked up (id_col; `ref_snp_id` for refSNP ids): the table's key
};

AVDB_HD const char* shape_error(const Shape& S) {
  if (S.n_fields < 2 || S.n_fields > AVDB_TXT_MAX_FIELDS) return "n_fields out of range (2 .. AVDB_TXT_MAX_FIELDS)";
  if (S.id_col >= S.n_fields) return "id_col out of range";
  if (S.key_col >= S.n_fields) return "key_col out of range";
  return nullptr;
}

// a line as csv.DictReader(fh, delimiter='\t') and __buffer_update_values see it
struct Line {
  uint32_t data;          // 1: a data line (0: the header and what precedes it, an empty line)
  uint32_t flags;         // AVDB_TXT_LINE_HOST, AVDB_TXT_LINE_BAD
  uint32_t n;             // the length without the line end
  uint32_t id_s, id_n;    // the `variant` field
  uint32_t key_s, key_n;  // the looked-up field
  uint32_t lab_n;         // the id up to its first ':' (id_n when it has none)
  uint32_t colon;         // 1: the id has a ':'
  uint32_t tail_len;      // the update values: n_fields - 1 fields, NULL and missing ones as \N
  uint32_t lone_cr;
};

template <class CP>
AVDB_HD bool is_null_word(CP p, uint32_t n) {
  return n == 4 && p[0] == 'N' && p[1] == 'U' && p[2] == 'L' && p[3] == 'L';
}

// One line of the file (its len bytes, '\n' excluded; nl: a '\n' follows).  past_header: the
// line comes after the header.  Outside the device subset (HOST): a field that starts with '"'
// (csv quoting), a byte above 0x7F (text-mode decoding), a field that is exactly \N (the row
// text cannot tell it from NULL); BAD as well: a row without its `variant` or looked-up field,
// or with an empty looked-up field.
template <class CP>
AVDB_HD Line parse_line(CP line, uint64_t len64, bool nl, bool past_header, const Shape& S) {
  Line L{};
  uint32_t n = len64 < 0x7FFFFFFFull ? uint32_t(len64) : 0x7FFFFFFFu;  // (lengths are u32: a longer line is cut)
  if (nl && n && line[n - 1] == '\r') --n;                              // "\r\n" is one line end
  L.n = n;
  if (!past_header || n == 0) return L;  // csv skips a row without fields
  L.data = 1;
  uint32_t f = 0, fs = 0, tail = 0;
  bool host = false, have_id = false, have_key = false;
  for (uint32_t i = 0; i <= n; ++i) {
    if (i < n) {
      const uint32_t c = line[i];
      if (c != '\t') {
        L.lone_cr += c == '\r';
        host = host || c >= 0x80u;
        continue;
      }
    }
    const uint32_t fn = i - fs;  // field f is [fs, i)
    host = host || (fn && line[fs] == '"') || (fn == 2 && line[fs] == '\\' && line[fs + 1] == 'N');
    if (f == S.id_col) {
      L.id_s = fs;
      L.id_n = fn;
      have_id = true;
    } else if (f < S.n_fields) {
      tail += is_null_word(line + fs, fn) ? 2u : fn;
    }
    if (f == S.key_col) {
      L.key_s = fs;
      L.key_n = fn;
      have_key = true;
    }
    ++f;
    fs = i + 1;
  }
  if (f < S.n_fields) tail += 2u * (S.n_fields - f - (S.id_col >= f ? 1u : 0u));  // restval=None
  L.tail_len = tail + (S.n_fields - 2);
  L.lab_n = L.id_n;
  for (uint32_t i = 0; i < L.id_n; ++i)
    if (line[L.id_s + i] == ':') {
      L.lab_n = i;
      L.colon = 1;
      break;
    }
  if (host) L.flags = AVDB_TXT_LINE_HOST;
  if (!have_id || !have_key || L.key_n == 0) L.flags = AVDB_TXT_LINE_HOST | AVDB_TXT_LINE_BAD;
  return L;
}

// the update values of a parsed line through put(k, c); returns their length (L.tail_len)
template <class CP, class Put>
AVDB_HD uint32_t render_tail(CP line, const Line& L, const Shape& S, Put put) {
  uint32_t k = 0, f = 0, fs = 0;
  bool first = true;
  auto null = [&]() {
    put(k++, uint32_t('\\'));
    put(k++, uint32_t('N'));
  };
  auto sep = [&]() {
    if (!first) put(k++, uint32_t('\t'));
    first = false;
  };
  for (uint32_t i = 0; i <= L.n && f < S.n_fields; ++i) {
    if (i < L.n && line[i] != '\t') continue;
    if (f != S.id_col) {
      sep();
      if (is_null_word(line + fs, i - fs)) {
        null();
      } else {
        for (uint32_t j = fs; j < i; ++j) put(k++, uint32_t(line[j]));
      }
    }
    ++f;
    fs = i + 1;
  }
  for (; f < S.n_fields; ++f)
    if (f != S.id_col) {
      sep();
      null();
    }
  return k;
}

// the line that starts at `start` as the write passes' host forms read it: f(line, len, nl, have)
template <class F>
AVDB_HD void with_line_at(const uint8_t* text, uint64_t text_bytes, uint64_t start, F f) {
  uint64_t len;
  bool nl;
  lof::line_at(text, text_bytes, start, &len, &nl);
  f(text + (start < text_bytes ? start : text_bytes), len, nl, start < text_bytes);
}

// ---- K19a: a table row's key and body -------------------------------------------------------
// A row's body is <label><TAB><tail>: the id up to its first ':' when it has one (the row's
// chromosome is chr<label>), nothing when it has none (AVDB_TXT_ROW_PK_CHROM: the chromosome comes
// from the primary key).
AVDB_HD uint32_t body_len(const Line& L) { return (L.colon ? L.lab_n : 0u) + 1u + L.tail_len; }

// The key of entry E through put(k, c), k < E.key_bytes, and the columns of its row.  A host
// line's span is left blank; so is the span of an entry whose columns do not describe the text.
// (line: the bytes at E.start, len of them up to the line end, nl: a '\n' follows; have: E.start lies in the text)
template <class CP, class Put>
AVDB_HD void render_entry_key(CP line, uint64_t len, bool nl, bool have, const lof::EntryRow& E, const lof::RowCols& R,
                              const Shape& S, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < E.key_bytes) put_any(k, c);
  };
  uint32_t k = 0, bits = AVDB_TXT_LINE_HOST;
  if (!(E.flags & AVDB_TXT_LINE_HOST) && have) {
    const Line L = parse_line(line, len, nl, true, S);
    if (L.data && !L.flags) {
      for (; k < L.key_n; ++k) put(k, uint32_t(line[L.key_s + k]));
      bits = L.colon ? 0u : AVDB_TXT_ROW_PK_CHROM;
    }
  }
  for (; k < E.key_bytes; ++k) put(k, uint32_t(' '));
  if (E.alts && E.first_row < R.n_rows) {  // (one row per entry)
    const uint64_t r = E.first_row;
    R.key_off[r] = E.key_base;
    R.json_off[r] = E.json_base;
    R.json_len[r] = E.json_len;
    R.line_start[r] = E.start;
    R.flags[r] = uint8_t(bits);
  }
}

// the body of entry E through put(k, c), k < E.json_len; blank for a host line
template <class CP, class Put>
AVDB_HD void render_entry_body(CP line, uint64_t len, bool nl, bool have, const lof::EntryRow& E, const Shape& S,
                               Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < E.json_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(E.flags & AVDB_TXT_LINE_HOST) && have) {
    const Line L = parse_line(line, len, nl, true, S);
    if (L.data && !L.flags) {
      if (L.colon)
        for (; k < L.lab_n; ++k) put(k, uint32_t(line[L.id_s + k]));
      put(k++, uint32_t('\t'));
      k += render_tail(line, L, S, [&](uint32_t j, uint32_t c) { put(k + j, c); });
    }
  }
  for (; k < E.json_len; ++k) put(k, uint32_t(' '));
}

// ---- K19b: one line of the export -------------------------------------------------------------
// the table as K19b reads it (avdb_txt_table): lof::Table's members and the rows' flags
struct Table {
  lof::Table t;
  const uint8_t* flags;
};

struct UpdLine {
  uint32_t is_row;  // 1: a row (BAD rows included)
  uint32_t missed;  // 1: its id is not in the table, counted `not_in_file` (no row)
  uint32_t pk_len, out_len, flags;
  int32_t row;      // the table row (-1: none)
  uint32_t lone_cr, coll;
};

// the primary key up to its first ':' (all of it when it has none)
template <class CP>
AVDB_HD uint32_t pk_label_len(CP pk, uint32_t pk_len) {
  for (uint32_t i = 0; i < pk_len; ++i)
    if (pk[i] == ':') return i;
  return pk_len;
}

constexpr uint32_t kTrueLen = 5;  // <TAB>true

// One line of the export by K13's conventions (caddupd::scan_line): the header line, a line of
// fewer than two fields and a line outside the contig mask are skipped; a metaseq id without its
// four parts is a BAD row; field key_col (1: metaseq_id, 2: ref_snp_id) is probed in the table.
template <class CP>
AVDB_HD UpdLine scan_export_line(CP line, uint64_t len64, bool nl, uint32_t contig_mask, uint32_t key_col, bool adsp,
                                 const Table& T) {
  UpdLine L{0, 0, 0, 0, 0, -1, 0, 0};
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
  const uint32_t bit = exist::contig_bit(line + m0, (nc ? col0 : m1) - m0);
  if (!((contig_mask >> bit) & 1u)) return L;
  if (nc != 3) {
    L.is_row = 1;
    L.flags = AVDB_TXTUPD_BAD;
    return L;
  }
  uint32_t k0 = m0, k1 = m1;
  if (key_col == 2) {  // ref_snp_id: none when absent, empty or \N
    k0 = nt >= 2 ? t[1] + 1 : n;
    k1 = nt >= 2 ? t[2] : n;
    if (k1 - k0 == 2 && line[k0] == '\\' && line[k0 + 1] == 'N') k1 = k0;
  }
  const lof::Table& K = T.t;
  const int32_t k = K.n_rows && k1 > k0 ? keyset::probe_text(K.keys, K.key_off, size_t(K.n_rows), K.tkey, K.tidx, K.mask,
                                                             line + k0, uint64_t(k1 - k0), &L.coll)
                                        : -1;
  if (k < 0) {
    L.missed = 1;
    return L;
  }
  const uint64_t row = K.n_rows - 1 - uint64_t(k);
  L.row = int32_t(row);
  uint64_t bs;
  uint32_t bn;
  lof::json_span(K, row, &bs, &bn);
  const uint32_t f = T.flags[row];
  const uint64_t out = uint64_t(L.pk_len) + 1 + 3 + ((f & AVDB_TXT_ROW_PK_CHROM) ? pk_label_len(line, L.pk_len) : 0u) + bn +
                       (adsp ? kTrueLen : 0u) + 1;
  L.is_row = 1;
  if (out > 0xFFFFFFFFull) {  // (no such row fits a slab)
    L.flags = AVDB_TXTUPD_BAD;
    return L;
  }
  L.flags = f & AVDB_TXT_LINE_HOST ? AVDB_TXTUPD_TABLE_HOST : 0u;
  L.out_len = uint32_t(out);
  return L;
}

template <class Put>
AVDB_HD uint32_t put_true(uint32_t k, Put put) {
  const char w[] = "\ttrue";
  for (uint32_t i = 0; i < kTrueLen; ++i) put(k + i, uint32_t(uint8_t(w[i])));
  return kTrueLen;
}

// one row's text: pk<TAB>chr<label><body from its TAB on>[<TAB>true]<LF>.  text(pos): the slab's
// byte at offset pos (0 outside the text); put(k, c) is called for k < row.out_len only.
template <class TextAt, class Put>
AVDB_HD void render_update_row(const lof::UpdRow& row, const Table& T, bool adsp, TextAt text, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < row.out_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(row.flags & AVDB_TXTUPD_BAD) && row.row >= 0 && uint64_t(row.row) < T.t.n_rows) {
    for (uint32_t i = 0; i < row.pk_len; ++i) put(k++, text(row.start + i));
    put(k++, uint32_t('\t'));
    put(k++, uint32_t('c'));
    put(k++, uint32_t('h'));
    put(k++, uint32_t('r'));
    if (T.flags[row.row] & AVDB_TXT_ROW_PK_CHROM)
      for (uint32_t i = 0; i < row.pk_len; ++i) {
        const uint32_t c = text(row.start + i);
        if (c == ':') break;
        put(k++, c);
      }
    uint64_t bs;
    uint32_t bn;
    lof::json_span(T.t, uint64_t(row.row), &bs, &bn);
    for (uint32_t j = 0; j < bn; ++j) put(k++, uint32_t(T.t.json[bs + j]));
    if (adsp) k += put_true(k, put);
    put(k++, uint32_t('\n'));
  }
  for (; k < row.out_len; ++k) put(k, uint32_t(' '));
}

// ---- K19c: a file of primary keys ---------------------------------------------------------------
// the length of a data line's row pk<TAB>chr<label><TAB>tail[<TAB>true]<LF>; 0: a host line, or none fits u32
AVDB_HD uint32_t direct_len(const Line& L, bool adsp) {
  if (!L.data || L.flags) return 0;
  const uint64_t out = uint64_t(L.id_n) + 1 + 3 + L.lab_n + 1 + L.tail_len + (adsp ? kTrueLen : 0u) + 1;
  return out > 0xFFFFFFFFull ? 0u : uint32_t(out);
}

// the row of the data line at `start` through put(k, c), k < out_len; blank when the line is
// not what out_len was counted for (a host line's span is the caller's)
template <class CP, class Put>
AVDB_HD void render_direct_row(CP line, uint64_t len, bool nl, bool have, uint32_t out_len, uint32_t flags,
                               const Shape& S, bool adsp, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < out_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(flags & AVDB_TXT_LINE_HOST) && have) {
    const Line L = parse_line(line, len, nl, true, S);
    if (direct_len(L, adsp) == out_len && out_len) {
      for (uint32_t i = 0; i < L.id_n; ++i) put(k++, uint32_t(line[L.id_s + i]));
      put(k++, uint32_t('\t'));
      put(k++, uint32_t('c'));
      put(k++, uint32_t('h'));
      put(k++, uint32_t('r'));
      for (uint32_t i = 0; i < L.lab_n; ++i) put(k++, uint32_t(line[L.id_s + i]));
      put(k++, uint32_t('\t'));
      k += render_tail(line, L, S, [&](uint32_t j, uint32_t c) { put(k + j, c); });
      if (adsp) k += put_true(k, put);
      put(k++, uint32_t('\n'));
    }
  }
  for (; k < out_len; ++k) put(k, uint32_t(' '));
}

}  // namespace txt
}  // namespace avdb
