// K19 — annotation update rows from a tab-delimited file with a header (gfx950).
//
// Replaces the per-line Python of Load/bin/update_variant_annotation.py on TextVariantLoader (a
// csv.DictReader row dict, a split(':') and a SimpleNamespace, a database lookup of the id, a loop
// over the update fields with its 'NULL' test, a tuple) with three device passes of two steps each,
// K19a and K19b on the skeleton of avdb_tables.hpp as K16 is (avdb_lof.hip).
// The header is the host's (csv's own parse of the slab's first bytes): the entries take the lines
// to skip, the header's field count and the columns of `variant` and of the looked-up id.
//   K19a, the table (avdb_txt_table_size / avdb_txt_table_write) over the file
//     k_txt_lines    one lane per line (lines::for_each_line): the line rule, the id, the length
//                    of the update values; 16 bytes of info and a mark per line
//     tables::k_compact<TxtBuild>, tables::k_totals
//     k_txt_keys     rows::write_rows over the key blob, one lane per entry: its looked-up id
//     k_txt_bodies   rows::write_rows over the body blob, one lane per entry: <label><TAB><values>
//                    (both read a trip's lines from LDS, staged per trip as the size pass stages them)
//   K19b, the update rows (avdb_txt_update_size / avdb_txt_update_write) over the export, with
//   the looked-up column chosen by key_col
//     k_txtupd_lines, tables::k_upd_compact<TxtJoin>, rows::begin_write,
//     tables::k_upd_write<kTxtWriteStage, TxtRows>
//   K19c, the update rows of a file of primary keys (avdb_txt_direct_size / avdb_txt_direct_write)
//     k_txtdir_lines, k_txtdir_compact, rows::begin_write, k_txtdir_write
// The per-line and per-row code is avdb_txt.hpp, shared with the _host entries.
#include "avdb_txt.hpp"
#include "avdb_tables.hpp"

namespace avdb {

using tables::EntCols;
using tables::EntryRow;
using tables::EntScans;
using tables::RowCols;
using tables::UpdCols;
using tables::UpdRow;
using tables::upd_layout;
using txt::Shape;

// Lines of such a file are tens of bytes to a few hundred (a JSON value): a trip that does not
// fit the stage is read from global memory, a trip of rows that does not is written bytewise.
constexpr uint32_t kTxtSizeStage = 48 * 1024;
constexpr uint32_t kTxtWriteStage = 32 * 1024;
// An export line is about 50 bytes (a primary key, a metaseq id, a refSNP id): 256 of them take
// 12 KB, and K16b's 32 KB stage holds them with room; the smaller stage leaves more workgroups a CU.
constexpr uint32_t kTxtUpdSizeStage = 32 * 1024;

// The text of a write pass's trip.  Entries and rows are in file order, so the lines of rows
// [r0, r0 + nr) lie in one span of the text, from the first one's start to the start of the next
// trip's first: it is staged in LDS as the size passes stage theirs, and a lane reads its line
// there.  A line that does not lie in the staged span (a span that does not fit, starts the caller
// overwrote) is read from global memory.
struct TripText {
  Window w;
  uint64_t s0, s1;
};

template <uint32_t kStageBytes>
__device__ __forceinline__ TripText stage_trip(const Heap& h, const uint64_t* __restrict__ at, size_t r0, uint32_t nr,
                                               size_t n, uint64_t text_bytes, u32x4* s_text) {
  TripText t;
  lines::trip_span(at, r0, r0 + nr, n, text_bytes, &t.s0, &t.s1);
  t.w = stage_window<kBlock, kStageBytes>(h, t.s0, t.s1, s_text);
  return t;
}

// f(line, len, nl, have): the line that starts at `start`, as txt::with_line_at gives it
template <class F>
__device__ __forceinline__ void with_trip_line(const uint8_t* __restrict__ text, uint64_t text_bytes, const Heap& h,
                                               const TripText& t, const u32x4* s_text, uint64_t start, F f) {
  if (t.w.staged && start >= t.s0 && start < t.s1) {
    const lds_cp p = (lds_cp)(reinterpret_cast<const uint8_t*>(s_text) + (h.lo + start - t.w.a0));
    const uint64_t room = t.s1 - start;
    uint64_t n = 0;
    while (n < room && p[n] != '\n') ++n;
    if (n < room || t.s1 >= text_bytes) {  // (else the line runs past the span)
      f(p, n, n < room, true);
      return;
    }
  }
  txt::with_line_at(text, text_bytes, start,
                    [&](const uint8_t* line, uint64_t len, bool nl, bool have) { f((glb_cp)line, len, nl, have); });
}

struct TxtBuild {  // (JSON_BYTES: the bodies' bytes)
  static constexpr int ROWS = AVDB_TXT_COUNT_ROWS, LINES = AVDB_TXT_COUNT_LINES, KEY_BYTES = AVDB_TXT_COUNT_KEY_BYTES,
                       JSON_BYTES = AVDB_TXT_COUNT_JSON_BYTES, HOST_LINES = AVDB_TXT_COUNT_HOST_LINES,
                       BAD = AVDB_TXT_COUNT_BAD, ENTRIES = AVDB_TXT_COUNT_ENTRIES, EXTRA = -1;
  static constexpr uint32_t HOST_BIT = AVDB_TXT_LINE_HOST, BAD_BIT = AVDB_TXT_LINE_BAD, EXTRA_BIT = 0;
  static constexpr bool ROW_PER_ENTRY = true;
  static AVDB_HD bool is_entry(uint32_t w) { return (w & 1u) != 0; }
};

struct TxtJoin {  // (no record is skipped for what it holds already)
  static constexpr int ROWS = AVDB_TXTUPD_COUNT_ROWS, SKIPPED_LINES = AVDB_TXTUPD_COUNT_SKIPPED_LINES, SKIPPED = -1,
                       MISSED = AVDB_TXTUPD_COUNT_NOT_IN_FILE, BAD = AVDB_TXTUPD_COUNT_BAD,
                       OUT_BYTES = AVDB_TXTUPD_COUNT_OUT_BYTES, LONE_CR = AVDB_TXTUPD_COUNT_LONE_CR,
                       HOST_ROWS = AVDB_TXTUPD_COUNT_HOST_ROWS;
  static constexpr uint32_t BAD_BIT = AVDB_TXTUPD_BAD, HOST_BIT = AVDB_TXTUPD_TABLE_HOST;
};

struct TxtRows {  // an update row against the table
  txt::Table T;
  uint32_t adsp;
  template <class TextAt, class Put>
  AVDB_HD void operator()(const UpdRow& row, TextAt text, Put put) const {
    txt::render_update_row(row, T, adsp != 0, text, put);
  }
};

// info[li] = {alts, key_bytes, body_len, is_entry | flags << 8}
__global__ __launch_bounds__(kBlock) void k_txt_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                      const uint64_t* __restrict__ starts, size_t n_lines, Shape S,
                                                      u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                      unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kTxtSizeStage / 16];
  uint64_t n_cr = 0;
  uint32_t n_skip = 0;
  lines::for_each_line<kTxtSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const txt::Line L = txt::parse_line(line, len, nl, li >= S.skip_lines, S);
      const bool dev = L.data && !L.flags;
      info[li] = u32x4{dev ? 1u : 0u, dev ? L.key_n : 0u, dev ? txt::body_len(L) : 0u, L.data | (L.flags << 8)};
      mark[li] = L.data;
      n_cr += L.lone_cr;
      n_skip += !L.data;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the entry count there
  wave_add(&counts[AVDB_TXT_COUNT_LONE_CR], n_cr);
  wave_add(&counts[AVDB_TXT_COUNT_SKIPPED_LINES], n_skip);
}

__global__ __launch_bounds__(kBlock) void k_txt_keys(const uint8_t* __restrict__ text, size_t text_bytes, Shape S,
                                                     EntCols o, EntScans sc, size_t n_entries, RowCols R,
                                                     uint8_t* __restrict__ keys, const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kTxtWriteStage / 8];
  __shared__ u32x4 s_text[kTxtWriteStage / 16];
  const Heap h = make_heap(text, text_bytes);
  TripText trip;
  rows::write_rows<kTxtWriteStage>(
      sc.key, n_entries, keys, totals + 2, s_out,
      [&](size_t r0, uint32_t nr) { trip = stage_trip<kTxtWriteStage>(h, o.start, r0, nr, n_entries, text_bytes, s_text); },
      [&](size_t e) { return tables::load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) {
        with_trip_line(text, text_bytes, h, trip, s_text, E.start, [&](auto line, uint64_t len, bool nl, bool have) {
          txt::render_entry_key(line, len, nl, have, E, R, S, put);
        });
      });
}

__global__ __launch_bounds__(kBlock) void k_txt_bodies(const uint8_t* __restrict__ text, size_t text_bytes, Shape S,
                                                       EntCols o, EntScans sc, size_t n_entries,
                                                       uint8_t* __restrict__ body,
                                                       const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kTxtWriteStage / 8];
  __shared__ u32x4 s_text[kTxtWriteStage / 16];
  const Heap h = make_heap(text, text_bytes);
  TripText trip;
  rows::write_rows<kTxtWriteStage>(
      sc.json, n_entries, body, totals + 2, s_out,
      [&](size_t r0, uint32_t nr) { trip = stage_trip<kTxtWriteStage>(h, o.start, r0, nr, n_entries, text_bytes, s_text); },
      [&](size_t e) { return tables::load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) {
        with_trip_line(text, text_bytes, h, trip, s_text, E.start, [&](auto line, uint64_t len, bool nl, bool have) {
          txt::render_entry_body(line, len, nl, have, E, S, put);
        });
      });
}

// ---- K19b ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_txtupd_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                         const uint64_t* __restrict__ starts, size_t n_lines,
                                                         txt::Table T, uint32_t contig_mask, uint32_t key_col,
                                                         uint32_t adsp, u32x4* __restrict__ info,
                                                         uint64_t* __restrict__ mark,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kTxtUpdSizeStage / 16];
  tables::UpdTally<TxtJoin> tally;
  lines::for_each_line<kTxtUpdSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const txt::UpdLine L = txt::scan_export_line(line, len, nl, contig_mask, key_col, adsp != 0, T);
      tally.line(L, li, info, mark, T.t.hit);
    });
  });
  tally.finish(mark, n_lines, counts);
}

// ---- K19c ---------------------------------------------------------------------------------
struct TxtDirCols {  // per row, n_lines entries allocated
  uint64_t* row_start;
  uint32_t* out_len;
  uint8_t* flags;
};

struct DirRow {
  uint64_t start;
  uint32_t out_len, flags;
};

// info[li] = {out_len, flags, is_row, 0}
__global__ __launch_bounds__(kBlock) void k_txtdir_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                         const uint64_t* __restrict__ starts, size_t n_lines, Shape S,
                                                         uint32_t adsp, u32x4* __restrict__ info,
                                                         uint64_t* __restrict__ mark,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kTxtSizeStage / 16];
  uint64_t n_cr = 0;
  uint32_t n_skip = 0;
  lines::for_each_line<kTxtSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      txt::Line L = txt::parse_line(line, len, nl, li >= S.skip_lines, S);
      uint32_t out = txt::direct_len(L, adsp != 0);
      if (L.data && !L.flags && !out) L.flags = AVDB_TXT_LINE_HOST | AVDB_TXT_LINE_BAD;  // (no such row fits a slab)
      info[li] = u32x4{out, L.flags, L.data, 0u};
      mark[li] = L.data;
      n_cr += L.lone_cr;
      n_skip += !L.data;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the row count there
  wave_add(&counts[AVDB_TXTDIR_COUNT_LONE_CR], n_cr);
  wave_add(&counts[AVDB_TXTDIR_COUNT_SKIPPED_LINES], n_skip);
}

__global__ __launch_bounds__(kBlock) void k_txtdir_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                           size_t n_lines, const u32x4* __restrict__ info,
                                                           const uint64_t* __restrict__ row_of, TxtDirCols o,
                                                           unsigned long long* __restrict__ counts) {
  uint64_t bytes = 0;
  uint32_t n_bad = 0, n_host = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 v = info[li];
    if (!v.z) continue;
    const uint64_t r = row_of[li];  // r < n_lines: at most one row per line
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    o.row_start[r] = s;
    o.out_len[r] = v.x;
    o.flags[r] = uint8_t(v.y);
    bytes += v.x;
    n_host += (v.y & AVDB_TXT_LINE_HOST) != 0;
    n_bad += (v.y & AVDB_TXT_LINE_BAD) != 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[AVDB_TXTDIR_COUNT_ROWS] = row_of[n_lines];
    counts[AVDB_TXTDIR_COUNT_LINES] = n_lines;
  }
  wave_add(&counts[AVDB_TXTDIR_COUNT_OUT_BYTES], bytes);
  wave_add(&counts[AVDB_TXTDIR_COUNT_HOST_ROWS], n_host);
  wave_add(&counts[AVDB_TXTDIR_COUNT_BAD], n_bad);
}

__global__ __launch_bounds__(kBlock) void k_txtdir_write(const uint8_t* __restrict__ text, size_t text_bytes, Shape S,
                                                         uint32_t adsp, TxtDirCols o,
                                                         const uint64_t* __restrict__ row_off, size_t n_rows,
                                                         uint8_t* __restrict__ out,
                                                         const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kTxtWriteStage / 8];
  __shared__ u32x4 s_text[kTxtWriteStage / 16];
  const Heap h = make_heap(text, text_bytes);
  TripText trip;
  rows::write_rows<kTxtWriteStage>(
      row_off, n_rows, out, totals, s_out,
      [&](size_t r0, uint32_t nr) { trip = stage_trip<kTxtWriteStage>(h, o.row_start, r0, nr, n_rows, text_bytes, s_text); },
      [&](size_t r) { return DirRow{o.row_start[r], o.out_len[r], o.flags[r]}; },
      [&](const DirRow& row, auto put) {
        with_trip_line(text, text_bytes, h, trip, s_text, row.start, [&](auto line, uint64_t len, bool nl, bool have) {
          txt::render_direct_row(line, len, nl, have, row.out_len, row.flags, S, adsp != 0, put);
        });
      });
}

}  // namespace avdb

using namespace avdb;

extern "C" int avdb_txt_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(tables::table_layout(n_lines).total, bytes);
}

extern "C" int avdb_txt_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(upd_layout(n_lines).total, bytes);
}

extern "C" int avdb_txt_direct_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(upd_layout(n_lines).total, bytes);
}

extern "C" int avdb_txt_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t key_col,
                                   uint64_t* ent_start, uint32_t* ent_alts, uint32_t* ent_key_bytes,
                                   uint32_t* ent_body_len, uint8_t* ent_flags, uint64_t* counts, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const Shape S{skip_lines, n_fields, id_col, key_col};
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_body_len, ent_flags};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tables::table_size<TxtBuild>(
      {"avdb_txt_table_size", ctx, {text, text_bytes, n_lines}, nullptr, txt::shape_error(S)}, o, counts,
      AVDB_TXT_N_COUNTS, {workspace, workspace_bytes, s}, "k_txt_lines",
      [&](unsigned grid, const uint64_t* starts, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        hipLaunchKernelGGL(k_txt_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, S, info, marks,
                           cnt);
      });
}

extern "C" int avdb_txt_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    size_t n_entries, size_t n_rows, uint32_t skip_lines, uint32_t n_fields,
                                    uint32_t id_col, uint32_t key_col, const uint64_t* ent_start,
                                    const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                    const uint32_t* ent_body_len, const uint8_t* ent_flags, uint8_t* keys,
                                    size_t key_cap, uint64_t* key_off, uint8_t* body, size_t body_cap,
                                    uint64_t* row_body_off, uint32_t* row_body_len, uint64_t* row_line_start,
                                    uint8_t* row_flags, uint64_t* totals, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const Shape S{skip_lines, n_fields, id_col, key_col};
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_body_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_body_off, row_body_len, row_line_start, row_flags, n_rows};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tables::table_write<TxtBuild>(
      {"avdb_txt_table_write", ctx, {text, text_bytes, n_lines}, nullptr, txt::shape_error(S)}, n_entries,
      n_rows, o, {keys, key_cap, body, body_cap, R, totals}, {workspace, workspace_bytes, s}, "k_txt_keys",
      [&](unsigned grid, const EntScans& sc) {
        hipLaunchKernelGGL(k_txt_keys, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, S, o, sc, n_entries, R, keys,
                           totals);
      },
      "k_txt_bodies",
      [&](unsigned grid, const EntScans& sc) {
        hipLaunchKernelGGL(k_txt_bodies, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, S, o, sc, n_entries, body,
                           totals);
      });
}

// ---- K19a on the host --------------------------------------------------------------------
extern "C" int avdb_txt_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t key_col,
                                        uint64_t* ent_start, uint32_t* ent_alts, uint32_t* ent_key_bytes,
                                        uint32_t* ent_body_len, uint8_t* ent_flags, uint64_t* counts) {
  const Shape S{skip_lines, n_fields, id_col, key_col};
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_body_len, ent_flags};
  return tables::table_size_host<TxtBuild>(
      {"avdb_txt_table_size_host", ctx, {text, text_bytes, n_lines}, nullptr, txt::shape_error(S)}, o,
      counts, AVDB_TXT_N_COUNTS, [&](size_t li, const uint8_t* line, uint64_t len, bool nl, lof::Entry* E) {
        const txt::Line L = txt::parse_line(line, len, nl, li >= S.skip_lines, S);
        const bool dev = L.data && !L.flags;
        *E = lof::Entry{dev ? 1u : 0u, dev ? L.key_n : 0u, dev ? txt::body_len(L) : 0u, L.flags};
        counts[AVDB_TXT_COUNT_LONE_CR] += L.lone_cr;
        counts[AVDB_TXT_COUNT_SKIPPED_LINES] += !L.data;
        return L.data != 0;
      });
}

extern "C" int avdb_txt_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         size_t n_entries, size_t n_rows, uint32_t skip_lines, uint32_t n_fields,
                                         uint32_t id_col, uint32_t key_col, const uint64_t* ent_start,
                                         const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                         const uint32_t* ent_body_len, const uint8_t* ent_flags, uint8_t* keys,
                                         size_t key_cap, uint64_t* key_off, uint8_t* body, size_t body_cap,
                                         uint64_t* row_body_off, uint32_t* row_body_len, uint64_t* row_line_start,
                                         uint8_t* row_flags, uint64_t* totals) {
  const Shape S{skip_lines, n_fields, id_col, key_col};
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_body_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_body_off, row_body_len, row_line_start, row_flags, n_rows};
  return tables::table_write_host<TxtBuild>(
      {"avdb_txt_table_write_host", ctx, {text, text_bytes, n_lines}, nullptr, txt::shape_error(S)},
      n_entries, n_rows, o, {keys, key_cap, body, body_cap, R, totals}, "body",
      [&](const EntryRow& E, auto put_key, auto put_body) {
        txt::with_line_at(text, text_bytes, E.start, [&](const uint8_t* line, uint64_t len, bool nl, bool have) {
          txt::render_entry_key(line, len, nl, have, E, R, S, put_key);
          txt::render_entry_body(line, len, nl, have, E, S, put_body);
        });
      });
}

// ---- K19b's entries -------------------------------------------------------------------------
static const char* table_view(const avdb_txt_table* t, txt::Table* T) {
  if (!t) return "null table";
  if (t->struct_size != sizeof(avdb_txt_table)) return "avdb_txt_table of another size";
  memset(T, 0, sizeof(*T));
  const char* err = tables::fill_table_view(&T->t, t->n_rows, t->keys, t->key_off, t->keyset, t->keyset_bytes, t->body,
                                            t->body_bytes, t->body_off, t->body_len, t->hit, !t->flags);
  if (!err && t->n_rows) T->flags = t->flags;
  return err;
}

static const char* key_col_error(uint32_t key_col) {
  return key_col != 1 && key_col != 2 ? "key_col out of range (1: metaseq_id, 2: ref_snp_id)" : nullptr;
}

extern "C" int avdb_txt_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const avdb_txt_table* table, uint32_t contig_mask, uint32_t key_col,
                                    uint32_t flags, uint64_t* row_start, uint32_t* pk_len, int32_t* match,
                                    uint32_t* out_len, uint8_t* row_flags, uint64_t* counts, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  txt::Table T;
  const char* err = table_view(table, &T);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t adsp = (flags & AVDB_TXT_ADSP) != 0;
  return tables::update_size<TxtJoin>(
      {"avdb_txt_update_size", ctx, {text, text_bytes, n_lines}, err, key_col_error(key_col)},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_TXTUPD_N_COUNTS,
      {workspace, workspace_bytes, s}, "k_txtupd_lines",
      [&](unsigned grid, const uint64_t* starts, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        hipLaunchKernelGGL(k_txtupd_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, T,
                           contig_mask, key_col, adsp, info, marks, cnt);
      });
}

extern "C" int avdb_txt_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     size_t n_rows, const avdb_txt_table* table, uint32_t flags,
                                     const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                     const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                                     uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  TxtRows render{};
  const char* err = table_view(table, &render.T);
  render.adsp = (flags & AVDB_TXT_ADSP) != 0;
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write<kTxtWriteStage>({"avdb_txt_update_write", ctx, {text, text_bytes, n_lines}, err}, n_rows, o,
                                              {out, out_cap, row_off, totals},
                                              {workspace, workspace_bytes, static_cast<hipStream_t>(stream)}, render);
}

extern "C" int avdb_txt_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         const avdb_txt_table* table, uint32_t contig_mask, uint32_t key_col,
                                         uint32_t flags, uint64_t* row_start, uint32_t* pk_len, int32_t* match,
                                         uint32_t* out_len, uint8_t* row_flags, uint64_t* counts) {
  txt::Table T;
  const char* err = table_view(table, &T);
  const bool adsp = (flags & AVDB_TXT_ADSP) != 0;
  return tables::update_size_host<TxtJoin>(
      {"avdb_txt_update_size_host", ctx, {text, text_bytes, n_lines}, err, key_col_error(key_col)},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_TXTUPD_N_COUNTS, err ? nullptr : T.t.hit,
      [&](const uint8_t* line, uint64_t len, bool nl) {
        return txt::scan_export_line(line, len, nl, contig_mask, key_col, adsp, T);
      });
}

extern "C" int avdb_txt_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          size_t n_rows, const avdb_txt_table* table, uint32_t flags,
                                          const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                          const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                                          size_t out_cap, uint64_t* row_off, uint64_t* totals) {
  TxtRows render{};
  const char* err = table_view(table, &render.T);
  render.adsp = (flags & AVDB_TXT_ADSP) != 0;
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write_host({"avdb_txt_update_write_host", ctx, {text, text_bytes, n_lines}, err}, n_rows, o,
                                   {out, out_cap, row_off, totals}, render);
}

// ---- K19c's entries -------------------------------------------------------------------------
static const char* dir_size_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                  const Shape& S, const TxtDirCols& o, const uint64_t* counts) {
  if (!ctx || !counts) return "null argument";
  if (const char* err = txt::shape_error(S)) return err;
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!o.row_start || !o.out_len || !o.flags)) return "null output array";
  return nullptr;
}

static const char* dir_write_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   size_t n_rows, const Shape& S, const TxtDirCols& o, const uint8_t* out,
                                   size_t out_cap, const uint64_t* row_off, const uint64_t* totals) {
  if (!ctx || !totals || !row_off) return "null argument";
  if (const char* err = txt::shape_error(S)) return err;
  if (const char* err = rows::text_rows_error(text, text_bytes, n_lines, n_rows)) return err;
  if (n_rows && (!o.row_start || !o.out_len || !o.flags)) return "null row array";
  return rows::out_error(out, out_cap);
}

extern "C" int avdb_txt_direct_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t flags,
                                    uint64_t* row_start, uint32_t* out_len, uint8_t* row_flags, uint64_t* counts,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const Shape S{skip_lines, n_fields, id_col, id_col};
  const TxtDirCols o{row_start, out_len, row_flags};
  if (const char* err = dir_size_error(ctx, text, text_bytes, n_lines, S, o, counts)) {
    avdb_set_error("avdb_txt_direct_size: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = upd_layout(n_lines);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_txt_direct_size", ctx, L.total, n_lines, workspace, workspace_bytes, counts,
                               AVDB_TXTDIR_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* info = reinterpret_cast<u32x4*>(w + L.info);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned grid = stream_grid(n_lines, kBlock, 4096);
  const uint32_t adsp = (flags & AVDB_TXT_ADSP) != 0;
  auto mark = [&](const uint64_t* starts, uint64_t* marks) {
    hipLaunchKernelGGL(k_txtdir_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, S, adsp, info,
                       marks, cnt);
  };
  if (int e = lines::number_rows(text, text_bytes, n_lines, w, L, s, "k_txtdir_lines", mark)) return e;
  hipLaunchKernelGGL(k_txtdir_compact, dim3(grid), dim3(kBlock), 0, s,
                     reinterpret_cast<const uint64_t*>(w + L.starts), text_bytes, n_lines, info,
                     reinterpret_cast<const uint64_t*>(w + L.row_of), o, cnt);
  AVDB_LAUNCH_CHECK("k_txtdir_compact");
  return AVDB_OK;
}

extern "C" int avdb_txt_direct_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     size_t n_rows, uint32_t skip_lines, uint32_t n_fields, uint32_t id_col,
                                     uint32_t flags, const uint64_t* row_start, const uint32_t* out_len,
                                     const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                     uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  const Shape S{skip_lines, n_fields, id_col, id_col};
  const TxtDirCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(out_len),
                     const_cast<uint8_t*>(row_flags)};
  if (const char* err = dir_write_error(ctx, text, text_bytes, n_lines, n_rows, S, o, out, out_cap, row_off, totals)) {
    avdb_set_error("avdb_txt_direct_write: %s", err);
    return AVDB_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_write("avdb_txt_direct_write", ctx, upd_layout(n_lines), n_lines, workspace, workspace_bytes,
                                out_len, n_rows, out_cap, row_off, totals, s))
    return e;
  if (n_rows == 0) return AVDB_OK;
  hipLaunchKernelGGL(k_txtdir_write, dim3(stream_grid(n_rows, kBlock, 2048)), dim3(kBlock), 0, s, text, text_bytes, S,
                     uint32_t((flags & AVDB_TXT_ADSP) != 0), o, row_off, n_rows, out, totals);
  AVDB_LAUNCH_CHECK("k_txtdir_write");
  return AVDB_OK;
}

extern "C" int avdb_txt_direct_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t flags,
                                         uint64_t* row_start, uint32_t* out_len, uint8_t* row_flags,
                                         uint64_t* counts) {
  const Shape S{skip_lines, n_fields, id_col, id_col};
  const TxtDirCols o{row_start, out_len, row_flags};
  if (const char* err = dir_size_error(ctx, text, text_bytes, n_lines, S, o, counts)) {
    avdb_set_error("avdb_txt_direct_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_TXTDIR_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  const bool adsp = (flags & AVDB_TXT_ADSP) != 0;
  uint64_t rows = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    bool nl;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e, &nl);
    txt::Line L = txt::parse_line(text + s, e - s, nl, li >= S.skip_lines, S);
    const uint32_t out = txt::direct_len(L, adsp);
    if (L.data && !L.flags && !out) L.flags = AVDB_TXT_LINE_HOST | AVDB_TXT_LINE_BAD;
    counts[AVDB_TXTDIR_COUNT_LONE_CR] += L.lone_cr;
    counts[AVDB_TXTDIR_COUNT_SKIPPED_LINES] += !L.data;
    if (!L.data) continue;
    row_start[rows] = s;
    out_len[rows] = out;
    row_flags[rows] = uint8_t(L.flags);
    ++rows;
    counts[AVDB_TXTDIR_COUNT_OUT_BYTES] += out;
    counts[AVDB_TXTDIR_COUNT_HOST_ROWS] += (L.flags & AVDB_TXT_LINE_HOST) != 0;
    counts[AVDB_TXTDIR_COUNT_BAD] += (L.flags & AVDB_TXT_LINE_BAD) != 0;
  }
  counts[AVDB_TXTDIR_COUNT_ROWS] = rows;
  counts[AVDB_TXTDIR_COUNT_LINES] = n_lines;
  return AVDB_OK;
}

extern "C" int avdb_txt_direct_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          size_t n_rows, uint32_t skip_lines, uint32_t n_fields, uint32_t id_col,
                                          uint32_t flags, const uint64_t* row_start, const uint32_t* out_len,
                                          const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                          uint64_t* totals) {
  const Shape S{skip_lines, n_fields, id_col, id_col};
  const TxtDirCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(out_len),
                     const_cast<uint8_t*>(row_flags)};
  if (const char* err = dir_write_error(ctx, text, text_bytes, n_lines, n_rows, S, o, out, out_cap, row_off, totals)) {
    avdb_set_error("avdb_txt_direct_write_host: %s", err);
    return AVDB_EINVAL;
  }
  if (int e = rows::host_row_offsets("avdb_txt_direct_write_host", out_len, n_rows, out_cap, row_off, totals)) return e;
  const bool adsp = (flags & AVDB_TXT_ADSP) != 0;
  for (size_t r = 0; r < n_rows; ++r) {
    const uint64_t off = row_off[r];
    txt::with_line_at(text, text_bytes, row_start[r], [&](const uint8_t* line, uint64_t len, bool nl, bool have) {
      txt::render_direct_row(line, len, nl, have, out_len[r], row_flags[r], S, adsp,
                             [&](uint32_t k, uint32_t c) { out[off + k] = uint8_t(c); });
    });
  }
  return AVDB_OK;
}
