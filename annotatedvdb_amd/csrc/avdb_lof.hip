// K16 — SnpEff LOF/NMD update rows from a VCF and an export of AnnotatedVDB.Variant (gfx950).
//
// Replaces the per-line Python of Load/bin/load_snpeff_lof.py (a VcfEntryParser with its INFO
// dict, a ':'.join and a dict insert per annotated alt allele, parse_annotation_string and an
// xstr(dict) per hit, a bulk SQL lookup per 1,000 ids) with two device passes of two steps each,
// on the skeleton of avdb_tables.hpp (its compaction, scans, totals, checks and host loops).
//   K16a, the table (avdb_lof_table_size / avdb_lof_table_write) over the SnpEff VCF
//     (avdb_lines.hpp in front: one start per line, marks scanned into entry numbers)
//     k_lof_lines    one lane per line (lines::for_each_line: 256 lines' text staged in LDS): the
//                    line rule, the first five fields, INFO by key, the length of the line's JSON
//                    and of its keys; 16 bytes of info and a mark per line
//     tables::k_compact<LofBuild>, tables::k_totals
//     k_lof_keys     rows::write_rows over the key blob, one lane per entry: its keys
//                    chrom:pos:ref:alt_k back to back, and the columns of its rows
//     k_lof_json     rows::write_rows over the JSON blob, one lane per entry: the JSON rendered
//                    once per line (the fraction rewritten by caddupd::score_text)
//   K16b, the update rows (avdb_lof_update_size / avdb_lof_update_write) over the export
//     k_lofupd_lines, tables::k_upd_compact<LofJoin>, rows::begin_write,
//     tables::k_upd_write<kLofWriteStage, LofRows>
// The per-line and per-row code is avdb_lof.hpp, shared with the _host entries.
#include "avdb_tables.hpp"

namespace avdb {

using lof::Table;
using lof::UpdLine;
using tables::EntCols;
using tables::EntryRow;
using tables::EntScans;
using tables::RowCols;
using tables::UpdCols;
using tables::UpdRow;

// VCF lines of a SnpEff run are 100 to 300 bytes (the ANN field): a trip that does not fit 48 KB
// is read from global memory.  Keys are about 12 bytes an alt and a JSON about 120 bytes an
// annotation: 256 entries fit 32 KB; a trip that does not is written bytewise.
constexpr uint32_t kLofSizeStage = 48 * 1024;
constexpr uint32_t kLofWriteStage = 32 * 1024;
constexpr uint32_t kLofUpdSizeStage = 32 * 1024;

struct LofBuild {
  static constexpr int ROWS = AVDB_LOF_COUNT_ROWS, LINES = AVDB_LOF_COUNT_LINES, KEY_BYTES = AVDB_LOF_COUNT_KEY_BYTES,
                       JSON_BYTES = AVDB_LOF_COUNT_JSON_BYTES, HOST_LINES = AVDB_LOF_COUNT_HOST_LINES,
                       BAD = AVDB_LOF_COUNT_BAD, ENTRIES = AVDB_LOF_COUNT_ENTRIES, EXTRA = -1;
  static constexpr uint32_t HOST_BIT = AVDB_LOF_LINE_HOST, BAD_BIT = AVDB_LOF_LINE_BAD, EXTRA_BIT = 0;
  static constexpr bool ROW_PER_ENTRY = false;
  static AVDB_HD bool is_entry(uint32_t w) { return (w & 0xFFu) == lof::kEntry; }
};

struct LofJoin {
  static constexpr int ROWS = AVDB_LOFUPD_COUNT_ROWS, SKIPPED_LINES = AVDB_LOFUPD_COUNT_SKIPPED_LINES,
                       SKIPPED = AVDB_LOFUPD_COUNT_SKIPPED, MISSED = AVDB_LOFUPD_COUNT_NOT_ANNOTATED,
                       BAD = AVDB_LOFUPD_COUNT_BAD, OUT_BYTES = AVDB_LOFUPD_COUNT_OUT_BYTES,
                       LONE_CR = AVDB_LOFUPD_COUNT_LONE_CR, HOST_ROWS = -1;
  static constexpr uint32_t BAD_BIT = AVDB_LOFUPD_BAD, HOST_BIT = 0;
};

struct LofRows {  // an update row against the table
  Table T;
  template <class TextAt, class Put>
  AVDB_HD void operator()(const UpdRow& row, TextAt text, Put put) const {
    lof::render_update_row(row, T, text, put);
  }
};

// info[li] = {alts, key_bytes, json_len, class | flags << 8}
__global__ __launch_bounds__(kBlock) void k_lof_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                      const uint64_t* __restrict__ starts, size_t n_lines,
                                                      u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                      unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kLofSizeStage / 16];
  uint64_t n_cr = 0;
  uint32_t n_comment = 0, n_plain = 0, n_none = 0;
  lines::for_each_line<kLofSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      lof::Parsed P = lof::parse_line(line, len, nl);
      const lof::Entry E = lof::entry_of(line, P);
      info[li] = u32x4{E.n_alts, E.key_bytes, E.json_len, P.cls | (E.flags << 8)};
      mark[li] = P.cls == lof::kEntry;
      n_cr += P.lone_cr;
      n_comment += P.cls == lof::kComment;
      n_plain += P.cls == lof::kUnannotated;
      n_none += P.cls == lof::kNoValues;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the entry count there
  wave_add(&counts[AVDB_LOF_COUNT_LONE_CR], n_cr);
  wave_add(&counts[AVDB_LOF_COUNT_COMMENT_LINES], n_comment);
  wave_add(&counts[AVDB_LOF_COUNT_UNANNOTATED_LINES], n_plain);
  wave_add(&counts[AVDB_LOF_COUNT_NO_VALUES], n_none);
}

__global__ __launch_bounds__(kBlock) void k_lof_keys(const uint8_t* __restrict__ text, size_t text_bytes, EntCols o,
                                                     EntScans sc, size_t n_entries, RowCols R,
                                                     uint8_t* __restrict__ keys, const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kLofWriteStage / 8];
  rows::write_rows<kLofWriteStage>(
      sc.key, n_entries, keys, totals + 2, s_out, [&](size_t e) { return tables::load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) { lof::render_entry_keys(text, text_bytes, E, R, put); });
}

__global__ __launch_bounds__(kBlock) void k_lof_json(const uint8_t* __restrict__ text, size_t text_bytes, EntCols o,
                                                     EntScans sc, size_t n_entries, uint8_t* __restrict__ json,
                                                     const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kLofWriteStage / 8];
  rows::write_rows<kLofWriteStage>(
      sc.json, n_entries, json, totals + 2, s_out, [&](size_t e) { return tables::load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) { lof::render_entry_json(text, text_bytes, E, put); });
}

// ---- K16b ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_lofupd_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                         const uint64_t* __restrict__ starts, size_t n_lines, Table T,
                                                         uint32_t contig_mask, uint32_t update_existing,
                                                         u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kLofUpdSizeStage / 16];
  tables::UpdTally<LofJoin> tally;
  lines::for_each_line<kLofUpdSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const UpdLine L = lof::scan_export_line(line, len, nl, contig_mask, update_existing != 0, T);
      tally.line(L, li, info, mark, T.hit);
    });
  });
  tally.finish(mark, n_lines, counts);
}

}  // namespace avdb

using namespace avdb;

extern "C" int avdb_lof_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(tables::table_layout(n_lines).total, bytes);
}

extern "C" int avdb_lof_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(tables::upd_layout(n_lines).total, bytes);
}

extern "C" int avdb_lof_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   uint64_t* ent_start, uint32_t* ent_alts, uint32_t* ent_key_bytes,
                                   uint32_t* ent_json_len, uint8_t* ent_flags, uint64_t* counts, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tables::table_size<LofBuild>(
      {"avdb_lof_table_size", ctx, {text, text_bytes, n_lines}}, o, counts, AVDB_LOF_N_COUNTS,
      {workspace, workspace_bytes, s}, "k_lof_lines",
      [&](unsigned grid, const uint64_t* starts, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        hipLaunchKernelGGL(k_lof_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, info, marks,
                           cnt);
      });
}

extern "C" int avdb_lof_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    size_t n_entries, size_t n_rows, const uint64_t* ent_start,
                                    const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                    const uint32_t* ent_json_len, const uint8_t* ent_flags, uint8_t* keys,
                                    size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                                    uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                                    uint8_t* row_flags, uint64_t* totals, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tables::table_write<LofBuild>(
      {"avdb_lof_table_write", ctx, {text, text_bytes, n_lines}}, n_entries, n_rows, o,
      {keys, key_cap, json, json_cap, R, totals}, {workspace, workspace_bytes, s}, "k_lof_keys",
      [&](unsigned grid, const EntScans& sc) {
        hipLaunchKernelGGL(k_lof_keys, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, o, sc, n_entries, R, keys,
                           totals);
      },
      "k_lof_json",
      [&](unsigned grid, const EntScans& sc) {
        hipLaunchKernelGGL(k_lof_json, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, o, sc, n_entries, json, totals);
      });
}

// ---- K16a on the host --------------------------------------------------------------------
extern "C" int avdb_lof_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        uint64_t* ent_start, uint32_t* ent_alts, uint32_t* ent_key_bytes,
                                        uint32_t* ent_json_len, uint8_t* ent_flags, uint64_t* counts) {
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  return tables::table_size_host<LofBuild>(
      {"avdb_lof_table_size_host", ctx, {text, text_bytes, n_lines}}, o, counts,
      AVDB_LOF_N_COUNTS, [&](size_t, const uint8_t* line, uint64_t len, bool nl, lof::Entry* E) {
        lof::Parsed P = lof::parse_line(line, len, nl);
        *E = lof::entry_of(line, P);
        counts[AVDB_LOF_COUNT_LONE_CR] += P.lone_cr;
        counts[AVDB_LOF_COUNT_COMMENT_LINES] += P.cls == lof::kComment;
        counts[AVDB_LOF_COUNT_UNANNOTATED_LINES] += P.cls == lof::kUnannotated;
        counts[AVDB_LOF_COUNT_NO_VALUES] += P.cls == lof::kNoValues;
        return P.cls == lof::kEntry;
      });
}

extern "C" int avdb_lof_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         size_t n_entries, size_t n_rows, const uint64_t* ent_start,
                                         const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                         const uint32_t* ent_json_len, const uint8_t* ent_flags, uint8_t* keys,
                                         size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                                         uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                                         uint8_t* row_flags, uint64_t* totals) {
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  return tables::table_write_host<LofBuild>(
      {"avdb_lof_table_write_host", ctx, {text, text_bytes, n_lines}}, n_entries, n_rows, o,
      {keys, key_cap, json, json_cap, R, totals}, "JSON", [&](const EntryRow& E, auto put_key, auto put_json) {
        lof::render_entry_keys(text, text_bytes, E, R, put_key);
        lof::render_entry_json(text, text_bytes, E, put_json);
      });
}

// ---- K16b's entries -------------------------------------------------------------------------
static const char* table_view(const avdb_lof_table* t, Table* T) {
  if (!t) return "null table";
  if (t->struct_size != sizeof(avdb_lof_table)) return "avdb_lof_table of another size";
  memset(T, 0, sizeof(*T));
  return tables::fill_table_view(T, t->n_rows, t->keys, t->key_off, t->keyset, t->keyset_bytes, t->json, t->json_bytes,
                                 t->json_off, t->json_len, t->hit);
}

extern "C" int avdb_lof_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const avdb_lof_table* table, uint32_t contig_mask, uint32_t flags,
                                    uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                                    uint8_t* row_flags, uint64_t* counts, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  Table T;
  const char* err = table_view(table, &T);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t upd = (flags & AVDB_LOFUPD_UPDATE_EXISTING) != 0;
  return tables::update_size<LofJoin>(
      {"avdb_lof_update_size", ctx, {text, text_bytes, n_lines}, err},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_LOFUPD_N_COUNTS,
      {workspace, workspace_bytes, s}, "k_lofupd_lines",
      [&](unsigned grid, const uint64_t* starts, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        hipLaunchKernelGGL(k_lofupd_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, T,
                           contig_mask, upd, info, marks, cnt);
      });
}

extern "C" int avdb_lof_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     size_t n_rows, const avdb_lof_table* table, const uint64_t* row_start,
                                     const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                     const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                     uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  LofRows render{};
  const char* err = table_view(table, &render.T);
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write<kLofWriteStage>({"avdb_lof_update_write", ctx, {text, text_bytes, n_lines}, err}, n_rows, o,
                                              {out, out_cap, row_off, totals},
                                              {workspace, workspace_bytes, static_cast<hipStream_t>(stream)}, render);
}

extern "C" int avdb_lof_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         const avdb_lof_table* table, uint32_t contig_mask, uint32_t flags,
                                         uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                                         uint8_t* row_flags, uint64_t* counts) {
  Table T;
  const char* err = table_view(table, &T);
  const bool upd = (flags & AVDB_LOFUPD_UPDATE_EXISTING) != 0;
  return tables::update_size_host<LofJoin>(
      {"avdb_lof_update_size_host", ctx, {text, text_bytes, n_lines}, err},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_LOFUPD_N_COUNTS, err ? nullptr : T.hit,
      [&](const uint8_t* line, uint64_t len, bool nl) {
        return lof::scan_export_line(line, len, nl, contig_mask, upd, T);
      });
}

extern "C" int avdb_lof_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          size_t n_rows, const avdb_lof_table* table, const uint64_t* row_start,
                                          const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                          const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                          uint64_t* totals) {
  LofRows render{};
  const char* err = table_view(table, &render.T);
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write_host({"avdb_lof_update_write_host", ctx, {text, text_bytes, n_lines}, err}, n_rows, o,
                                   {out, out_cap, row_off, totals}, render);
}
