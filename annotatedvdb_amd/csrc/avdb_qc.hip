// K17 — ADSP QC pVCF update rows from a VCF and an export of AnnotatedVDB.Variant (gfx950).
//
// Replaces the per-line Python of Load/bin/update_from_qc_pvcf_file.py (a VcfEntryParser with two
// dict comprehensions over INFO and to_numeric on every value, a ':'.join and a dict insert per alt
// allele, an xstr(dict) per hit, a bulk SQL lookup per 1,000 ids) with two device passes of two
// steps each, on the skeleton of avdb_tables.hpp as K16 is (avdb_lof.hip).
//   K17a, the table (avdb_qc_table_size / avdb_qc_table_write) over the QC VCF
//     k_qc_lines     one lane per line (lines::for_each_line: 256 lines' text staged in LDS): the
//                    first five fields, the bytes of QUAL .. FORMAT, INFO's keys, the length of
//                    the line's JSON and of its keys; 16 bytes of info and a mark per line
//     tables::k_compact<QcBuild> (it counts AVDB_QC_PASS too), tables::k_totals
//     k_qc_keys      rows::write_rows over the key blob, one lane per entry
//     k_qc_json      rows::write_rows over the JSON blob, one lane per entry: INFO, FILTER, QUAL
//                    and FORMAT rendered as json.dumps prints what to_numeric makes of them
//   K17b, the update rows (avdb_qc_update_size / avdb_qc_update_write) over the export, with the
//   depth-1 key scan of the adsp_qc column in place of K16b's NULL test
//     k_qcupd_lines, tables::k_upd_compact<QcJoin>, rows::begin_write,
//     tables::k_upd_write<kQcJsonStage, QcRows>
// The per-line and per-row code is avdb_qc.hpp, shared with the _host entries.
#include "avdb_qc.hpp"
#include "avdb_tables.hpp"

namespace avdb {

using qc::Release;
using qc::Table;
using qc::UpdLine;
using tables::EntCols;
using tables::EntryRow;
using tables::EntScans;
using tables::RowCols;
using tables::UpdCols;
using tables::UpdRow;

// A QC line without its sample columns is 150 to 300 bytes, its JSON about as long again; a line
// with sample columns is far longer, and a trip that does not fit 48 KB is read from global memory.
// 256 JSON texts of up to 256 bytes fit the 64 KB a workgroup can have; a trip that does not fit is
// written bytewise.
constexpr uint32_t kQcSizeStage = 48 * 1024;
constexpr uint32_t kQcKeyStage = 32 * 1024;
constexpr uint32_t kQcJsonStage = 64 * 1024;
constexpr uint32_t kQcUpdSizeStage = 48 * 1024;

struct QcBuild {
  static constexpr int ROWS = AVDB_QC_COUNT_ROWS, LINES = AVDB_QC_COUNT_LINES, KEY_BYTES = AVDB_QC_COUNT_KEY_BYTES,
                       JSON_BYTES = AVDB_QC_COUNT_JSON_BYTES, HOST_LINES = AVDB_QC_COUNT_HOST_LINES,
                       BAD = AVDB_QC_COUNT_BAD, ENTRIES = AVDB_QC_COUNT_ENTRIES, EXTRA = AVDB_QC_COUNT_PASS;
  static constexpr uint32_t HOST_BIT = AVDB_QC_LINE_HOST, BAD_BIT = AVDB_QC_LINE_BAD, EXTRA_BIT = AVDB_QC_PASS;
  static constexpr bool ROW_PER_ENTRY = false;
  static AVDB_HD bool is_entry(uint32_t w) { return (w & 0xFFu) == lof::kEntry; }
};

struct QcJoin {
  static constexpr int ROWS = AVDB_QCUPD_COUNT_ROWS, SKIPPED_LINES = AVDB_QCUPD_COUNT_SKIPPED_LINES,
                       SKIPPED = AVDB_QCUPD_COUNT_SKIPPED, MISSED = AVDB_QCUPD_COUNT_NOT_IN_VCF,
                       BAD = AVDB_QCUPD_COUNT_BAD, OUT_BYTES = AVDB_QCUPD_COUNT_OUT_BYTES,
                       LONE_CR = AVDB_QCUPD_COUNT_LONE_CR, HOST_ROWS = AVDB_QCUPD_COUNT_HOST_ROWS;
  static constexpr uint32_t BAD_BIT = AVDB_QCUPD_BAD, HOST_BIT = AVDB_QCUPD_ROW_HOST;
};

struct QcRows {  // an update row against the table
  Table T;
  template <class TextAt, class Put>
  AVDB_HD void operator()(const UpdRow& row, TextAt text, Put put) const {
    qc::render_update_row(row, T, text, put);
  }
};

// info[li] = {alts, key_bytes, json_len, class | flags << 8}
__global__ __launch_bounds__(kBlock) void k_qc_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                     const uint64_t* __restrict__ starts, size_t n_lines, Release rel,
                                                     u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                     unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kQcSizeStage / 16];
  uint64_t n_cr = 0;
  uint32_t n_comment = 0;
  lines::for_each_line<kQcSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      qc::Parsed Q = qc::parse_line(line, len, nl, true);
      const lof::Entry E = qc::entry_of(line, Q, rel);
      info[li] = u32x4{E.n_alts, E.key_bytes, E.json_len, Q.b.cls | (E.flags << 8)};
      mark[li] = Q.b.cls == lof::kEntry;
      n_cr += Q.b.lone_cr;
      n_comment += Q.b.cls == lof::kComment;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the entry count there
  wave_add(&counts[AVDB_QC_COUNT_LONE_CR], n_cr);
  wave_add(&counts[AVDB_QC_COUNT_COMMENT_LINES], n_comment);
}

__global__ __launch_bounds__(kBlock) void k_qc_keys(const uint8_t* __restrict__ text, size_t text_bytes, EntCols o,
                                                    EntScans sc, size_t n_entries, RowCols R,
                                                    uint8_t* __restrict__ keys, const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kQcKeyStage / 8];
  rows::write_rows<kQcKeyStage>(
      sc.key, n_entries, keys, totals + 2, s_out, [&](size_t e) { return tables::load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) { qc::render_entry_keys(text, text_bytes, E, R, put); });
}

__global__ __launch_bounds__(kBlock) void k_qc_json(const uint8_t* __restrict__ text, size_t text_bytes, Release rel,
                                                    EntCols o, EntScans sc, size_t n_entries,
                                                    uint8_t* __restrict__ json, const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kQcJsonStage / 8];
  rows::write_rows<kQcJsonStage>(
      sc.json, n_entries, json, totals + 2, s_out, [&](size_t e) { return tables::load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) { qc::render_entry_json(text, text_bytes, E, rel, put); });
}

// ---- K17b ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_qcupd_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                        const uint64_t* __restrict__ starts, size_t n_lines, Table T,
                                                        uint32_t contig_mask, uint32_t update_existing,
                                                        u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kQcUpdSizeStage / 16];
  tables::UpdTally<QcJoin> tally;
  lines::for_each_line<kQcUpdSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const UpdLine L = qc::scan_export_line(line, len, nl, contig_mask, update_existing != 0, T);
      tally.line(L, li, info, mark, T.t.hit);
    });
  });
  tally.finish(mark, n_lines, counts);
}

}  // namespace avdb

using namespace avdb;

extern "C" int avdb_qc_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(tables::table_layout(n_lines).total, bytes);
}

extern "C" int avdb_qc_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(tables::upd_layout(n_lines).total, bytes);
}

static const char* release_view(const uint8_t* release, size_t release_len, Release* rel) {
  memset(rel, 0, sizeof(*rel));
  if (!qc::release_ok(release, release_len)) return "the release must be 1 .. 64 ASCII bytes without '\"', '\\' and control bytes";
  memcpy(rel->b, release, release_len);
  rel->n = uint32_t(release_len);
  return nullptr;
}

extern "C" int avdb_qc_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                  const uint8_t* release, size_t release_len, uint64_t* ent_start, uint32_t* ent_alts,
                                  uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags, uint64_t* counts,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tables::table_size<QcBuild>(
      {"avdb_qc_table_size", ctx, {text, text_bytes, n_lines}, err}, o, counts, AVDB_QC_N_COUNTS,
      {workspace, workspace_bytes, s}, "k_qc_lines",
      [&](unsigned grid, const uint64_t* starts, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        hipLaunchKernelGGL(k_qc_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, rel, info,
                           marks, cnt);
      });
}

extern "C" int avdb_qc_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   size_t n_entries, size_t n_rows, const uint8_t* release, size_t release_len,
                                   const uint64_t* ent_start, const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                   const uint32_t* ent_json_len, const uint8_t* ent_flags, uint8_t* keys,
                                   size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                                   uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                                   uint8_t* row_flags, uint64_t* totals, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tables::table_write<QcBuild>(
      {"avdb_qc_table_write", ctx, {text, text_bytes, n_lines}, err}, n_entries, n_rows, o,
      {keys, key_cap, json, json_cap, R, totals}, {workspace, workspace_bytes, s}, "k_qc_keys",
      [&](unsigned grid, const EntScans& sc) {
        hipLaunchKernelGGL(k_qc_keys, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, o, sc, n_entries, R, keys,
                           totals);
      },
      "k_qc_json",
      [&](unsigned grid, const EntScans& sc) {
        hipLaunchKernelGGL(k_qc_json, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, rel, o, sc, n_entries, json,
                           totals);
      });
}

// ---- K17a on the host --------------------------------------------------------------------
extern "C" int avdb_qc_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                       const uint8_t* release, size_t release_len, uint64_t* ent_start,
                                       uint32_t* ent_alts, uint32_t* ent_key_bytes, uint32_t* ent_json_len,
                                       uint8_t* ent_flags, uint64_t* counts) {
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  return tables::table_size_host<QcBuild>(
      {"avdb_qc_table_size_host", ctx, {text, text_bytes, n_lines}, err}, o, counts, AVDB_QC_N_COUNTS,
      [&](size_t, const uint8_t* line, uint64_t len, bool nl, lof::Entry* E) {
        qc::Parsed Q = qc::parse_line(line, len, nl, true);
        *E = qc::entry_of(line, Q, rel);
        counts[AVDB_QC_COUNT_LONE_CR] += Q.b.lone_cr;
        counts[AVDB_QC_COUNT_COMMENT_LINES] += Q.b.cls == lof::kComment;
        return Q.b.cls == lof::kEntry;
      });
}

extern "C" int avdb_qc_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        size_t n_entries, size_t n_rows, const uint8_t* release, size_t release_len,
                                        const uint64_t* ent_start, const uint32_t* ent_alts,
                                        const uint32_t* ent_key_bytes, const uint32_t* ent_json_len,
                                        const uint8_t* ent_flags, uint8_t* keys, size_t key_cap, uint64_t* key_off,
                                        uint8_t* json, size_t json_cap, uint64_t* row_json_off, uint32_t* row_json_len,
                                        uint64_t* row_line_start, uint8_t* row_flags, uint64_t* totals) {
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  return tables::table_write_host<QcBuild>(
      {"avdb_qc_table_write_host", ctx, {text, text_bytes, n_lines}, err}, n_entries, n_rows, o,
      {keys, key_cap, json, json_cap, R, totals}, "JSON", [&](const EntryRow& E, auto put_key, auto put_json) {
        qc::render_entry_keys(text, text_bytes, E, R, put_key);
        qc::render_entry_json(text, text_bytes, E, rel, put_json);
      });
}

// ---- K17b's entries -------------------------------------------------------------------------
static const char* qc_table_view(const avdb_qc_table* t, Table* Q) {
  if (!t) return "null table";
  if (t->struct_size != sizeof(avdb_qc_table)) return "avdb_qc_table of another size";
  memset(Q, 0, sizeof(*Q));
  if (const char* err = release_view(t->release, t->release_len, &Q->rel)) return err;
  const char* err = tables::fill_table_view(&Q->t, t->n_rows, t->keys, t->key_off, t->keyset, t->keyset_bytes, t->json,
                                            t->json_bytes, t->json_off, t->json_len, t->hit, !t->flags);
  if (!err && t->n_rows) Q->row_flags = t->flags;
  return err;
}

extern "C" int avdb_qc_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const avdb_qc_table* table, uint32_t contig_mask, uint32_t flags,
                                   uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                                   uint8_t* row_flags, uint64_t* counts, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  Table T;
  const char* err = qc_table_view(table, &T);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t upd = (flags & AVDB_QCUPD_UPDATE_EXISTING) != 0;
  return tables::update_size<QcJoin>(
      {"avdb_qc_update_size", ctx, {text, text_bytes, n_lines}, err},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_QCUPD_N_COUNTS,
      {workspace, workspace_bytes, s}, "k_qcupd_lines",
      [&](unsigned grid, const uint64_t* starts, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        hipLaunchKernelGGL(k_qcupd_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, T,
                           contig_mask, upd, info, marks, cnt);
      });
}

extern "C" int avdb_qc_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    size_t n_rows, const avdb_qc_table* table, const uint64_t* row_start,
                                    const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                    const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                    uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  QcRows render{};
  const char* err = qc_table_view(table, &render.T);
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write<kQcJsonStage>({"avdb_qc_update_write", ctx, {text, text_bytes, n_lines}, err}, n_rows, o,
                                            {out, out_cap, row_off, totals},
                                            {workspace, workspace_bytes, static_cast<hipStream_t>(stream)}, render);
}

extern "C" int avdb_qc_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        const avdb_qc_table* table, uint32_t contig_mask, uint32_t flags,
                                        uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                                        uint8_t* row_flags, uint64_t* counts) {
  Table T;
  const char* err = qc_table_view(table, &T);
  const bool upd = (flags & AVDB_QCUPD_UPDATE_EXISTING) != 0;
  return tables::update_size_host<QcJoin>(
      {"avdb_qc_update_size_host", ctx, {text, text_bytes, n_lines}, err},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_QCUPD_N_COUNTS, err ? nullptr : T.t.hit,
      [&](const uint8_t* line, uint64_t len, bool nl) {
        return qc::scan_export_line(line, len, nl, contig_mask, upd, T);
      });
}

extern "C" int avdb_qc_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         size_t n_rows, const avdb_qc_table* table, const uint64_t* row_start,
                                         const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                         const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                         uint64_t* totals) {
  QcRows render{};
  const char* err = qc_table_view(table, &render.T);
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write_host({"avdb_qc_update_write_host", ctx, {text, text_bytes, n_lines}, err}, n_rows, o,
                                   {out, out_cap, row_off, totals}, render);
}
