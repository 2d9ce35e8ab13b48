// K17 — ADSP QC pVCF update rows from a VCF and an export of AnnotatedVDB.Variant (gfx950).
//
// Replaces the per-line Python of Load/bin/update_from_qc_pvcf_file.py (a VcfEntryParser with two
// dict comprehensions over INFO and to_numeric on every value, a ':'.join and a dict insert per alt
// allele, an xstr(dict) per hit, a bulk SQL lookup per 1,000 ids) with two device passes of two
// steps each, in K16's shape (avdb_lof.hip).
//   K17a, the table (avdb_qc_table_size / avdb_qc_table_write) over the QC VCF
//     k_qc_lines     one lane per line (lines::for_each_line: 256 lines' text staged in LDS): the
//                    first five fields, the bytes of QUAL .. FORMAT, INFO's keys, the length of
//                    the line's JSON and of its keys; 16 bytes of info and a mark per line
//     k_qc_compact   one lane per line: an entry's columns to its entry number; the counts
//     (the write entry: three exclusive scans; k_qc_totals: the totals against the capacities)
//     k_qc_keys      rows::write_rows over the key blob, one lane per entry
//     k_qc_json      rows::write_rows over the JSON blob, one lane per entry: INFO, FILTER, QUAL
//                    and FORMAT rendered as json.dumps prints what to_numeric makes of them
//   K17b, the update rows (avdb_qc_update_size / avdb_qc_update_write) over the export: K16b's
//   shape with the depth-1 key scan of the adsp_qc column in place of the NULL test
//     k_qcupd_lines, k_qcupd_compact, rows::begin_write, k_qcupd_write
// The per-line and per-row code is avdb_qc.hpp, shared with the _host entries.
#include "avdb_qc.hpp"
#include "avdb_rows.hpp"

#include <string.h>

namespace avdb {

using lof::EntryRow;
using lof::RowCols;
using qc::Release;
using qc::Table;
using qc::UpdLine;
using qc::UpdRow;

// A QC line without its sample columns is 150 to 300 bytes, its JSON about as long again; a line
// with sample columns is far longer, and a trip that does not fit 48 KB is read from global memory.
// 256 JSON texts of up to 256 bytes fit the 64 KB a workgroup can have; a trip that does not fit is
// written bytewise.
constexpr uint32_t kQcSizeStage = 48 * 1024;
constexpr uint32_t kQcKeyStage = 32 * 1024;
constexpr uint32_t kQcJsonStage = 64 * 1024;
constexpr uint32_t kQcUpdSizeStage = 48 * 1024;

struct QcEntCols {  // per entry, n_lines entries allocated
  uint64_t* start;
  uint32_t* alts;
  uint32_t* key_bytes;
  uint32_t* json_len;
  uint8_t* flags;
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

__global__ __launch_bounds__(kBlock) void k_qc_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                       size_t n_lines, const u32x4* __restrict__ info,
                                                       const uint64_t* __restrict__ ent_of, QcEntCols o,
                                                       unsigned long long* __restrict__ counts) {
  uint64_t rows = 0, kb = 0, jb = 0;
  uint32_t n_host = 0, n_bad = 0, n_pass = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 v = info[li];
    if ((v.w & 0xFFu) != lof::kEntry) continue;
    const uint64_t e = ent_of[li];  // e < n_lines: at most one entry per line (rows are numbered by the write pass)
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    const uint32_t flags = (v.w >> 8) & 0xFFu;
    o.start[e] = s;
    o.alts[e] = v.x;
    o.key_bytes[e] = v.y;
    o.json_len[e] = v.z;
    o.flags[e] = uint8_t(flags);
    rows += v.x;
    kb += v.y;
    jb += v.z;
    n_host += (flags & AVDB_QC_LINE_HOST) != 0;
    n_bad += (flags & AVDB_QC_LINE_BAD) != 0;
    n_pass += (flags & AVDB_QC_PASS) != 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[AVDB_QC_COUNT_ENTRIES] = ent_of[n_lines];
    counts[AVDB_QC_COUNT_LINES] = n_lines;
  }
  wave_add(&counts[AVDB_QC_COUNT_ROWS], rows);
  wave_add(&counts[AVDB_QC_COUNT_KEY_BYTES], kb);
  wave_add(&counts[AVDB_QC_COUNT_JSON_BYTES], jb);
  wave_add(&counts[AVDB_QC_COUNT_HOST_LINES], n_host);
  wave_add(&counts[AVDB_QC_COUNT_BAD], n_bad);
  wave_add(&counts[AVDB_QC_COUNT_PASS], n_pass);
}

struct QcEntScans {  // n_entries + 1 each
  uint64_t* row;
  uint64_t* key;
  uint64_t* json;
};

// the three totals against the capacities; totals[3]: 1 when they do not fit (nothing is written)
__global__ void k_qc_totals(QcEntCols o, QcEntScans sc, size_t n_entries, uint64_t n_rows, uint64_t key_cap,
                            uint64_t json_cap, uint64_t* __restrict__ key_off, uint64_t* __restrict__ totals) {
  if (blockIdx.x || threadIdx.x) return;
  uint64_t r = 0, k = 0, j = 0;
  if (n_entries) {
    r = sc.row[n_entries - 1] + o.alts[n_entries - 1];
    k = sc.key[n_entries - 1] + o.key_bytes[n_entries - 1];
    j = sc.json[n_entries - 1] + o.json_len[n_entries - 1];
  }
  sc.row[n_entries] = r;
  sc.key[n_entries] = k;
  sc.json[n_entries] = j;
  const bool over = k > key_cap || j > json_cap || r != n_rows;
  totals[0] = k;
  totals[1] = j;
  totals[2] = r;
  totals[3] = over;
  if (!over) key_off[n_rows] = k;
}

__device__ __forceinline__ EntryRow qc_load_entry(const QcEntCols& o, const QcEntScans& sc, size_t e) {
  return EntryRow{o.start[e], o.alts[e], o.key_bytes[e], o.json_len[e], o.flags[e], sc.row[e], sc.key[e], sc.json[e]};
}

__global__ __launch_bounds__(kBlock) void k_qc_keys(const uint8_t* __restrict__ text, size_t text_bytes, QcEntCols o,
                                                    QcEntScans sc, size_t n_entries, RowCols R,
                                                    uint8_t* __restrict__ keys, const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kQcKeyStage / 8];
  rows::write_rows<kQcKeyStage>(
      sc.key, n_entries, keys, totals + 2, s_out, [&](size_t e) { return qc_load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) { qc::render_entry_keys(text, text_bytes, E, R, put); });
}

__global__ __launch_bounds__(kBlock) void k_qc_json(const uint8_t* __restrict__ text, size_t text_bytes, Release rel,
                                                    QcEntCols o, QcEntScans sc, size_t n_entries,
                                                    uint8_t* __restrict__ json, const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kQcJsonStage / 8];
  rows::write_rows<kQcJsonStage>(
      sc.json, n_entries, json, totals + 2, s_out, [&](size_t e) { return qc_load_entry(o, sc, e); },
      [&](const EntryRow& E, auto put) { qc::render_entry_json(text, text_bytes, E, rel, put); });
}

// ---- K17b ---------------------------------------------------------------------------------
struct QcUpdCols {  // per row, n_lines entries allocated
  uint64_t* row_start;
  uint32_t* pk_len;
  int32_t* match;
  uint32_t* out_len;
  uint8_t* flags;
};

// info[li] = {pk_len, out_len, match, flags | is_row << 8}
__global__ __launch_bounds__(kBlock) void k_qcupd_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                        const uint64_t* __restrict__ starts, size_t n_lines, Table T,
                                                        uint32_t contig_mask, uint32_t update_existing,
                                                        u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kQcUpdSizeStage / 16];
  uint64_t n_cr = 0;
  uint32_t n_skip = 0, n_miss = 0;
  lines::for_each_line<kQcUpdSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const UpdLine L = qc::scan_export_line(line, len, nl, contig_mask, update_existing != 0, T);
      info[li] = u32x4{L.pk_len, L.out_len, uint32_t(L.row), L.flags | (L.is_row << 8)};
      mark[li] = L.is_row;
      if (L.row >= 0 && T.t.hit) T.t.hit[L.row] = 1;  // (every writer stores the same byte)
      n_cr += L.lone_cr;
      n_skip += L.skipped;
      n_miss += L.missed;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the row count there
  wave_add(&counts[AVDB_QCUPD_COUNT_LONE_CR], n_cr);
  wave_add(&counts[AVDB_QCUPD_COUNT_SKIPPED], n_skip);
  wave_add(&counts[AVDB_QCUPD_COUNT_NOT_IN_VCF], n_miss);
}

__global__ __launch_bounds__(kBlock) void k_qcupd_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                          size_t n_lines, const u32x4* __restrict__ info,
                                                          const uint64_t* __restrict__ row_of, QcUpdCols o,
                                                          unsigned long long* __restrict__ counts) {
  uint64_t bytes = 0;
  uint32_t n_bad = 0, n_host = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 v = info[li];
    if (!((v.w >> 8) & 1u)) continue;
    const uint64_t r = row_of[li];  // r < n_lines: at most one row per line
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    const uint32_t flags = v.w & 0xFFu;
    o.row_start[r] = s;
    o.pk_len[r] = v.x;
    o.out_len[r] = v.y;
    o.match[r] = int32_t(v.z);
    o.flags[r] = uint8_t(flags);
    bytes += v.y;
    n_bad += (flags & AVDB_QCUPD_BAD) != 0;
    n_host += (flags & AVDB_QCUPD_ROW_HOST) != 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // (k_qcupd_lines, which counts the skipped and the unmatched records, has finished)
    const uint64_t rows = row_of[n_lines];
    counts[AVDB_QCUPD_COUNT_ROWS] = rows;
    counts[AVDB_QCUPD_COUNT_SKIPPED_LINES] =
        n_lines - rows - counts[AVDB_QCUPD_COUNT_SKIPPED] - counts[AVDB_QCUPD_COUNT_NOT_IN_VCF];
  }
  wave_add(&counts[AVDB_QCUPD_COUNT_OUT_BYTES], bytes);
  wave_add(&counts[AVDB_QCUPD_COUNT_BAD], n_bad);
  wave_add(&counts[AVDB_QCUPD_COUNT_HOST_ROWS], n_host);
}

__global__ __launch_bounds__(kBlock) void k_qcupd_write(const uint8_t* __restrict__ text, size_t text_bytes, Table T,
                                                        QcUpdCols o, const uint64_t* __restrict__ row_off,
                                                        size_t n_rows, uint8_t* __restrict__ out,
                                                        const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kQcJsonStage / 8];
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  rows::write_rows<kQcJsonStage>(
      row_off, n_rows, out, totals, s_out,
      [&](size_t r) { return UpdRow{o.row_start[r], o.pk_len[r], o.out_len[r], o.flags[r], o.match[r]}; },
      [&](const UpdRow& row, auto put) { qc::render_update_row(row, T, tb, put); });
}

}  // namespace avdb

using namespace avdb;

// K17a's workspace: K16a's (16 bytes of info per line, three scanned arrays of n_entries + 1 offsets)
static rows::Layout qc_table_layout(size_t n_lines) { return rows::layout(n_lines, 16, 32); }
static rows::Layout qc_upd_layout(size_t n_lines) { return rows::layout(n_lines, 16); }

static QcEntScans qc_ent_scans(char* w, const rows::Layout& L, size_t n_lines) {
  auto* base = reinterpret_cast<uint64_t*>(w + L.extra);
  return QcEntScans{base, base + (n_lines + 1), base + 2 * (n_lines + 1)};
}

extern "C" int avdb_qc_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(qc_table_layout(n_lines).total, bytes);
}

extern "C" int avdb_qc_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(qc_upd_layout(n_lines).total, bytes);
}

static const char* release_view(const uint8_t* release, size_t release_len, Release* rel) {
  memset(rel, 0, sizeof(*rel));
  if (!qc::release_ok(release, release_len)) return "the release must be 1 .. 64 ASCII bytes without '\"', '\\' and control bytes";
  memcpy(rel->b, release, release_len);
  rel->n = uint32_t(release_len);
  return nullptr;
}

static const char* qc_table_size_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                       const QcEntCols& o, const uint64_t* counts) {
  if (!ctx || !counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!o.start || !o.alts || !o.key_bytes || !o.json_len || !o.flags)) return "null output array";
  return nullptr;
}

static const char* qc_table_write_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        size_t n_entries, size_t n_rows, const QcEntCols& o, const uint8_t* keys,
                                        size_t key_cap, const uint64_t* key_off, const uint8_t* json, size_t json_cap,
                                        const RowCols& R, const uint64_t* totals) {
  if (!ctx || !totals || !key_off) return "null argument";
  if (const char* err = rows::text_rows_error(text, text_bytes, n_lines, n_entries)) return err;
  if (n_rows >= 0x7FFFFFFFull) return "too many rows (rows are numbered in int32)";
  if (n_entries && (!o.start || !o.alts || !o.key_bytes || !o.json_len || !o.flags)) return "null entry array";
  if (n_rows && (!R.json_off || !R.json_len || !R.line_start || !R.flags)) return "null row array";
  if (const char* err = rows::out_error(keys, key_cap)) return err;
  return rows::out_error(json, json_cap);
}

extern "C" int avdb_qc_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                  const uint8_t* release, size_t release_len, uint64_t* ent_start, uint32_t* ent_alts,
                                  uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags, uint64_t* counts,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  const QcEntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  if (!err) err = qc_table_size_error(ctx, text, text_bytes, n_lines, o, counts);
  if (err) {
    avdb_set_error("avdb_qc_table_size: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = qc_table_layout(n_lines);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_qc_table_size", ctx, L.total, n_lines, workspace, workspace_bytes, counts,
                               AVDB_QC_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* info = reinterpret_cast<u32x4*>(w + L.info);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned grid = stream_grid(n_lines, kBlock, 4096);
  auto mark = [&](const uint64_t* starts, uint64_t* marks) {
    hipLaunchKernelGGL(k_qc_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, rel, info, marks,
                       cnt);
  };
  if (int e = lines::number_rows(text, text_bytes, n_lines, w, L, s, "k_qc_lines", mark)) return e;
  hipLaunchKernelGGL(k_qc_compact, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<const uint64_t*>(w + L.starts),
                     text_bytes, n_lines, info, reinterpret_cast<const uint64_t*>(w + L.row_of), o, cnt);
  AVDB_LAUNCH_CHECK("k_qc_compact");
  return AVDB_OK;
}

extern "C" int avdb_qc_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   size_t n_entries, size_t n_rows, const uint8_t* release, size_t release_len,
                                   const uint64_t* ent_start, const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                   const uint32_t* ent_json_len, const uint8_t* ent_flags, uint8_t* keys,
                                   size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                                   uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                                   uint8_t* row_flags, uint64_t* totals, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const QcEntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                    const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                    const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  if (!err)
    err = qc_table_write_error(ctx, text, text_bytes, n_lines, n_entries, n_rows, o, keys, key_cap, key_off, json,
                               json_cap, R, totals);
  if (err) {
    avdb_set_error("avdb_qc_table_write: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = qc_table_layout(n_lines);
  if (int e = n_lines ? lines::workspace_error("avdb_qc_table_write", L.total, workspace, workspace_bytes) : 0) return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_lines == 0) {  // no entries and no workspace: zero totals, or rows that nothing bears out
    AVDB_HIP_TRY(hipMemsetAsync(totals, 0, 32, s));
    AVDB_HIP_TRY(hipMemsetAsync(n_rows ? totals + 3 : key_off, n_rows ? 1 : 0, n_rows ? 1 : 8, s));
    return AVDB_OK;
  }
  char* w = static_cast<char*>(workspace);
  const QcEntScans sc = qc_ent_scans(w, L, n_lines);
  if (n_entries) {
    if (int e = scan::exclusive_u64(ent_alts, sc.row, n_entries, w + L.scan, L.scan_bytes, s)) return e;
    if (int e = scan::exclusive_u64(ent_key_bytes, sc.key, n_entries, w + L.scan, L.scan_bytes, s)) return e;
    if (int e = scan::exclusive_u64(ent_json_len, sc.json, n_entries, w + L.scan, L.scan_bytes, s)) return e;
  }
  hipLaunchKernelGGL(k_qc_totals, dim3(1), dim3(kWave), 0, s, o, sc, n_entries, uint64_t(n_rows), uint64_t(key_cap),
                     uint64_t(json_cap), key_off, totals);
  AVDB_LAUNCH_CHECK("k_qc_totals");
  if (n_entries == 0) return AVDB_OK;
  const unsigned grid = stream_grid(n_entries, kBlock, 2048);
  hipLaunchKernelGGL(k_qc_keys, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, o, sc, n_entries, R, keys, totals);
  AVDB_LAUNCH_CHECK("k_qc_keys");
  hipLaunchKernelGGL(k_qc_json, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, rel, o, sc, n_entries, json, totals);
  AVDB_LAUNCH_CHECK("k_qc_json");
  return AVDB_OK;
}

// ---- K17a on the host --------------------------------------------------------------------
extern "C" int avdb_qc_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                       const uint8_t* release, size_t release_len, uint64_t* ent_start,
                                       uint32_t* ent_alts, uint32_t* ent_key_bytes, uint32_t* ent_json_len,
                                       uint8_t* ent_flags, uint64_t* counts) {
  const QcEntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  if (!err) err = qc_table_size_error(ctx, text, text_bytes, n_lines, o, counts);
  if (err) {
    avdb_set_error("avdb_qc_table_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_QC_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  uint64_t n = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    bool nl;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e, &nl);
    qc::Parsed Q = qc::parse_line(text + s, e - s, nl, true);
    const lof::Entry E = qc::entry_of(text + s, Q, rel);
    counts[AVDB_QC_COUNT_LONE_CR] += Q.b.lone_cr;
    counts[AVDB_QC_COUNT_COMMENT_LINES] += Q.b.cls == lof::kComment;
    if (Q.b.cls != lof::kEntry) continue;
    ent_start[n] = s;
    ent_alts[n] = E.n_alts;
    ent_key_bytes[n] = E.key_bytes;
    ent_json_len[n] = E.json_len;
    ent_flags[n] = uint8_t(E.flags);
    ++n;
    counts[AVDB_QC_COUNT_ROWS] += E.n_alts;
    counts[AVDB_QC_COUNT_KEY_BYTES] += E.key_bytes;
    counts[AVDB_QC_COUNT_JSON_BYTES] += E.json_len;
    counts[AVDB_QC_COUNT_HOST_LINES] += (E.flags & AVDB_QC_LINE_HOST) != 0;
    counts[AVDB_QC_COUNT_BAD] += (E.flags & AVDB_QC_LINE_BAD) != 0;
    counts[AVDB_QC_COUNT_PASS] += (E.flags & AVDB_QC_PASS) != 0;
  }
  counts[AVDB_QC_COUNT_ENTRIES] = n;
  counts[AVDB_QC_COUNT_LINES] = n_lines;
  return AVDB_OK;
}

extern "C" int avdb_qc_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        size_t n_entries, size_t n_rows, const uint8_t* release, size_t release_len,
                                        const uint64_t* ent_start, const uint32_t* ent_alts,
                                        const uint32_t* ent_key_bytes, const uint32_t* ent_json_len,
                                        const uint8_t* ent_flags, uint8_t* keys, size_t key_cap, uint64_t* key_off,
                                        uint8_t* json, size_t json_cap, uint64_t* row_json_off, uint32_t* row_json_len,
                                        uint64_t* row_line_start, uint8_t* row_flags, uint64_t* totals) {
  const QcEntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                    const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                    const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  Release rel;
  const char* err = release_view(release, release_len, &rel);
  if (!err)
    err = qc_table_write_error(ctx, text, text_bytes, n_lines, n_entries, n_rows, o, keys, key_cap, key_off, json,
                               json_cap, R, totals);
  if (err) {
    avdb_set_error("avdb_qc_table_write_host: %s", err);
    return AVDB_EINVAL;
  }
  uint64_t r = 0, k = 0, j = 0;
  for (size_t e = 0; e < n_entries; ++e) {
    r += ent_alts[e];
    k += ent_key_bytes[e];
    j += ent_json_len[e];
  }
  const bool over = k > key_cap || j > json_cap || r != n_rows;
  totals[0] = k;
  totals[1] = j;
  totals[2] = r;
  totals[3] = over;
  if (over) {
    avdb_set_error("avdb_qc_table_write_host: %llu key bytes, %llu JSON bytes and %llu rows required",
                   (unsigned long long)k, (unsigned long long)j, (unsigned long long)r);
    return AVDB_ERANGE;
  }
  key_off[n_rows] = k;
  r = k = j = 0;
  for (size_t e = 0; e < n_entries; ++e) {
    const EntryRow E{ent_start[e], ent_alts[e], ent_key_bytes[e], ent_json_len[e], ent_flags[e], r, k, j};
    qc::render_entry_keys(text, text_bytes, E, R, [&](uint32_t i, uint32_t c) { keys[k + i] = uint8_t(c); });
    qc::render_entry_json(text, text_bytes, E, rel, [&](uint32_t i, uint32_t c) { json[j + i] = uint8_t(c); });
    r += E.alts;
    k += E.key_bytes;
    j += E.json_len;
  }
  return AVDB_OK;
}

// ---- K17b's entries -------------------------------------------------------------------------
static const char* qc_table_view(const avdb_qc_table* t, Table* Q) {
  if (!t) return "null table";
  if (t->struct_size != sizeof(avdb_qc_table)) return "avdb_qc_table of another size";
  memset(Q, 0, sizeof(*Q));
  if (const char* err = release_view(t->release, t->release_len, &Q->rel)) return err;
  if (t->n_rows >= 0x7FFFFFFFull) return "too many table rows";
  if (t->n_rows == 0) return nullptr;
  if (!t->keys || !t->key_off || !t->keyset || !t->json_off || !t->json_len || !t->flags || (t->json_bytes && !t->json))
    return "null table array";
  const uint64_t slots = keyset::slots(size_t(t->n_rows));
  if (t->keyset_bytes < slots * 12) return "key set smaller than avdb_keyset_workspace_size";
  lof::Table& T = Q->t;
  T.n_rows = t->n_rows;
  T.keys = t->keys;
  T.key_off = t->key_off;
  T.tkey = static_cast<const unsigned long long*>(t->keyset);
  T.tidx = reinterpret_cast<const uint32_t*>(T.tkey + slots);
  T.mask = slots - 1;
  T.json = t->json;
  T.json_bytes = t->json_bytes;
  T.json_off = t->json_off;
  T.json_len = t->json_len;
  T.hit = t->hit;
  Q->row_flags = t->flags;
  return nullptr;
}

static const char* qc_upd_size_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     const QcUpdCols& o, const uint64_t* counts) {
  if (!ctx || !counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!o.row_start || !o.pk_len || !o.match || !o.out_len || !o.flags)) return "null output array";
  return nullptr;
}

static const char* qc_upd_write_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                      size_t n_rows, const QcUpdCols& o, const uint8_t* out, size_t out_cap,
                                      const uint64_t* row_off, const uint64_t* totals) {
  if (!ctx || !totals || !row_off) return "null argument";
  if (const char* err = rows::text_rows_error(text, text_bytes, n_lines, n_rows)) return err;
  if (n_rows && (!o.row_start || !o.pk_len || !o.match || !o.out_len || !o.flags)) return "null row array";
  return rows::out_error(out, out_cap);
}

extern "C" int avdb_qc_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const avdb_qc_table* table, uint32_t contig_mask, uint32_t flags,
                                   uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                                   uint8_t* row_flags, uint64_t* counts, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  Table T;
  const QcUpdCols o{row_start, pk_len, match, out_len, row_flags};
  const char* err = qc_table_view(table, &T);
  if (!err) err = qc_upd_size_error(ctx, text, text_bytes, n_lines, o, counts);
  if (err) {
    avdb_set_error("avdb_qc_update_size: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = qc_upd_layout(n_lines);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_qc_update_size", ctx, L.total, n_lines, workspace, workspace_bytes, counts,
                               AVDB_QCUPD_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* info = reinterpret_cast<u32x4*>(w + L.info);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned grid = stream_grid(n_lines, kBlock, 4096);
  const uint32_t upd = (flags & AVDB_QCUPD_UPDATE_EXISTING) != 0;
  auto mark = [&](const uint64_t* starts, uint64_t* marks) {
    hipLaunchKernelGGL(k_qcupd_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, T, contig_mask,
                       upd, info, marks, cnt);
  };
  if (int e = lines::number_rows(text, text_bytes, n_lines, w, L, s, "k_qcupd_lines", mark)) return e;
  hipLaunchKernelGGL(k_qcupd_compact, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<const uint64_t*>(w + L.starts),
                     text_bytes, n_lines, info, reinterpret_cast<const uint64_t*>(w + L.row_of), o, cnt);
  AVDB_LAUNCH_CHECK("k_qcupd_compact");
  return AVDB_OK;
}

extern "C" int avdb_qc_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    size_t n_rows, const avdb_qc_table* table, const uint64_t* row_start,
                                    const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                    const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                    uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  Table T;
  const QcUpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                    const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const char* err = qc_table_view(table, &T);
  if (!err) err = qc_upd_write_error(ctx, text, text_bytes, n_lines, n_rows, o, out, out_cap, row_off, totals);
  if (err) {
    avdb_set_error("avdb_qc_update_write: %s", err);
    return AVDB_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_write("avdb_qc_update_write", ctx, qc_upd_layout(n_lines), n_lines, workspace, workspace_bytes,
                                out_len, n_rows, out_cap, row_off, totals, s))
    return e;
  if (n_rows == 0) return AVDB_OK;
  hipLaunchKernelGGL(k_qcupd_write, dim3(stream_grid(n_rows, kBlock, 2048)), dim3(kBlock), 0, s, text, text_bytes, T, o,
                     row_off, n_rows, out, totals);
  AVDB_LAUNCH_CHECK("k_qcupd_write");
  return AVDB_OK;
}

extern "C" int avdb_qc_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        const avdb_qc_table* table, uint32_t contig_mask, uint32_t flags,
                                        uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                                        uint8_t* row_flags, uint64_t* counts) {
  Table T;
  const QcUpdCols o{row_start, pk_len, match, out_len, row_flags};
  const char* err = qc_table_view(table, &T);
  if (!err) err = qc_upd_size_error(ctx, text, text_bytes, n_lines, o, counts);
  if (err) {
    avdb_set_error("avdb_qc_update_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_QCUPD_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  const bool upd = (flags & AVDB_QCUPD_UPDATE_EXISTING) != 0;
  uint64_t rows = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    bool nl;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e, &nl);
    const UpdLine L = qc::scan_export_line(text + s, e - s, nl, contig_mask, upd, T);
    counts[AVDB_QCUPD_COUNT_LONE_CR] += L.lone_cr;
    counts[AVDB_QCUPD_COUNT_SKIPPED] += L.skipped;
    counts[AVDB_QCUPD_COUNT_NOT_IN_VCF] += L.missed;
    if (L.row >= 0 && T.t.hit) T.t.hit[L.row] = 1;
    if (!L.is_row) continue;
    row_start[rows] = s;
    pk_len[rows] = L.pk_len;
    match[rows] = L.row;
    out_len[rows] = L.out_len;
    row_flags[rows] = uint8_t(L.flags);
    ++rows;
    counts[AVDB_QCUPD_COUNT_OUT_BYTES] += L.out_len;
    counts[AVDB_QCUPD_COUNT_BAD] += (L.flags & AVDB_QCUPD_BAD) != 0;
    counts[AVDB_QCUPD_COUNT_HOST_ROWS] += (L.flags & AVDB_QCUPD_ROW_HOST) != 0;
  }
  counts[AVDB_QCUPD_COUNT_ROWS] = rows;
  counts[AVDB_QCUPD_COUNT_SKIPPED_LINES] =
      n_lines - rows - counts[AVDB_QCUPD_COUNT_SKIPPED] - counts[AVDB_QCUPD_COUNT_NOT_IN_VCF];
  return AVDB_OK;
}

extern "C" int avdb_qc_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         size_t n_rows, const avdb_qc_table* table, const uint64_t* row_start,
                                         const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                         const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                         uint64_t* totals) {
  Table T;
  const QcUpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                    const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const char* err = qc_table_view(table, &T);
  if (!err) err = qc_upd_write_error(ctx, text, text_bytes, n_lines, n_rows, o, out, out_cap, row_off, totals);
  if (err) {
    avdb_set_error("avdb_qc_update_write_host: %s", err);
    return AVDB_EINVAL;
  }
  if (int e = rows::host_row_offsets("avdb_qc_update_write_host", out_len, n_rows, out_cap, row_off, totals)) return e;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (size_t r = 0; r < n_rows; ++r) {
    const UpdRow row{row_start[r], pk_len[r], out_len[r], row_flags[r], match[r]};
    const uint64_t off = row_off[r];
    qc::render_update_row(row, T, tb, [&](uint32_t k, uint32_t c) { out[off + k] = uint8_t(c); });
  }
  return AVDB_OK;
}
