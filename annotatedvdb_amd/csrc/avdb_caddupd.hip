// K13 — CADD update rows rendered from an export of AnnotatedVDB.Variant (gfx950).
//
// Replaces the per-record Python of the CADD pass around the K10 join
// (CADDUpdater.match_batch: a split, an int, two encodes and five appends per id;
// buffer_variants: a tuple, a dict and a json.dumps per record) with two passes over
// the export text (record_primary_key<TAB>metaseq_id<TAB>cadd_scores) on the device:
//   size pass (avdb_cadd_update_size)
//     (avdb_lines.hpp, the front end shared with K10, K12 and K14: one start per line, the
//      marks scanned into row numbers; rows::begin_size)
//     k_caddupd_lines    one lane per line (lines::for_each_line: 256 lines' text staged
//                        in LDS): the row rule, the skip, the metaseq id's four parts, the
//                        K10 join (cadd::match_rows, the alleles read where they lie in
//                        the export), the length of the row's text; 16 bytes of info and
//                        a mark per line
//     k_caddupd_compact  one lane per line: a row's columns to its row number; the counts
//   write pass (avdb_cadd_update_write)
//     (avdb_rows.hpp, the back end shared with K12 and K14.  rows::begin_write: the
//      exclusive scan of the output lengths into row_off, k_row_totals: the total against
//      the caller's capacity)
//     k_caddupd_write    rows::write_rows, one workgroup per 256 rows: each lane renders its
//                        row into the workgroup's LDS stage (the scores rewritten from the
//                        table's own text, caddupd::score_text), then the trip's one
//                        contiguous span of the output is stored as aligned 8-byte words
// The per-line and per-row code is avdb_caddupd.hpp, shared with the _host entries.
#include "avdb_caddupd.hpp"
#include "avdb_rows.hpp"

#include <string.h>

namespace avdb {

using caddupd::Chrom;
using caddupd::Line;
using caddupd::Row;
using caddupd::Tables;

// Export lines run to about 100 bytes (a primary key, a metaseq id, \N or the 60 bytes
// of an earlier pass's JSON): 256 lines are 25 KB, staged in 32 KB.  An update row is
// about 90 bytes (the key, 'chr' + label, 55 bytes of JSON): the write pass stages a
// trip's 23 KB of output in 32 KB.  A trip that does not fit is read from, or written
// to, global memory bytewise.
constexpr uint32_t kUpdSizeStage = 32 * 1024;
constexpr uint32_t kUpdWriteStage = 32 * 1024;

struct UpdCols {  // per row, n_lines entries allocated
  uint64_t* row_start;
  uint32_t* pk_len;
  uint8_t* kind;
  int32_t* match;
  uint32_t* out_len;
  uint8_t* flags;
};

// info[li] = {pk_len, out_len, match, kind | flags << 8 | is_row << 16}
__global__ __launch_bounds__(kBlock) void k_caddupd_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                          const uint64_t* __restrict__ starts, size_t n_lines,
                                                          Tables T, Chrom ch, uint32_t contig_mask, uint32_t skip,
                                                          u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                          unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kUpdSizeStage / 16];
  uint64_t n_cr = 0;
  uint32_t n_skip = 0;
  lines::for_each_line<kUpdSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t s, uint64_t len, bool nl, auto line) {
      const Line L = caddupd::scan_line(line, text + s, len, nl, contig_mask, skip != 0, ch, T);
      info[li] = u32x4{L.pk_len, L.out_len, uint32_t(L.row), L.kind | (L.flags << 8) | (L.is_row << 16)};
      mark[li] = L.is_row;
      n_cr += L.lone_cr;
      n_skip += L.skipped;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the row count there
  wave_add(&counts[AVDB_CADDUPD_COUNT_LONE_CR], n_cr);
  wave_add(&counts[AVDB_CADDUPD_COUNT_SKIPPED], n_skip);
}

__global__ __launch_bounds__(kBlock) void k_caddupd_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                            size_t n_lines, const u32x4* __restrict__ info,
                                                            const uint64_t* __restrict__ row_of, UpdCols o,
                                                            unsigned long long* __restrict__ counts) {
  uint64_t bytes = 0;
  uint32_t n_snv = 0, n_indel = 0, n_none = 0, n_host = 0, n_bad = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 v = info[li];
    if (!((v.w >> 16) & 1u)) continue;
    const uint64_t r = row_of[li];  // r < n_lines: at most one row per line
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    const uint32_t kind = v.w & 0xFFu, flags = (v.w >> 8) & 0xFFu;
    o.row_start[r] = s;
    o.pk_len[r] = v.x;
    o.out_len[r] = v.y;
    o.match[r] = int32_t(v.z);
    o.kind[r] = uint8_t(kind);
    o.flags[r] = uint8_t(flags);
    bytes += v.y;
    n_host += (flags & AVDB_CADDUPD_ROW_HOST) != 0;
    n_bad += (flags & AVDB_CADDUPD_BAD) != 0;
    n_snv += !flags && kind == AVDB_CADD_SNV;
    n_indel += !flags && kind == AVDB_CADD_INDEL;
    n_none += !flags && kind == AVDB_CADD_NONE;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // (k_caddupd_lines, which counts the skipped records, has finished)
    const uint64_t rows = row_of[n_lines];
    counts[AVDB_CADDUPD_COUNT_ROWS] = rows;
    counts[AVDB_CADDUPD_COUNT_SKIPPED_LINES] = n_lines - rows - counts[AVDB_CADDUPD_COUNT_SKIPPED];
  }
  wave_add(&counts[AVDB_CADDUPD_COUNT_OUT_BYTES], bytes);
  wave_add(&counts[AVDB_CADDUPD_COUNT_SNV], n_snv);
  wave_add(&counts[AVDB_CADDUPD_COUNT_INDEL], n_indel);
  wave_add(&counts[AVDB_CADDUPD_COUNT_NOT_MATCHED], n_none);
  wave_add(&counts[AVDB_CADDUPD_COUNT_HOST_ROWS], n_host);
  wave_add(&counts[AVDB_CADDUPD_COUNT_BAD], n_bad);
}

// The write pass (rows::write_rows): a lane renders its row, the scores rewritten from the
// table's own text, into the workgroup's stage.
__global__ __launch_bounds__(kBlock) void k_caddupd_write(const uint8_t* __restrict__ text, size_t text_bytes,
                                                          Tables T, Chrom ch, UpdCols o,
                                                          const uint64_t* __restrict__ row_off, size_t n_rows,
                                                          uint8_t* __restrict__ out,
                                                          const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kUpdWriteStage / 8];
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  rows::write_rows<kUpdWriteStage>(
      row_off, n_rows, out, totals, s_out,
      [&](size_t r) { return Row{o.row_start[r], o.pk_len[r], o.kind[r], o.out_len[r], o.flags[r], o.match[r]}; },
      [&](const Row& row, auto put) { caddupd::render_row(row, ch, T, tb, put); });
}

}  // namespace avdb

using namespace avdb;

// workspace: rows::Layout with 16 bytes of info per line
static rows::Layout upd_layout(size_t n_lines) { return rows::layout(n_lines, 16); }

extern "C" int avdb_cadd_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(upd_layout(n_lines).total, bytes);
}

// the arguments both passes share: the tables and the chromosome text
static const char* shared_args_error(const void* ctx, const avdb_cadd_table* snv, const avdb_cadd_table* indel,
                                     const char* chrom, size_t chrom_len, Tables* T, Chrom* ch) {
  if (!ctx) return "null context";
  const char* err = nullptr;
  if (!cadd::table_view(snv, &T->snv, &err) || !cadd::table_view(indel, &T->indel, &err)) return err;
  T->snv_bytes = T->snv.n_rows ? snv->text_bytes : 0;
  T->indel_bytes = T->indel.n_rows ? indel->text_bytes : 0;
  memset(ch, 0, sizeof(*ch));
  if (chrom_len > caddupd::kChromMax) return "chromosome text longer than AVDB_CADDUPD_CHROM_MAX bytes";
  if (chrom_len && !chrom) return "null chromosome text";
  ch->len = uint32_t(chrom_len);
  if (chrom_len) memcpy(ch->text, chrom, chrom_len);
  return nullptr;
}

static const char* size_args_error(const uint8_t* text, size_t text_bytes, size_t n_lines, const UpdCols& o,
                                   const uint64_t* counts) {
  if (!counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!o.row_start || !o.pk_len || !o.kind || !o.match || !o.out_len || !o.flags)) return "null output array";
  return nullptr;
}

static const char* write_args_error(const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                                    const UpdCols& o, const uint8_t* out, size_t out_cap, const uint64_t* row_off,
                                    const uint64_t* totals) {
  if (!totals || !row_off) return "null argument";
  if (const char* err = rows::text_rows_error(text, text_bytes, n_lines, n_rows)) return err;
  if (n_rows && (!o.row_start || !o.pk_len || !o.kind || !o.match || !o.out_len || !o.flags)) return "null row array";
  return rows::out_error(out, out_cap);
}

extern "C" int avdb_cadd_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     const avdb_cadd_table* snv, const avdb_cadd_table* indel, const char* chrom,
                                     size_t chrom_len, uint32_t contig_mask, uint32_t flags, uint64_t* row_start,
                                     uint32_t* pk_len, uint8_t* kind, int32_t* match, uint32_t* out_len,
                                     uint8_t* row_flags, uint64_t* counts, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  Tables T;
  Chrom ch;
  const UpdCols o{row_start, pk_len, kind, match, out_len, row_flags};
  const char* err = shared_args_error(ctx, snv, indel, chrom, chrom_len, &T, &ch);
  if (!err) err = size_args_error(text, text_bytes, n_lines, o, counts);
  if (err) {
    avdb_set_error("avdb_cadd_update_size: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = upd_layout(n_lines);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_cadd_update_size", ctx, L.total, n_lines, workspace, workspace_bytes, counts,
                               AVDB_CADDUPD_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* info = reinterpret_cast<u32x4*>(w + L.info);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned grid = stream_grid(n_lines, kBlock, 4096);
  const uint32_t skip = (flags & AVDB_CADDUPD_SKIP_EXISTING) != 0;
  auto mark = [&](const uint64_t* starts, uint64_t* marks) {
    hipLaunchKernelGGL(k_caddupd_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, T, ch,
                       contig_mask, skip, info, marks, cnt);
  };
  if (int e = lines::number_rows(text, text_bytes, n_lines, w, L, s, "k_caddupd_lines", mark)) return e;
  hipLaunchKernelGGL(k_caddupd_compact, dim3(grid), dim3(kBlock), 0, s,
                     reinterpret_cast<const uint64_t*>(w + L.starts), text_bytes, n_lines, info,
                     reinterpret_cast<const uint64_t*>(w + L.row_of), o, cnt);
  AVDB_LAUNCH_CHECK("k_caddupd_compact");
  return AVDB_OK;
}

extern "C" int avdb_cadd_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                      size_t n_rows, const avdb_cadd_table* snv, const avdb_cadd_table* indel,
                                      const char* chrom, size_t chrom_len, const uint64_t* row_start,
                                      const uint32_t* pk_len, const uint8_t* kind, const int32_t* match,
                                      const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                                      uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  Tables T;
  Chrom ch;
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<uint8_t*>(kind),
                  const_cast<int32_t*>(match),      const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const char* err = shared_args_error(ctx, snv, indel, chrom, chrom_len, &T, &ch);
  if (!err) err = write_args_error(text, text_bytes, n_lines, n_rows, o, out, out_cap, row_off, totals);
  if (err) {
    avdb_set_error("avdb_cadd_update_write: %s", err);
    return AVDB_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_write("avdb_cadd_update_write", ctx, upd_layout(n_lines), n_lines, workspace, workspace_bytes,
                                out_len, n_rows, out_cap, row_off, totals, s))
    return e;
  if (n_rows == 0) return AVDB_OK;
  hipLaunchKernelGGL(k_caddupd_write, dim3(stream_grid(n_rows, kBlock, 2048)), dim3(kBlock), 0, s, text, text_bytes, T,
                     ch, o, row_off, n_rows, out, totals);
  AVDB_LAUNCH_CHECK("k_caddupd_write");
  return AVDB_OK;
}

// ---- the same code on the host ------------------------------------------------
extern "C" int avdb_cadd_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          const avdb_cadd_table* snv, const avdb_cadd_table* indel, const char* chrom,
                                          size_t chrom_len, uint32_t contig_mask, uint32_t flags, uint64_t* row_start,
                                          uint32_t* pk_len, uint8_t* kind, int32_t* match, uint32_t* out_len,
                                          uint8_t* row_flags, uint64_t* counts) {
  Tables T;
  Chrom ch;
  const UpdCols o{row_start, pk_len, kind, match, out_len, row_flags};
  const char* err = shared_args_error(ctx, snv, indel, chrom, chrom_len, &T, &ch);
  if (!err) err = size_args_error(text, text_bytes, n_lines, o, counts);
  if (err) {
    avdb_set_error("avdb_cadd_update_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_CADDUPD_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  const bool skip = (flags & AVDB_CADDUPD_SKIP_EXISTING) != 0;
  uint64_t rows = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    bool nl;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e, &nl);
    const Line L = caddupd::scan_line(text + s, text + s, e - s, nl, contig_mask, skip, ch, T);
    counts[AVDB_CADDUPD_COUNT_LONE_CR] += L.lone_cr;
    counts[AVDB_CADDUPD_COUNT_SKIPPED] += L.skipped;
    if (!L.is_row) continue;
    row_start[rows] = s;
    pk_len[rows] = L.pk_len;
    kind[rows] = uint8_t(L.kind);
    match[rows] = L.row;
    out_len[rows] = L.out_len;
    row_flags[rows] = uint8_t(L.flags);
    ++rows;
    counts[AVDB_CADDUPD_COUNT_OUT_BYTES] += L.out_len;
    counts[AVDB_CADDUPD_COUNT_HOST_ROWS] += (L.flags & AVDB_CADDUPD_ROW_HOST) != 0;
    counts[AVDB_CADDUPD_COUNT_BAD] += (L.flags & AVDB_CADDUPD_BAD) != 0;
    if (!L.flags)
      ++counts[L.kind == AVDB_CADD_SNV     ? AVDB_CADDUPD_COUNT_SNV
               : L.kind == AVDB_CADD_INDEL ? AVDB_CADDUPD_COUNT_INDEL
                                           : AVDB_CADDUPD_COUNT_NOT_MATCHED];
  }
  counts[AVDB_CADDUPD_COUNT_ROWS] = rows;
  counts[AVDB_CADDUPD_COUNT_SKIPPED_LINES] = n_lines - rows - counts[AVDB_CADDUPD_COUNT_SKIPPED];
  return AVDB_OK;
}

extern "C" int avdb_cadd_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                           size_t n_rows, const avdb_cadd_table* snv, const avdb_cadd_table* indel,
                                           const char* chrom, size_t chrom_len, const uint64_t* row_start,
                                           const uint32_t* pk_len, const uint8_t* kind, const int32_t* match,
                                           const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                                           size_t out_cap, uint64_t* row_off, uint64_t* totals) {
  Tables T;
  Chrom ch;
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<uint8_t*>(kind),
                  const_cast<int32_t*>(match),      const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const char* err = shared_args_error(ctx, snv, indel, chrom, chrom_len, &T, &ch);
  if (!err) err = write_args_error(text, text_bytes, n_lines, n_rows, o, out, out_cap, row_off, totals);
  if (err) {
    avdb_set_error("avdb_cadd_update_write_host: %s", err);
    return AVDB_EINVAL;
  }
  if (int e = rows::host_row_offsets("avdb_cadd_update_write_host", out_len, n_rows, out_cap, row_off, totals)) return e;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (size_t r = 0; r < n_rows; ++r) {
    const Row row{row_start[r], pk_len[r], kind[r], out_len[r], row_flags[r], match[r]};
    const uint64_t off = row_off[r];
    caddupd::render_row(row, ch, T, tb, [&](uint32_t k, uint32_t c) { out[off + k] = uint8_t(c); });
  }
  return AVDB_OK;
}

// json.dumps(float(text)) of one score text: its bytes to out (cap >= AVDB_CADDUPD_SCORE_MAX),
// *len its length; returns 1, or 0 for a text the device does not render
extern "C" int avdb_cadd_score_text_host(const uint8_t* text, size_t n, uint8_t* out, size_t cap, size_t* len) {
  if ((n && !text) || !out || !len || cap < AVDB_CADDUPD_SCORE_MAX) {
    avdb_set_error("avdb_cadd_score_text_host: null argument, or an output of fewer than %d bytes",
                   AVDB_CADDUPD_SCORE_MAX);
    return AVDB_EINVAL;
  }
  *len = 0;
  if (n >= 0x7FFFFFFFull) return 0;
  const uint32_t k = caddupd::score_text(text, uint32_t(n), [&](uint32_t j, uint32_t c) {
    if (j < cap) out[j] = uint8_t(c);
  });
  *len = k;
  return k ? 1 : 0;
}
