// K13 — CADD update rows rendered from an export of AnnotatedVDB.Variant (gfx950).
//
// Replaces the per-record Python of the CADD pass around the K10 join
// (CADDUpdater.match_batch: a split, an int, two encodes and five appends per id;
// buffer_variants: a tuple, a dict and a json.dumps per record) with two passes over
// the export text (record_primary_key<TAB>metaseq_id<TAB>cadd_scores) on the device:
//   size pass (avdb_cadd_update_size)
//     (avdb_lines.hpp, shared with K10 and K12: one start per line, the marks scanned
//      into row numbers)
//     k_caddupd_lines    one lane per line (lines::for_each_line: 256 lines' text staged
//                        in LDS): the row rule, the skip, the metaseq id's four parts, the
//                        K10 join (cadd::match_rows, the alleles read where they lie in
//                        the export), the length of the row's text; 16 bytes of info and
//                        a mark per line
//     k_caddupd_compact  one lane per line: a row's columns to its row number; the counts
//   write pass (avdb_cadd_update_write)
//     (exclusive scan of the output lengths into row_off)
//     k_caddupd_totals   the total against the caller's capacity
//     k_caddupd_write    one workgroup per 256 rows: each lane renders its row into the
//                        workgroup's LDS stage (the scores rewritten from the table's own
//                        text, caddupd::score_text), then the trip's one contiguous span
//                        of the output is stored as aligned 8-byte words, one per lane
// The per-line and per-row code is avdb_caddupd.hpp, shared with the _host entries.
#include "avdb_caddupd.hpp"

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

// row_off[n_rows] = totals[0] = the bytes of all rows; totals[1]: 1 when they exceed cap
// (the write kernel then writes nothing)
__global__ void k_caddupd_totals(const uint32_t* __restrict__ out_len, uint64_t* __restrict__ row_off, size_t n_rows,
                                 uint64_t cap, uint64_t* __restrict__ totals) {
  if (blockIdx.x || threadIdx.x) return;
  const uint64_t t = n_rows ? row_off[n_rows - 1] + out_len[n_rows - 1] : 0ull;
  row_off[n_rows] = t;
  totals[0] = t;
  totals[1] = t > cap;
}

// The write pass stores about 90 bytes per row.  A lane storing its own row to global
// memory issues one store per byte or word with 64 different cache lines under it (what
// bounds K5's write pass).  Here a lane renders its row into LDS, at the place the row
// has in the trip's span of the output — the 256 rows of a trip own one contiguous span —
// and the span then goes out as aligned 8-byte words, lane i taking the i-th: a wave's
// store instruction covers 512 contiguous bytes.  Only the span's two edge words, shared
// with the neighbouring trips, are stored bytewise.
__global__ __launch_bounds__(kBlock) void k_caddupd_write(const uint8_t* __restrict__ text, size_t text_bytes,
                                                          Tables T, Chrom ch, UpdCols o,
                                                          const uint64_t* __restrict__ row_off, size_t n_rows,
                                                          uint8_t* __restrict__ out,
                                                          const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kUpdWriteStage / 8];
  if (totals[1]) return;  // the capacity is too small: nothing is written
  uint8_t* s_bytes = reinterpret_cast<uint8_t*>(s_out);
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (size_t r0 = size_t(blockIdx.x) * kBlock; r0 < n_rows; r0 += size_t(gridDim.x) * kBlock) {
    const uint32_t nr = n_rows - r0 < kBlock ? uint32_t(n_rows - r0) : uint32_t(kBlock);
    const uint64_t b = row_off[r0], e = row_off[r0 + nr], b8 = b & ~7ull;
    const bool staged = e >= b && e - b8 <= kUpdWriteStage;  // (workgroup-uniform)
    const uint32_t t = threadIdx.x;
    if (t < nr) {
      const size_t r = r0 + t;
      const uint64_t off = row_off[r];
      const Row row{o.row_start[r], o.pk_len[r], o.kind[r], o.out_len[r], o.flags[r], o.match[r]};
      // (off + k < off + out_len = row_off[r + 1] <= e: inside the span, and the stage)
      if (staged) {
        const uint32_t at = uint32_t(off - b8);
        caddupd::render_row(row, ch, T, tb, [&](uint32_t k, uint32_t c) { s_bytes[at + k] = uint8_t(c); });
      } else {
        caddupd::render_row(row, ch, T, tb, [&](uint32_t k, uint32_t c) { out[off + k] = uint8_t(c); });
      }
    }
    __syncthreads();
    if (staged) {
      for (uint64_t c = b8 + 8ull * t; c < e; c += 8ull * kBlock) {
        const uint32_t at = uint32_t(c - b8);
        if (c >= b && c + 8 <= e) {
          *reinterpret_cast<uint64_t*>(out + c) = s_out[at / 8];
        } else {
          const uint64_t lo = c > b ? c : b, hi = c + 8 < e ? c + 8 : e;
          for (uint64_t p = lo; p < hi; ++p) out[p] = s_bytes[uint32_t(p - b8)];
        }
      }
    }
    __syncthreads();  // the stage is reused by the next trip
  }
}

}  // namespace avdb

using namespace avdb;

// workspace: lines::Layout | line info | scan temp
struct UpdLayout : lines::Layout {
  size_t info, total;
};
static UpdLayout upd_layout(size_t n_lines) {
  UpdLayout L{lines::layout(n_lines)};
  L.info = L.next;
  L.scan = L.info + lines::pad256(16 * n_lines);
  L.scan_bytes = lines::pad256(scan::workspace_bytes(n_lines + 1));
  L.total = L.scan + L.scan_bytes;
  return L;
}

extern "C" int avdb_cadd_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  if (!bytes) return AVDB_EINVAL;
  *bytes = upd_layout(n_lines).total;
  return AVDB_OK;
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
  if (text_bytes && !text) return "null text";
  if (n_rows > n_lines || n_lines > text_bytes || n_lines >= 0x7FFFFFFFull) return "n_rows / n_lines out of range";
  if (n_rows && (!o.row_start || !o.pk_len || !o.kind || !o.match || !o.out_len || !o.flags)) return "null row array";
  if (out_cap && !out) return "null output";
  if (reinterpret_cast<uintptr_t>(out) % 8) return "the output must be 8-byte aligned";
  return nullptr;
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
  const UpdLayout L = upd_layout(n_lines);
  if (int e = n_lines ? lines::workspace_error("avdb_cadd_update_size", L.total, workspace, workspace_bytes) : 0)
    return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  AVDB_HIP_TRY(hipMemsetAsync(counts, 0, 8 * AVDB_CADDUPD_N_COUNTS, s));
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
  const UpdLayout L = upd_layout(n_lines);
  if (int e = n_lines ? lines::workspace_error("avdb_cadd_update_write", L.total, workspace, workspace_bytes) : 0)
    return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  if (n_rows)
    if (int e = scan::exclusive_u64(out_len, row_off, n_rows, w + L.scan, L.scan_bytes, s)) return e;
  hipLaunchKernelGGL(k_caddupd_totals, dim3(1), dim3(kWave), 0, s, out_len, row_off, n_rows, uint64_t(out_cap), totals);
  AVDB_LAUNCH_CHECK("k_caddupd_totals");
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
  uint64_t t = 0;
  for (size_t r = 0; r < n_rows; ++r) {
    row_off[r] = t;
    t += out_len[r];
  }
  row_off[n_rows] = t;
  totals[0] = t;
  totals[1] = t > out_cap;
  if (totals[1]) {
    avdb_set_error("avdb_cadd_update_write_host: output of %llu bytes required", (unsigned long long)t);
    return AVDB_ERANGE;
  }
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
