// K14 — the per-chromosome VCF files of an export of AnnotatedVDB.Variant (gfx950).
//
// Replaces the per-record Python of Util/bin/export_variant2vcf.py (run: a RealDictCursor
// dict, a regex search and a dict insert per record; print_file: a split and an
// eight-field print per record) with two passes over the export text
// (record_primary_key<TAB>metaseq_id<TAB>row_algorithm_id) on the device:
//   size pass (avdb_export_vcf_size)
//     (avdb_lines.hpp, the front end shared with K10, K12 and K13: one start per line; the two
//      marks of a line, valid and invalid, share one 64-bit word, so one scan numbers both
//      lists; rows::begin_size)
//     k_expvcf_lines     one lane per line (lines::for_each_line: 256 lines' text staged in
//                        LDS): the row rule, the class, the lengths, K6's hash of the key;
//                        16 bytes of info, the hash and a mark per line
//     k_expvcf_compact   one lane per line: a row's columns to its number in its list; the counts
//   write pass (avdb_export_vcf_write, once per stream over its own row list)
//     (avdb_rows.hpp, the back end shared with K12 and K13.  rows::begin_write: the exclusive
//      scan of the output lengths into row_off, k_row_totals: the total against the caller's
//      capacity)
//     k_expvcf_write     rows::write_rows, one workgroup per 256 rows: each lane renders its
//                        row into the workgroup's LDS stage, then the trip's one contiguous
//                        span of the output is stored as aligned 8-byte words, one per lane
// The per-line and per-row code is avdb_expvcf.hpp, shared with the _host entries.
#include "avdb_expvcf.hpp"
#include "avdb_rows.hpp"

#include <string.h>

namespace avdb {

using expvcf::Line;
using expvcf::Row;

// Export lines run to about 60 bytes (a primary key, a metaseq id, an algorithm id), to
// about 110 with digest-form keys: 256 lines are 15 to 28 KB, staged in 32 KB.  A VCF row
// is its key and its metaseq id and 8 bytes more, an invalid row shorter: the write pass
// stages a trip's output in 32 KB.  Four workgroups' stages fit a CU's 160 KB.  A trip
// that does not fit is read from, or written to, global memory bytewise.
constexpr uint32_t kVcfSizeStage = 32 * 1024;
constexpr uint32_t kVcfWriteStage = 32 * 1024;

struct VcfCols {  // the valid rows' list, n_lines entries allocated
  uint64_t* row_start;
  uint32_t *pk_len, *ms_len, *out_len;
  uint8_t* flags;
  uint64_t* pk_hash;
};

struct InvCols {  // the invalid rows' list, n_lines entries allocated
  uint64_t* row_start;
  uint32_t *pk_len, *out_len;
};

// info[li] = {pk_len, ms_len, out_len, flags | class << 8}; mark[li] = valid | invalid << 32
__global__ __launch_bounds__(kBlock) void k_expvcf_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                         const uint64_t* __restrict__ starts, size_t n_lines,
                                                         uint32_t contig_mask, u32x4* __restrict__ info,
                                                         uint64_t* __restrict__ hash, uint64_t* __restrict__ mark,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kVcfSizeStage / 16];
  uint64_t n_cr = 0;
  uint32_t n_filtered = 0;
  lines::for_each_line<kVcfSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const Line L = expvcf::scan_line(line, len, nl, contig_mask);
      info[li] = u32x4{L.pk_len, L.ms_len, L.out_len, L.flags | (L.cls << 8)};
      hash[li] = L.pk_hash;
      mark[li] = uint64_t(L.cls == expvcf::kValid) | (uint64_t(L.cls == expvcf::kInvalid) << 32);
      n_cr += L.lone_cr;
      n_filtered += L.filtered;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the two row counts there
  wave_add(&counts[AVDB_EXPVCF_COUNT_LONE_CR], n_cr);
  wave_add(&counts[AVDB_EXPVCF_COUNT_FILTERED], n_filtered);
}

__global__ __launch_bounds__(kBlock) void k_expvcf_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                           size_t n_lines, const u32x4* __restrict__ info,
                                                           const uint64_t* __restrict__ hash,
                                                           const uint64_t* __restrict__ row_of, VcfCols v, InvCols iv,
                                                           unsigned long long* __restrict__ counts) {
  uint64_t vcf_bytes = 0, inv_bytes = 0;
  uint32_t n_bad = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 x = info[li];
    const uint32_t cls = (x.w >> 8) & 0xFFu, flags = x.w & 0xFFu;
    if (!cls) continue;
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    // (both halves of row_of[li] are below n_lines: at most one row per line)
    if (cls == expvcf::kValid) {
      const uint64_t r = row_of[li] & 0xFFFFFFFFull;
      v.row_start[r] = s;
      v.pk_len[r] = x.x;
      v.ms_len[r] = x.y;
      v.out_len[r] = x.z;
      v.flags[r] = uint8_t(flags);
      v.pk_hash[r] = hash[li];
      vcf_bytes += x.z;
      n_bad += (flags & AVDB_EXPVCF_BAD) != 0;
    } else {
      const uint64_t r = row_of[li] >> 32;
      iv.row_start[r] = s;
      iv.pk_len[r] = x.x;
      iv.out_len[r] = x.z;
      inv_bytes += x.z;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // (k_expvcf_lines, which counts the filtered lines, has finished)
    const uint64_t valid = row_of[n_lines] & 0xFFFFFFFFull, invalid = row_of[n_lines] >> 32;
    counts[AVDB_EXPVCF_COUNT_VALID] = valid;
    counts[AVDB_EXPVCF_COUNT_INVALID] = invalid;
    counts[AVDB_EXPVCF_COUNT_SKIPPED_LINES] = n_lines - valid - invalid - counts[AVDB_EXPVCF_COUNT_FILTERED];
  }
  wave_add(&counts[AVDB_EXPVCF_COUNT_VCF_BYTES], vcf_bytes);
  wave_add(&counts[AVDB_EXPVCF_COUNT_INVALID_BYTES], inv_bytes);
  wave_add(&counts[AVDB_EXPVCF_COUNT_BAD], n_bad);
}

// The write pass of either stream (rows::write_rows).  kInvalidStream: the rows are the
// invalid file's (ms_len and flags are not read).
template <bool kInvalidStream>
__global__ __launch_bounds__(kBlock) void k_expvcf_write(const uint8_t* __restrict__ text, size_t text_bytes,
                                                         const uint64_t* __restrict__ row_start,
                                                         const uint32_t* __restrict__ pk_len,
                                                         const uint32_t* __restrict__ ms_len,
                                                         const uint32_t* __restrict__ out_len,
                                                         const uint8_t* __restrict__ flags,
                                                         const uint64_t* __restrict__ row_off, size_t n_rows,
                                                         uint8_t* __restrict__ out,
                                                         const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kVcfWriteStage / 8];
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  rows::write_rows<kVcfWriteStage>(
      row_off, n_rows, out, totals, s_out,
      [&](size_t r) {
        Row row{row_start[r], pk_len[r], 0, out_len[r], 0};
        if constexpr (!kInvalidStream) {
          row.ms_len = ms_len[r];
          row.flags = flags[r];
        }
        return row;
      },
      [&](const Row& row, auto put) {
        if constexpr (kInvalidStream)
          expvcf::render_invalid_row(row, text_bytes, tb, put);
        else
          expvcf::render_vcf_row(row, tb, put);
      });
}

}  // namespace avdb

using namespace avdb;

// workspace: rows::Layout with 16 bytes of info and the 8 of the key's hash per line
static rows::Layout vcf_layout(size_t n_lines) { return rows::layout(n_lines, 16, 8); }

extern "C" int avdb_export_vcf_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(vcf_layout(n_lines).total, bytes);
}

static const char* size_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const VcfCols& v, const InvCols& iv, const uint64_t* counts) {
  if (!ctx) return "null context";
  if (!counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!v.row_start || !v.pk_len || !v.ms_len || !v.out_len || !v.flags || !v.pk_hash || !iv.row_start ||
                  !iv.pk_len || !iv.out_len))
    return "null output array";
  return nullptr;
}

static const char* write_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    uint32_t which, size_t n_rows, const uint64_t* row_start, const uint32_t* pk_len,
                                    const uint32_t* ms_len, const uint32_t* out_len, const uint8_t* row_flags,
                                    const uint8_t* out, size_t out_cap, const uint64_t* row_off,
                                    const uint64_t* totals) {
  if (!ctx) return "null context";
  if (!totals || !row_off) return "null argument";
  if (which != AVDB_EXPVCF_STREAM_VCF && which != AVDB_EXPVCF_STREAM_INVALID) return "no such stream";
  if (const char* err = rows::text_rows_error(text, text_bytes, n_lines, n_rows)) return err;
  if (n_rows && (!row_start || !pk_len || !out_len)) return "null row array";
  if (n_rows && which == AVDB_EXPVCF_STREAM_VCF && (!ms_len || !row_flags)) return "null row array";
  return rows::out_error(out, out_cap);
}

extern "C" int avdb_export_vcf_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    uint32_t contig_mask, uint64_t* row_start, uint32_t* pk_len, uint32_t* ms_len,
                                    uint32_t* out_len, uint8_t* row_flags, uint64_t* pk_hash, uint64_t* inv_start,
                                    uint32_t* inv_pk_len, uint32_t* inv_out_len, uint64_t* counts, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const VcfCols v{row_start, pk_len, ms_len, out_len, row_flags, pk_hash};
  const InvCols iv{inv_start, inv_pk_len, inv_out_len};
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, v, iv, counts)) {
    avdb_set_error("avdb_export_vcf_size: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = vcf_layout(n_lines);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_export_vcf_size", ctx, L.total, n_lines, workspace, workspace_bytes, counts,
                               AVDB_EXPVCF_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* info = reinterpret_cast<u32x4*>(w + L.info);
  auto* hash = reinterpret_cast<uint64_t*>(w + L.extra);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned grid = stream_grid(n_lines, kBlock, 4096);
  auto mark = [&](const uint64_t* starts, uint64_t* marks) {
    hipLaunchKernelGGL(k_expvcf_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, contig_mask,
                       info, hash, marks, cnt);
  };
  if (int e = lines::number_rows(text, text_bytes, n_lines, w, L, s, "k_expvcf_lines", mark)) return e;
  hipLaunchKernelGGL(k_expvcf_compact, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<const uint64_t*>(w + L.starts),
                     text_bytes, n_lines, info, hash, reinterpret_cast<const uint64_t*>(w + L.row_of), v, iv, cnt);
  AVDB_LAUNCH_CHECK("k_expvcf_compact");
  return AVDB_OK;
}

extern "C" int avdb_export_vcf_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     uint32_t which, size_t n_rows, const uint64_t* row_start, const uint32_t* pk_len,
                                     const uint32_t* ms_len, const uint32_t* out_len, const uint8_t* row_flags,
                                     uint8_t* out, size_t out_cap, uint64_t* row_off, uint64_t* totals,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, which, n_rows, row_start, pk_len, ms_len,
                                         out_len, row_flags, out, out_cap, row_off, totals)) {
    avdb_set_error("avdb_export_vcf_write: %s", err);
    return AVDB_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_write("avdb_export_vcf_write", ctx, vcf_layout(n_lines), n_lines, workspace, workspace_bytes,
                                out_len, n_rows, out_cap, row_off, totals, s))
    return e;
  if (n_rows == 0) return AVDB_OK;
  const dim3 grid(stream_grid(n_rows, kBlock, 2048));
  if (which == AVDB_EXPVCF_STREAM_VCF)
    hipLaunchKernelGGL(k_expvcf_write<false>, grid, dim3(kBlock), 0, s, text, text_bytes, row_start, pk_len, ms_len,
                       out_len, row_flags, row_off, n_rows, out, totals);
  else
    hipLaunchKernelGGL(k_expvcf_write<true>, grid, dim3(kBlock), 0, s, text, text_bytes, row_start, pk_len, ms_len,
                       out_len, row_flags, row_off, n_rows, out, totals);
  AVDB_LAUNCH_CHECK("k_expvcf_write");
  return AVDB_OK;
}

// ---- the same code on the host ------------------------------------------------
extern "C" int avdb_export_vcf_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         uint32_t contig_mask, uint64_t* row_start, uint32_t* pk_len, uint32_t* ms_len,
                                         uint32_t* out_len, uint8_t* row_flags, uint64_t* pk_hash, uint64_t* inv_start,
                                         uint32_t* inv_pk_len, uint32_t* inv_out_len, uint64_t* counts) {
  const VcfCols v{row_start, pk_len, ms_len, out_len, row_flags, pk_hash};
  const InvCols iv{inv_start, inv_pk_len, inv_out_len};
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, v, iv, counts)) {
    avdb_set_error("avdb_export_vcf_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_EXPVCF_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  uint64_t valid = 0, invalid = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    bool nl;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e, &nl);
    const Line L = expvcf::scan_line(text + s, e - s, nl, contig_mask);
    counts[AVDB_EXPVCF_COUNT_LONE_CR] += L.lone_cr;
    counts[AVDB_EXPVCF_COUNT_FILTERED] += L.filtered;
    if (L.cls == expvcf::kValid) {
      row_start[valid] = s;
      pk_len[valid] = L.pk_len;
      ms_len[valid] = L.ms_len;
      out_len[valid] = L.out_len;
      row_flags[valid] = uint8_t(L.flags);
      pk_hash[valid] = L.pk_hash;
      ++valid;
      counts[AVDB_EXPVCF_COUNT_VCF_BYTES] += L.out_len;
      counts[AVDB_EXPVCF_COUNT_BAD] += (L.flags & AVDB_EXPVCF_BAD) != 0;
    } else if (L.cls == expvcf::kInvalid) {
      inv_start[invalid] = s;
      inv_pk_len[invalid] = L.pk_len;
      inv_out_len[invalid] = L.out_len;
      ++invalid;
      counts[AVDB_EXPVCF_COUNT_INVALID_BYTES] += L.out_len;
    }
  }
  counts[AVDB_EXPVCF_COUNT_VALID] = valid;
  counts[AVDB_EXPVCF_COUNT_INVALID] = invalid;
  counts[AVDB_EXPVCF_COUNT_SKIPPED_LINES] = n_lines - valid - invalid - counts[AVDB_EXPVCF_COUNT_FILTERED];
  return AVDB_OK;
}

extern "C" int avdb_export_vcf_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          uint32_t which, size_t n_rows, const uint64_t* row_start,
                                          const uint32_t* pk_len, const uint32_t* ms_len, const uint32_t* out_len,
                                          const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                          uint64_t* totals) {
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, which, n_rows, row_start, pk_len, ms_len,
                                         out_len, row_flags, out, out_cap, row_off, totals)) {
    avdb_set_error("avdb_export_vcf_write_host: %s", err);
    return AVDB_EINVAL;
  }
  if (int e = rows::host_row_offsets("avdb_export_vcf_write_host", out_len, n_rows, out_cap, row_off, totals)) return e;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (size_t r = 0; r < n_rows; ++r) {
    const uint64_t off = row_off[r];
    auto put = [&](uint32_t k, uint32_t c) { out[off + k] = uint8_t(c); };
    if (which == AVDB_EXPVCF_STREAM_VCF)
      expvcf::render_vcf_row(Row{row_start[r], pk_len[r], ms_len[r], out_len[r], row_flags[r]}, tb, put);
    else
      expvcf::render_invalid_row(Row{row_start[r], pk_len[r], 0, out_len[r], 0}, text_bytes, tb, put);
  }
  return AVDB_OK;
}
