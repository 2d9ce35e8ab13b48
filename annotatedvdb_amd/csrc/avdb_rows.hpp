// The back end of the two-pass exports over a text slab (K12, avdb_existing.hip; K13,
// avdb_caddupd.hip; K14, avdb_expvcf.hip; K15, avdb_splitvcf.hip), behind the front end of
// avdb_lines.hpp: the workspace of a size pass and a write pass, the entries' prologues and the
// argument checks they share, a stream's offsets and totals on the device (k_row_totals) and on the
// host (host_row_offsets), and the write pass of rows rendered per lane (write_rows: a trip's rows
// staged in LDS, its span of the output stored as aligned 8-byte words).  Compiled for both sides,
// as avdb_lines.hpp is.
#pragma once

#include "avdb_lines.hpp"

namespace avdb {
namespace rows {

// workspace: lines::Layout | info_bytes of info per line | extra_bytes more per line | scan temp
// (of the row numbering, n_lines + 1 marks, or of the write pass's scan_arrays length arrays of up
// to n_lines rows, whichever is larger)
struct Layout : lines::Layout {
  size_t info, extra, total;
};
inline Layout layout(size_t n_lines, size_t info_bytes, size_t extra_bytes = 0, int scan_arrays = 1) {
  Layout L{lines::layout(n_lines)};
  L.info = L.next;
  L.extra = L.info + lines::pad256(info_bytes * n_lines);
  L.scan = extra_bytes ? L.extra + lines::pad256(extra_bytes * n_lines) : L.extra;
  const size_t a = scan::workspace_bytes(n_lines + 1), b = scan::workspace_bytes(n_lines, scan_arrays);
  L.scan_bytes = lines::pad256(a > b ? a : b);
  L.total = L.scan + L.scan_bytes;
  return L;
}

// what a *_workspace_size entry returns
inline int workspace_size(size_t total, size_t* bytes) {
  if (!bytes) return AVDB_EINVAL;
  *bytes = total;
  return AVDB_OK;
}

// the checks the write entries share; an entry's own null-array checks go between the two
inline const char* text_rows_error(const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows) {
  if (text_bytes && !text) return "null text";
  if (n_rows > n_lines || n_lines > text_bytes || n_lines >= 0x7FFFFFFFull) return "n_rows / n_lines out of range";
  return nullptr;
}
inline const char* out_error(const uint8_t* out, size_t out_cap) {
  if (out_cap && !out) return "null output";
  if (reinterpret_cast<uintptr_t>(out) % 8) return "the output must be 8-byte aligned";
  return nullptr;
}

// A size entry after its argument checks: the workspace of `total` bytes (none is needed
// for no lines), the device, the first n_counts counts zeroed.
inline int begin_size(const char* fn, const avdb_ctx* ctx, size_t total, size_t n_lines, const void* workspace,
                      size_t workspace_bytes, uint64_t* counts, size_t n_counts, hipStream_t s) {
  if (int e = n_lines ? lines::workspace_error(fn, total, workspace, workspace_bytes) : 0) return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  AVDB_HIP_TRY(hipMemsetAsync(counts, 0, 8 * n_counts, s));
  return AVDB_OK;
}

// row_off[n_rows] = totals[0] = the bytes of all rows; totals[1]: 1 when they exceed cap
// (the write kernel then writes nothing)
template <class T>
__global__ void k_row_totals(const T* __restrict__ out_len, uint64_t* __restrict__ row_off, size_t n_rows, uint64_t cap,
                             uint64_t* __restrict__ totals) {
  if (blockIdx.x || threadIdx.x) return;
  const uint64_t t = n_rows ? row_off[n_rows - 1] + out_len[n_rows - 1] : 0ull;
  row_off[n_rows] = t;
  totals[0] = t;
  totals[1] = t > cap;
}

// A single-stream write entry after its argument checks: the workspace, the device, the
// exclusive scan of out_len into row_off, the totals.
inline int begin_write(const char* fn, const avdb_ctx* ctx, const Layout& L, size_t n_lines, void* workspace,
                       size_t workspace_bytes, const uint32_t* out_len, size_t n_rows, size_t out_cap,
                       uint64_t* row_off, uint64_t* totals, hipStream_t s) {
  if (int e = n_lines ? lines::workspace_error(fn, L.total, workspace, workspace_bytes) : 0) return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  if (n_rows)
    if (int e = scan::exclusive_u64(out_len, row_off, n_rows, static_cast<char*>(workspace) + L.scan, L.scan_bytes, s))
      return e;
  hipLaunchKernelGGL(k_row_totals<uint32_t>, dim3(1), dim3(kWave), 0, s, out_len, row_off, n_rows, uint64_t(out_cap),
                     totals);
  AVDB_LAUNCH_CHECK("k_row_totals");
  return AVDB_OK;
}

// the same on the host: off[0 .. n_rows] = the exclusive sums of len, *total their sum;
// whether it exceeds cap
inline bool host_offsets(const uint32_t* len, size_t n_rows, uint64_t cap, uint64_t* off, uint64_t* total) {
  uint64_t t = 0;
  for (size_t r = 0; r < n_rows; ++r) {
    off[r] = t;
    t += len[r];
  }
  off[n_rows] = t;
  *total = t;
  return t > cap;
}
// ... of a _host write entry's one stream: totals as k_row_totals leaves them, AVDB_ERANGE
// under the entry's name when the capacity is too small
inline int host_row_offsets(const char* fn, const uint32_t* out_len, size_t n_rows, uint64_t cap, uint64_t* row_off,
                            uint64_t* totals) {
  totals[1] = host_offsets(out_len, n_rows, cap, row_off, &totals[0]);
  if (!totals[1]) return AVDB_OK;
  avdb_set_error("%s: output of %llu bytes required", fn, (unsigned long long)totals[0]);
  return AVDB_ERANGE;
}

// The write pass of rows rendered one per lane.  A lane storing its own row to global
// memory issues one store per byte or word with 64 different cache lines under it (what
// bounds K5's write pass).  Here a lane renders its row into LDS, at the place the row
// has in the trip's span of the output — the 256 rows of a trip own one contiguous span —
// and the span then goes out as aligned 8-byte words, lane i taking the i-th: a wave's
// store instruction covers 512 contiguous bytes.  Only the span's two edge words, shared
// with the neighbouring trips, are stored bytewise.  A trip whose span does not fit the
// caller's kStageBytes of LDS (s_out) is rendered to global memory bytewise.
// load(r) gives row r's columns, read once, before the trip's staged-or-not branch;
// render(row, put) renders them through put(k, c): byte k of the row is c, k below the
// row's out_len (row_off[r + 1] - row_off[r]).  begin_trip(r0, nr) runs in every thread of the
// workgroup before rows [r0, r0 + nr) are loaded (K19 stages their lines' text there); what it
// leaves in LDS may be read until the trip's rows are rendered.
template <uint32_t kStageBytes, class BeginTrip, class Load, class Render>
__device__ __forceinline__ void write_rows(const uint64_t* __restrict__ row_off, size_t n_rows,
                                           uint8_t* __restrict__ out, const uint64_t* __restrict__ totals,
                                           uint64_t* s_out, BeginTrip begin_trip, Load load, Render render) {
  if (totals[1]) return;  // the capacity is too small: nothing is written
  uint8_t* s_bytes = reinterpret_cast<uint8_t*>(s_out);
  for (size_t r0 = size_t(blockIdx.x) * kBlock; r0 < n_rows; r0 += size_t(gridDim.x) * kBlock) {
    const uint32_t nr = n_rows - r0 < kBlock ? uint32_t(n_rows - r0) : uint32_t(kBlock);
    begin_trip(r0, nr);
    const uint64_t b = row_off[r0], e = row_off[r0 + nr], b8 = b & ~7ull;
    const bool staged = e >= b && e - b8 <= kStageBytes;  // (workgroup-uniform)
    const uint32_t t = threadIdx.x;
    if (t < nr) {
      const size_t r = r0 + t;
      const uint64_t off = row_off[r];
      const auto row = load(r);
      // (off + k < off + out_len = row_off[r + 1] <= e: inside the span, and the stage)
      if (staged) {
        const uint32_t at = uint32_t(off - b8);
        render(row, [&](uint32_t k, uint32_t c) { s_bytes[at + k] = uint8_t(c); });
      } else {
        render(row, [&](uint32_t k, uint32_t c) { out[off + k] = uint8_t(c); });
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

template <uint32_t kStageBytes, class Load, class Render>
__device__ __forceinline__ void write_rows(const uint64_t* __restrict__ row_off, size_t n_rows,
                                           uint8_t* __restrict__ out, const uint64_t* __restrict__ totals,
                                           uint64_t* s_out, Load load, Render render) {
  write_rows<kStageBytes>(row_off, n_rows, out, totals, s_out, [](size_t, uint32_t) {}, load, render);
}

}  // namespace rows
}  // namespace avdb
