// K15 — a whole-genome VCF split into per-chromosome texts (gfx950).
//
// Replaces the per-line Python of Util/bin/split_vcf_by_chr.py (run: a gzip read, a decode,
// an rstrip, a split, a dict lookup and a print per line on one host thread) with a stable
// 26-way partition of the slab's lines on the device:
//   size pass (avdb_vcf_split_size; rows::begin_size, the prologue shared with K12, K13 and K14:
//   avdb_rows.hpp)
//     (K0's count and line-starts passes write the caller's line_start)
//     k_split_lines    one lane per line, 256 lines' text staged in LDS: the stored length
//                      (rstrip), the comment test, the key's stream (exact label, or the
//                      chromosome map); the counts through an LDS tally per workgroup
//   write pass (avdb_vcf_split_write)
//     k_split_tiles    one workgroup per 256-line tile: the tile's bytes per stream into the
//                      stream-major matrix tile_bytes[c * n_tiles + t]
//     (one exclusive scan of that matrix: every tile's base in every stream; the stream
//      starts are its column heads)
//     k_split_offsets  stream_off and the total against the caller's capacity
//     k_split_copy     one workgroup per tile, its text staged in LDS: a line's offset among
//                      the tile's lines of its stream (one wave sum when the wave's lines
//                      share a stream, else one masked sum per stream present; the four
//                      waves' totals in LDS), then each wave copies its lines one at a time,
//                      64 consecutive bytes per store
// The per-line code is avdb_splitvcf.hpp, shared with the _host entries.
#include "avdb_splitvcf.hpp"
#include "avdb_rows.hpp"

#include <string.h>

namespace avdb {

using splitvcf::kStreams;
using splitvcf::Line;

constexpr uint32_t kSplitNone = kStreams;  // a lane's stream when its line has no output

// v of lane `src`, in every lane
__device__ __forceinline__ uint64_t lane_value64(uint64_t v, int src) {
  return (uint64_t(uint32_t(__shfl(uint32_t(v >> 32), src, kWave))) << 32) | uint32_t(__shfl(uint32_t(v), src, kWave));
}

// v of lane j (wave-uniform j), without an LDS round trip
__device__ __forceinline__ uint32_t read_lane(uint32_t v, int j) { return uint32_t(__builtin_amdgcn_readlane(int(v), j)); }
__device__ __forceinline__ uint64_t read_lane64(uint64_t v, int j) {
  return (uint64_t(read_lane(uint32_t(v >> 32), j)) << 32) | read_lane(uint32_t(v), j);
}

// Whether the wave's lanes with a stream (st < kStreams) all have the same one, *c0; mask:
// those lanes (0: none, and nothing to do).  Called by all lanes.
__device__ __forceinline__ bool wave_one_stream(uint32_t st, uint64_t* mask, uint32_t* c0) {
  const bool active = st < kStreams;
  *mask = __ballot(active);
  if (!*mask) return true;
  *c0 = uint32_t(__shfl(int(st), __builtin_ctzll(*mask), kWave));
  return __ballot(active && st != *c0) == 0;
}

__global__ __launch_bounds__(kBlock) void k_split_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                        const uint64_t* __restrict__ starts, size_t n_lines,
                                                        ChromMapView cm, uint8_t* __restrict__ code,
                                                        uint32_t* __restrict__ out_len,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kStage / 16];
  __shared__ unsigned long long s_cnt[AVDB_SPLIT_N_COUNTS];
  for (uint32_t i = threadIdx.x; i < AVDB_SPLIT_N_COUNTS; i += kBlock)
    s_cnt[i] = i == AVDB_SPLIT_COUNT_FIRST_OTHER ? ~0ull : 0ull;
  __syncthreads();
  const Heap h = make_heap(text, text_bytes);
  for (size_t base = size_t(blockIdx.x) * kBlock; base < n_lines; base += size_t(gridDim.x) * kBlock) {
    const size_t last = base + kBlock < n_lines ? base + kBlock : n_lines;
    uint64_t s0, s1;
    lines::trip_span(starts, base, last, n_lines, text_bytes, &s0, &s1);
    const Window w = stage_window<kBlock, kStage>(h, s0, s1, s_text);
    const size_t li = base + threadIdx.x;
    // a lane's stream in the tally: 0..25, kStreams for a comment, kStreams + 1 for no line
    uint32_t st = kStreams + 1, bytes = 0, host = 0;
    if (li < n_lines) {
      uint64_t s, e;
      lines::line_span(text, text_bytes, starts, n_lines, li, &s, &e);
      const Line L = w.staged && s >= s0 && e <= s1
                         ? splitvcf::scan_line((lds_cp)(reinterpret_cast<const uint8_t*>(s_text) + (h.lo + s - w.a0)),
                                               e - s, cm)
                         : splitvcf::scan_line((glb_cp)(text + s), e - s, cm);
      code[li] = uint8_t(L.code);
      out_len[li] = L.out_len;
      st = L.code < kStreams ? L.code : kStreams;
      bytes = L.out_len & ~AVDB_SPLIT_LINE_HOST;
      host = (L.out_len & AVDB_SPLIT_LINE_HOST) != 0;
      if (L.code == AVDB_SPLIT_OTHER) atomicMin(&s_cnt[AVDB_SPLIT_COUNT_FIRST_OTHER], (unsigned long long)li);
    }
    // the tally (all lanes here): a wave of one stream, what a sorted VCF gives, adds once
    const uint32_t first = uint32_t(__shfl(int(st), 0, kWave));
    if (__ballot(st != first) == 0) {
      const uint64_t tot = wave_sum(uint64_t(bytes));
      if (__lane_id() == 0 && first <= kStreams) {
        if (first < kStreams) {
          atomicAdd(&s_cnt[AVDB_SPLIT_COUNT_LINES + first], (unsigned long long)kWave);
          atomicAdd(&s_cnt[AVDB_SPLIT_COUNT_BYTES + first], (unsigned long long)tot);
        } else {
          atomicAdd(&s_cnt[AVDB_SPLIT_COUNT_COMMENTS], (unsigned long long)kWave);
        }
      }
    } else if (st < kStreams) {
      atomicAdd(&s_cnt[AVDB_SPLIT_COUNT_LINES + st], 1ull);
      atomicAdd(&s_cnt[AVDB_SPLIT_COUNT_BYTES + st], (unsigned long long)bytes);
    } else if (st == kStreams) {
      atomicAdd(&s_cnt[AVDB_SPLIT_COUNT_COMMENTS], 1ull);
    }
    wave_add(&s_cnt[AVDB_SPLIT_COUNT_HOST_LINES], host);
    __syncthreads();  // the stage is reused by the next trip
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < AVDB_SPLIT_N_COUNTS; i += kBlock) {
    const unsigned long long v = s_cnt[i];
    if (i == AVDB_SPLIT_COUNT_FIRST_OTHER) {
      if (v != ~0ull) atomicMin(&counts[i], v);
    } else if (v) {
      atomicAdd(&counts[i], v);
    }
  }
}

// a lane's line in the write pass: its stream (kSplitNone: no output) and its bytes
__device__ __forceinline__ void load_line(const uint8_t* __restrict__ code, const uint32_t* __restrict__ out_len,
                                          size_t li, size_t n_lines, uint32_t* st, uint32_t* len) {
  *st = kSplitNone;
  *len = 0;
  if (li < n_lines) {
    const uint32_t ol = out_len[li] & ~AVDB_SPLIT_LINE_HOST;
    *st = splitvcf::stream_of(code[li], ol);
    *len = *st < kStreams ? ol : 0u;
  }
}

// tile_bytes[c * n_tiles + t] = the bytes of tile t's lines of stream c; tile_bytes[26 * n_tiles] = 0
__global__ __launch_bounds__(kBlock) void k_split_tiles(const uint8_t* __restrict__ code,
                                                        const uint32_t* __restrict__ out_len, size_t n_lines,
                                                        size_t n_tiles, uint64_t* __restrict__ tile_bytes) {
  __shared__ unsigned long long s_sum[kStreams];
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[kStreams * n_tiles] = 0;
  for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (threadIdx.x < kStreams) s_sum[threadIdx.x] = 0;
    __syncthreads();
    uint32_t st, len;
    load_line(code, out_len, t * kBlock + threadIdx.x, n_lines, &st, &len);
    uint64_t mask;
    uint32_t c0 = 0;
    if (wave_one_stream(st, &mask, &c0)) {
      if (mask) {
        const uint64_t tot = wave_sum(uint64_t(len));
        if (__lane_id() == 0) atomicAdd(&s_sum[c0], (unsigned long long)tot);
      }
    } else if (st < kStreams) {
      atomicAdd(&s_sum[st], (unsigned long long)len);
    }
    __syncthreads();
    if (threadIdx.x < kStreams) tile_bytes[size_t(threadIdx.x) * n_tiles + t] = s_sum[threadIdx.x];
    __syncthreads();  // s_sum is reused by the next trip
  }
}

// stream_off[c] = the scanned matrix's column heads, stream_off[26] = totals[0] = the bytes of
// all streams; totals[1]: 1 when they exceed cap (the copy kernel then writes nothing)
__global__ void k_split_offsets(const uint64_t* __restrict__ tile_off, size_t n_tiles, uint64_t cap,
                                uint64_t* __restrict__ stream_off, uint64_t* __restrict__ totals) {
  const uint32_t c = threadIdx.x;
  if (blockIdx.x || c > kStreams) return;
  const uint64_t v = n_tiles ? tile_off[size_t(c) * n_tiles] : 0ull;
  stream_off[c] = v;
  if (c == kStreams) {
    totals[0] = v;
    totals[1] = v > cap;
  }
}

__global__ __launch_bounds__(kBlock) void k_split_copy(const uint8_t* __restrict__ text, size_t text_bytes,
                                                       size_t n_lines, const uint8_t* __restrict__ code,
                                                       const uint64_t* __restrict__ line_start,
                                                       const uint32_t* __restrict__ out_len, size_t n_tiles,
                                                       const uint64_t* __restrict__ tile_off,
                                                       uint8_t* __restrict__ out, uint64_t out_cap,
                                                       uint64_t* __restrict__ dst_off,
                                                       const uint64_t* __restrict__ totals) {
  __shared__ u32x4 s_text[kStage / 16];
  __shared__ uint64_t s_wave[kBlock / kWave][kStreams];  // a wave's bytes per stream in this tile
  if (totals[1]) return;  // the capacity is too small: nothing is written
  const lds_cp s_bytes = (lds_cp)(reinterpret_cast<const uint8_t*>(s_text));
  const Heap h = make_heap(text, text_bytes);
  const uint32_t lane = __lane_id(), wv = threadIdx.x / kWave;
  for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const size_t base = t * kBlock, last = base + kBlock < n_lines ? base + kBlock : n_lines;
    for (uint32_t i = threadIdx.x; i < (kBlock / kWave) * kStreams; i += kBlock) (&s_wave[0][0])[i] = 0;
    uint64_t s0, s1;
    lines::trip_span(line_start, base, last, n_lines, text_bytes, &s0, &s1);
    const Window w = stage_window<kBlock, kStage>(h, s0, s1, s_text);  // (ends in a barrier: s_wave is zero)
    const size_t li = base + threadIdx.x;
    uint32_t st, len;
    load_line(code, out_len, li, n_lines, &st, &len);
    uint64_t s = 0;
    if (st < kStreams) {
      s = line_start[li];
      if (s > text_bytes) s = text_bytes;
    }
    // the line's offset among its wave's lines of the same stream
    uint64_t mask, excl = 0;
    uint32_t c0 = 0;
    if (wave_one_stream(st, &mask, &c0)) {
      if (mask) {
        const uint64_t incl = wave_incl_sum(uint64_t(len));
        excl = incl - len;
        const uint64_t tot = lane_value64(incl, kWave - 1);
        if (lane == 0) s_wave[wv][c0] = tot;
      }
    } else {
      for (uint64_t rem = mask; rem;) {  // one masked sum per stream present
        const uint32_t c = uint32_t(__shfl(int(st), __builtin_ctzll(rem), kWave));
        const bool mine = st == c;
        const uint64_t incl = wave_incl_sum(mine ? uint64_t(len) : uint64_t(0));
        if (mine) excl = incl - len;
        const uint64_t tot = lane_value64(incl, kWave - 1);
        if (lane == 0) s_wave[wv][c] = tot;
        rem &= ~__ballot(mine);
      }
    }
    __syncthreads();
    uint64_t dst = ~0ull;
    if (st < kStreams) {
      dst = tile_off[size_t(st) * n_tiles + t] + excl;
      for (uint32_t v = 0; v < wv; ++v) dst += s_wave[v][st];
    }
    if (dst_off && li < n_lines) dst_off[li] = dst;
    // the copy: the wave's lines one at a time, lane k the line's bytes k, k + 64, ...; the
    // stored bytes come from the stage (or from global memory where the line is not in
    // it), the last one is the '\n'
    const uint32_t pay = len ? len - 1 : 0u;
    const bool in_lds = w.staged && s >= s0 && s + pay <= s1;
    const uint32_t lds_at = in_lds ? uint32_t(h.lo + s - w.a0) : 0u;
    const uint64_t lds_mask = __ballot(in_lds);
    for (uint64_t m = mask; m; m &= m - 1) {
      const int j = __builtin_ctzll(m);  // (wave-uniform: the line's values are read from its lane's registers)
      const uint32_t len_j = read_lane(len, j), pay_j = len_j - 1;
      const uint64_t dst_j = read_lane64(dst, j);
      if (dst_j > out_cap || len_j > out_cap - dst_j) continue;  // (never, with the arrays the tile pass read)
      if ((lds_mask >> j) & 1) {
        const uint32_t at_j = read_lane(lds_at, j);
        for (uint32_t k = lane; k < len_j; k += kWave) out[dst_j + k] = k < pay_j ? s_bytes[at_j + k] : uint8_t('\n');
      } else {
        const uint64_t s_j = read_lane64(s, j);
        for (uint32_t k = lane; k < len_j; k += kWave) {
          const uint64_t p = s_j + k;
          out[dst_j + k] = k < pay_j ? (p < text_bytes ? text[p] : uint8_t(0)) : uint8_t('\n');
        }
      }
    }
    __syncthreads();  // the stage and s_wave are reused by the next trip
  }
}

}  // namespace avdb

using namespace avdb;

// workspace: count workspace | tile matrix (26 * n_tiles + 1) | scan temp
struct SplitLayout {
  size_t n_tiles, n_mat, mat, scan, scan_bytes, total;
};
static SplitLayout split_layout(size_t n_lines) {
  SplitLayout L;
  L.n_tiles = (n_lines + kBlock - 1) / kBlock;
  L.n_mat = size_t(kStreams) * L.n_tiles + 1;
  L.mat = AVDB_VCF_COUNT_WORKSPACE_BYTES;
  L.scan = L.mat + lines::pad256(8 * L.n_mat);
  L.scan_bytes = lines::pad256(scan::workspace_bytes(L.n_mat));
  L.total = L.scan + L.scan_bytes;
  return L;
}

extern "C" int avdb_vcf_split_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(split_layout(n_lines).total, bytes);
}

static const char* size_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const uint8_t* code, const uint64_t* line_start, const uint32_t* out_len,
                                   const uint64_t* counts) {
  if (!ctx) return "null context";
  if (!counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!code || !line_start || !out_len)) return "null output array";
  return nullptr;
}

static const char* write_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const uint8_t* code, const uint64_t* line_start, const uint32_t* out_len,
                                    const uint8_t* out, size_t out_cap, const uint64_t* stream_off,
                                    const uint64_t* totals) {
  if (!ctx) return "null context";
  if (!totals || !stream_off) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!code || !line_start || !out_len)) return "null line array";
  if (out_cap && !out) return "null output";
  return nullptr;
}

extern "C" int avdb_vcf_split_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const avdb_chrom_map* chrom_map, uint8_t* code, uint64_t* line_start,
                                   uint32_t* out_len, uint64_t* counts, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, code, line_start, out_len, counts)) {
    avdb_set_error("avdb_vcf_split_size: %s", err);
    return AVDB_EINVAL;
  }
  if (chrom_map && chrom_map->device != ctx->device) {
    avdb_set_error("avdb_vcf_split_size: chromosome map made for device %d", chrom_map->device);
    return AVDB_EINVAL;
  }
  const SplitLayout L = split_layout(n_lines);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_vcf_split_size", ctx, L.total, n_lines, workspace, workspace_bytes, counts,
                               AVDB_SPLIT_COUNT_FIRST_OTHER, s))
    return e;
  AVDB_HIP_TRY(hipMemsetAsync(counts + AVDB_SPLIT_COUNT_FIRST_OTHER, 0xFF, 8, s));
  if (n_lines == 0) return AVDB_OK;
  AVDB_HIP_TRY(hipMemsetAsync(line_start, 0xFF, 8 * n_lines, s));
  if (int e = text_line_starts(text, text_bytes, n_lines, workspace, line_start, s)) return e;
  const ChromMapView cm = chrom_map ? chrom_map->dev : ChromMapView{};
  hipLaunchKernelGGL(k_split_lines, dim3(stream_grid(n_lines, kBlock, 4096)), dim3(kBlock), 0, s, text, text_bytes,
                     line_start, n_lines, cm, code, out_len, reinterpret_cast<unsigned long long*>(counts));
  AVDB_LAUNCH_CHECK("k_split_lines");
  return AVDB_OK;
}

extern "C" int avdb_vcf_split_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const uint8_t* code, const uint64_t* line_start, const uint32_t* out_len,
                                    uint8_t* out, size_t out_cap, uint64_t* stream_off, uint64_t* dst_off,
                                    uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, code, line_start, out_len, out, out_cap,
                                         stream_off, totals)) {
    avdb_set_error("avdb_vcf_split_write: %s", err);
    return AVDB_EINVAL;
  }
  const SplitLayout L = split_layout(n_lines);
  if (int e = n_lines ? lines::workspace_error("avdb_vcf_split_write", L.total, workspace, workspace_bytes) : 0) return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  uint64_t* mat = n_lines ? reinterpret_cast<uint64_t*>(w + L.mat) : nullptr;
  const unsigned grid = stream_grid(L.n_tiles, 1, 4096);
  if (n_lines) {
    hipLaunchKernelGGL(k_split_tiles, dim3(grid), dim3(kBlock), 0, s, code, out_len, n_lines, L.n_tiles, mat);
    AVDB_LAUNCH_CHECK("k_split_tiles");
    if (int e = scan::exclusive_u64(mat, mat, L.n_mat, w + L.scan, L.scan_bytes, s)) return e;
  }
  hipLaunchKernelGGL(k_split_offsets, dim3(1), dim3(kWave), 0, s, mat, L.n_tiles, uint64_t(out_cap), stream_off, totals);
  AVDB_LAUNCH_CHECK("k_split_offsets");
  if (n_lines == 0) return AVDB_OK;
  hipLaunchKernelGGL(k_split_copy, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, n_lines, code, line_start, out_len,
                     L.n_tiles, mat, out, uint64_t(out_cap), dst_off, totals);
  AVDB_LAUNCH_CHECK("k_split_copy");
  return AVDB_OK;
}

// ---- the same code on the host ------------------------------------------------
extern "C" int avdb_vcf_split_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        const avdb_chrom_map* chrom_map, uint8_t* code, uint64_t* line_start,
                                        uint32_t* out_len, uint64_t* counts) {
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, code, line_start, out_len, counts)) {
    avdb_set_error("avdb_vcf_split_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_SPLIT_N_COUNTS);
  counts[AVDB_SPLIT_COUNT_FIRST_OTHER] = ~0ull;
  if (n_lines == 0) return AVDB_OK;
  const ChromMapView cm = chrom_map ? chrom_map->host_view() : ChromMapView{};
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e);
    const Line L = splitvcf::scan_line(text + s, e - s, cm);
    code[li] = uint8_t(L.code);
    line_start[li] = starts[li];
    out_len[li] = L.out_len;
    counts[AVDB_SPLIT_COUNT_HOST_LINES] += (L.out_len & AVDB_SPLIT_LINE_HOST) != 0;
    if (L.code >= kStreams) {
      ++counts[AVDB_SPLIT_COUNT_COMMENTS];
      continue;
    }
    ++counts[AVDB_SPLIT_COUNT_LINES + L.code];
    counts[AVDB_SPLIT_COUNT_BYTES + L.code] += L.out_len & ~AVDB_SPLIT_LINE_HOST;
    if (L.code == AVDB_SPLIT_OTHER && counts[AVDB_SPLIT_COUNT_FIRST_OTHER] == ~0ull)
      counts[AVDB_SPLIT_COUNT_FIRST_OTHER] = li;
  }
  return AVDB_OK;
}

extern "C" int avdb_vcf_split_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         const uint8_t* code, const uint64_t* line_start, const uint32_t* out_len,
                                         uint8_t* out, size_t out_cap, uint64_t* stream_off, uint64_t* dst_off,
                                         uint64_t* totals) {
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, code, line_start, out_len, out, out_cap,
                                         stream_off, totals)) {
    avdb_set_error("avdb_vcf_split_write_host: %s", err);
    return AVDB_EINVAL;
  }
  uint64_t bytes[kStreams + 1] = {0};
  for (size_t li = 0; li < n_lines; ++li) {
    const uint32_t ol = out_len[li] & ~AVDB_SPLIT_LINE_HOST;
    bytes[splitvcf::stream_of(code[li], ol)] += ol;
  }
  uint64_t t = 0, next[kStreams];
  for (uint32_t c = 0; c < kStreams; ++c) {
    stream_off[c] = next[c] = t;
    t += bytes[c];
  }
  stream_off[kStreams] = t;
  totals[0] = t;
  totals[1] = t > out_cap;
  if (totals[1]) {
    avdb_set_error("avdb_vcf_split_write_host: output of %llu bytes required", (unsigned long long)t);
    return AVDB_ERANGE;
  }
  for (size_t li = 0; li < n_lines; ++li) {
    const uint32_t ol = out_len[li] & ~AVDB_SPLIT_LINE_HOST, st = splitvcf::stream_of(code[li], ol);
    if (st >= kStreams) {
      if (dst_off) dst_off[li] = ~0ull;
      continue;
    }
    const uint64_t d = next[st], s = line_start[li] < text_bytes ? line_start[li] : text_bytes;
    next[st] += ol;
    if (dst_off) dst_off[li] = d;
    for (uint32_t k = 0; k + 1 < ol; ++k) out[d + k] = s + k < text_bytes ? text[s + k] : uint8_t(0);
    out[d + ol - 1] = uint8_t('\n');
  }
  return AVDB_OK;
}
