// K11 — BGZF (bgzip) input inflated on the GPU (gfx950).
//
// Replaces the one-host-thread gzip read in front of K0 and K10a: a BGZF file is a chain
// of independent gzip members of at most 64 KiB of output each, every one stating its
// compressed size (BSIZE) and its output size (ISIZE):
//   avdb_bgzf_index_host   one pointer-chase over the headers: member offsets and the
//                          exclusive sum of ISIZE (host)
//   k_bgzf_inflate         one 64-lane wave per member, a resident grid striding over
//                          the members: Huffman tables built by the wave in LDS, one
//                          uniform symbol chain, matches copied by all lanes into the
//                          wave's 64 KiB window, CRC-32 in 64 chunks combined by powers
//                          of x, the window flushed with 16-byte stores once the CRC matched
// The per-member code is avdb_inflate.hpp, shared with avdb_bgzf_inflate_host.
//
// The symbol chain is latency-bound (each lookup waits for the one before it), so
// throughput is members in flight, not speed per member.  The window is therefore a slot
// of a workspace in global memory (owned by the context, one slot per wave of the grid),
// read back through L2, and only the tables (5 KiB) are in LDS: 128 VGPRs admit 16 waves
// per CU.  With the window in LDS (71 KiB with the tables: two waves per CU) the same
// code inflated 335 MB of VCF text in 51.0 ms, against 17.3 ms with the window in global
// memory and 8 waves per CU, 13.5 ms with 12 and 12.4 ms with 16 (1.34 GB: 60.0, 46.7 and
// 38.5 ms); profiles/k11_ab/window_lds_vs_global.txt, profiles/k11_ab/grid_sweep.txt.
#include "avdb_inflate.hpp"

#include <string.h>

#include <memory>

namespace avdb {

constexpr int kK11WavesPerCu = 16;  // what 128 VGPRs admit (4 per SIMD); the window workspace is then 256 MiB

__global__ __launch_bounds__(kWave, 4) void k_bgzf_inflate(const uint8_t* __restrict__ comp, size_t comp_bytes,
                                                         const uint64_t* __restrict__ in_off,
                                                         const uint64_t* __restrict__ out_off, size_t n_blocks,
                                                         uint8_t* __restrict__ out, size_t out_cap,
                                                         uint8_t* __restrict__ status,
                                                         unsigned long long* __restrict__ counts,
                                                         inflate::Window* __restrict__ windows) {
  __shared__ inflate::State S;
  inflate::Window& W = windows[blockIdx.x];  // (gridDim.x slots)
  const inflate::Lanes L{threadIdx.x, uint32_t(kWave)};
  unsigned long long n_ok = 0, n_bad = 0, first_bad = ~0ull;
  for (size_t k = blockIdx.x; k < n_blocks; k += gridDim.x) {
    const uint32_t st = inflate::inflate_member(L, S, W.b, comp, comp_bytes, in_off[k], out_off[k], out_off[k + 1], out, out_cap);
    if (threadIdx.x == 0) status[k] = uint8_t(st);
    if (st == AVDB_BGZF_OK) {
      ++n_ok;
    } else {
      ++n_bad;
      if (k < first_bad) first_bad = k;
    }
    __syncthreads();  // the window and the tables are reused by the next trip
  }
  if (threadIdx.x == 0) {
    if (n_ok) atomicAdd(&counts[AVDB_BGZF_COUNT_OK], n_ok);
    if (n_bad) {
      atomicAdd(&counts[AVDB_BGZF_COUNT_FAILED], n_bad);
      atomicMin(&counts[AVDB_BGZF_COUNT_FIRST_FAILED], first_bad);
    }
  }
}

}  // namespace avdb

using namespace avdb;

extern "C" int avdb_bgzf_index_host(const uint8_t* data, size_t bytes, size_t blocks_cap, uint64_t* in_off,
                                    uint64_t* out_off, size_t* n_blocks, size_t* consumed, uint64_t* out_bytes) {
  if (!n_blocks || !consumed || !out_bytes || (bytes && !data) || (blocks_cap && (!in_off || !out_off))) {
    avdb_set_error("avdb_bgzf_index_host: null argument");
    return AVDB_EINVAL;
  }
  size_t n = 0, at = 0;
  uint64_t total = 0;
  while (n < blocks_cap && at < bytes) {  // (a member is at least 26 bytes)
    inflate::Member m;
    const int r = inflate::parse_member(data + at, bytes - at, &m);
    if (r == inflate::kMemberIncomplete) break;
    if (r != inflate::kMemberOk) {
      if (n == 0 && r == inflate::kMemberNotBgzf) {
        avdb_set_error("avdb_bgzf_index_host: a gzip stream, but not BGZF");
        return AVDB_ENOTBGZF;
      }
      avdb_set_error("avdb_bgzf_index_host: no BGZF member at offset %zu (%s)", at,
                     r == inflate::kMemberNotGzip ? "no gzip magic" : "no BC subfield, or BSIZE / ISIZE out of range");
      return AVDB_EINVAL;
    }
    in_off[n] = at;
    out_off[n] = total;
    total += m.isize;
    at += m.total_bytes;
    ++n;
  }
  if (blocks_cap) out_off[n] = total;
  *n_blocks = n;
  *consumed = at;
  *out_bytes = total;
  return AVDB_OK;
}

static const char* inflate_args_error(const void* ctx, const uint8_t* comp, const uint64_t* in_off, const uint64_t* out_off,
                                      size_t n_blocks, const uint8_t* out, size_t out_cap, const uint8_t* status,
                                      const uint64_t* counts) {
  if (!ctx || !counts) return "null argument";
  if (n_blocks && (!comp || !in_off || !out_off || !status)) return "null array";
  if (out_cap && !out) return "null output";
  return nullptr;
}

extern "C" int avdb_bgzf_inflate(avdb_ctx* ctx, const uint8_t* comp, size_t comp_bytes, const uint64_t* in_off,
                                 const uint64_t* out_off, size_t n_blocks, uint8_t* out, size_t out_cap,
                                 uint8_t* status, uint64_t* counts, void* stream) {
  if (const char* err = inflate_args_error(ctx, comp, in_off, out_off, n_blocks, out, out_cap, status, counts)) {
    avdb_set_error("avdb_bgzf_inflate: %s", err);
    return AVDB_EINVAL;
  }
  if (ctx->device < 0) {
    avdb_set_error("avdb_bgzf_inflate: a host-only context (use avdb_bgzf_inflate_host)");
    return AVDB_EINVAL;
  }
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  AVDB_HIP_TRY(hipMemsetAsync(counts, 0, 8 * AVDB_BGZF_COUNT_FIRST_FAILED, s));
  AVDB_HIP_TRY(hipMemsetAsync(counts + AVDB_BGZF_COUNT_FIRST_FAILED, 0xFF, 8, s));
  if (n_blocks == 0) return AVDB_OK;
  // a resident grid striding over the chain, and one window per wave of it: the context's, grown when a
  // call needs more (calls on one context are ordered on one stream, so no two launches share a slot)
  size_t grid = ctx->k11_grid > 0 ? size_t(ctx->k11_grid) : size_t(ctx->n_cu) * kK11WavesPerCu;
  if (grid > n_blocks) grid = n_blocks;
  if (grid > ctx->k11_windows_n) {
    if (ctx->k11_windows) AVDB_HIP_TRY(hipFree(ctx->k11_windows));  // (waits for the launches that use it)
    ctx->k11_windows = nullptr;
    ctx->k11_windows_n = 0;
    AVDB_HIP_TRY(hipMalloc(&ctx->k11_windows, grid * sizeof(inflate::Window)));
    ctx->k11_windows_n = grid;
  }
  hipLaunchKernelGGL(k_bgzf_inflate, dim3(unsigned(grid)), dim3(kWave), 0, s, comp, comp_bytes, in_off, out_off,
                     n_blocks, out, out_cap, status, reinterpret_cast<unsigned long long*>(counts),
                     static_cast<inflate::Window*>(ctx->k11_windows));
  AVDB_LAUNCH_CHECK("k_bgzf_inflate");
  return AVDB_OK;
}

extern "C" int avdb_bgzf_inflate_host(const avdb_ctx* ctx, const uint8_t* comp, size_t comp_bytes,
                                      const uint64_t* in_off, const uint64_t* out_off, size_t n_blocks, uint8_t* out,
                                      size_t out_cap, uint8_t* status, uint64_t* counts) {
  if (const char* err = inflate_args_error(ctx, comp, in_off, out_off, n_blocks, out, out_cap, status, counts)) {
    avdb_set_error("avdb_bgzf_inflate_host: %s", err);
    return AVDB_EINVAL;
  }
  counts[AVDB_BGZF_COUNT_OK] = counts[AVDB_BGZF_COUNT_FAILED] = 0;
  counts[AVDB_BGZF_COUNT_FIRST_FAILED] = ~0ull;
  if (n_blocks == 0) return AVDB_OK;
  std::unique_ptr<inflate::State> S(new (std::nothrow) inflate::State());
  std::unique_ptr<inflate::Window> W(new (std::nothrow) inflate::Window());
  if (!S || !W) {
    avdb_set_error("avdb_bgzf_inflate_host: out of memory");
    return AVDB_ENOMEM;
  }
  const inflate::Lanes L{0, 1};
  for (size_t k = 0; k < n_blocks; ++k) {
    const uint32_t st = inflate::inflate_member(L, *S, W->b, comp, comp_bytes, in_off[k], out_off[k], out_off[k + 1], out, out_cap);
    status[k] = uint8_t(st);
    if (st == AVDB_BGZF_OK) {
      ++counts[AVDB_BGZF_COUNT_OK];
    } else {
      ++counts[AVDB_BGZF_COUNT_FAILED];
      if (k < counts[AVDB_BGZF_COUNT_FIRST_FAILED]) counts[AVDB_BGZF_COUNT_FIRST_FAILED] = k;
    }
  }
  return AVDB_OK;
}
