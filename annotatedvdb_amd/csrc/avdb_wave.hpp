// Wave and workgroup sums, scans and appends (device code; included from
// avdb_internal.hpp).  Every function here must be called by all 64 lanes of the
// wave, and block_excl by all NT threads of the workgroup, from wave- (workgroup-)
// uniform control flow: the shuffles and the DPP scan read neighbouring lanes'
// registers whether or not those lanes are active, and block_excl has barriers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace avdb {

constexpr int kWave = 64;  // gfx950 runs wave64

// 64-bit lane reads from two 32-bit ones
static __device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int d) {
  return (uint64_t(uint32_t(__shfl_xor(uint32_t(v >> 32), d, kWave))) << 32) | uint32_t(__shfl_xor(uint32_t(v), d, kWave));
}
// v of the lane d below (the lane's own v in lanes < d)
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  return (uint64_t(uint32_t(__shfl_up(uint32_t(v >> 32), d, kWave))) << 32) | uint32_t(__shfl_up(uint32_t(v), d, kWave));
}

// v summed over the wave, in every lane (xor butterfly)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += shfl_xor64(v, d);
  return v;
}

// inclusive wave64 prefix sum through DPP row shifts and row broadcasts: six
// VALU adds with no LDS round trip (__shfl_up lowers to ds_bpermute: six
// dependent LDS trips per value)
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x) {
  x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xF, 0xF, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1, 3
  x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2, 3
  return x;
}
// the 64-bit one is the shuffle ladder (a DPP form would need a carry pass)
__device__ __forceinline__ uint64_t wave_incl_sum(uint64_t x) {
  const uint32_t lane = __lane_id();
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint64_t u = shfl_up64(x, d);
    if (lane >= uint32_t(d)) x += u;
  }
  return x;
}

// *dst += v summed over the wave: one atomic per wave (LDS or global), none for 0
__device__ __forceinline__ void wave_add(unsigned long long* dst, uint32_t v) {
  v = wave_sum(v);
  if (__lane_id() == 0 && v) atomicAdd(dst, (unsigned long long)v);
}
__device__ __forceinline__ void wave_add(unsigned long long* dst, uint64_t v) {
  v = wave_sum(v);
  if (__lane_id() == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

// Wave-aggregated append to a list whose length is *counter (LDS): the wave claims
// its lanes' cnt slots with one atomic (none when it has nothing to append);
// returns this lane's first slot.
__device__ __forceinline__ uint32_t wave_append(uint32_t cnt, uint32_t* counter) {
  const uint32_t incl = wave_incl_sum(cnt);
  const uint32_t total = __shfl(incl, kWave - 1, kWave);
  if (!total) return 0;
  uint32_t base = 0;
  if (__lane_id() == kWave - 1) base = atomicAdd(counter, total);
  return __shfl(base, kWave - 1, kWave) + incl - cnt;
}

// Exclusive scan over the NT threads of the workgroup of N values per thread, in
// place in v; total[a] = the sum of value a.  One barrier pair: s_w (N rows of one
// word per wave) may be reused as soon as the call returns.
template <int NT, class T, int N = 1>
__device__ __forceinline__ void block_excl(T (&v)[N], T (*s_w)[NT / kWave], T (&total)[N]) {
  static_assert(NT % kWave == 0, "whole waves");
  const uint32_t lane = __lane_id(), wv = threadIdx.x / kWave;
  T x[N];
#pragma unroll
  for (int a = 0; a < N; ++a) {
    x[a] = wave_incl_sum(v[a]);
    if (lane == kWave - 1) s_w[a][wv] = x[a];
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < N; ++a) {
    T base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < NT / kWave; ++w) {
      const T t = s_w[a][w];
      if (w < wv) base += t;
      tot += t;
    }
    total[a] = tot;
    v[a] = base + x[a] - v[a];
  }
  __syncthreads();
}
// one value per thread: returns its exclusive prefix; s_w holds NT / kWave words
template <int NT, class T>
__device__ __forceinline__ T block_excl(T v, T* s_w, T* total) {
  T a[1] = {v}, t[1];
  block_excl<NT, T, 1>(a, reinterpret_cast<T(*)[NT / kWave]>(s_w), t);
  *total = t[0];
  return a[0];
}

}  // namespace avdb
