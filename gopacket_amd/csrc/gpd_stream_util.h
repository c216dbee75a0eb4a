// gpd_stream_util.h — device helpers the stream builders share (gpd_tcpstream.hip,
// gpd_ip4reasm.hip, gpd_tcpasm.hip): the two-level scan over an array of per-item values (block
// sums, gpd_compact.h's compact_scan over them, the prefix per item) and the byte shuffles of the
// 16-byte gather (gpd_gather.h).  The two writers (gpd_write_scan.h) take the byte shuffles and
// the 64-bit wave helpers from here too.  No kernel here waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpd_compact.h"

namespace gpd {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// ---- the two-level scan: block sums, compact_scan over them, the prefix per item -----------------
// Called by the 256 lanes of workgroup blockIdx.x.  total64 (may be NULL) gets the exact sum.
template <class F>
__device__ __forceinline__ void scan_sum(uint32_t n, uint32_t *blk, uint64_t *total64, F val) {
  __shared__ uint64_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * kCompactBlock;
  uint64_t c = 0;
  for (uint32_t r = 0; r < kCompactBlock / 256u; ++r) {
    const uint32_t i = base + r * 256u + threadIdx.x;
    if (i < n) c += val(i);
  }
#pragma unroll
  for (uint32_t d = 32; d >= 1u; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)c, d, 64), hi = __shfl_xor((uint32_t)(c >> 32), d, 64);
    c += ((uint64_t)hi << 32) | lo;
  }
  if (lane == 0) wsum[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    blk[blockIdx.x] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    if (total64) atomicAdd(reinterpret_cast<unsigned long long *>(total64), (unsigned long long)s);
  }
}

// out[i] = the sum of val over the items before i; with_total: out[n] = the sum of all.  out may
// be the array val reads (a lane reads its item before it writes it).
template <class F>
__device__ __forceinline__ void scan_apply(uint32_t n, const uint32_t *blk, uint32_t *out, bool with_total, F val) {
  __shared__ uint32_t ws[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * kCompactBlock;
  uint32_t carry = blk[blockIdx.x];
  for (uint32_t r = 0; r < kCompactBlock / 256u; ++r) {
    const uint32_t i = base + r * 256u + threadIdx.x;
    const uint32_t v = i < n ? val(i) : 0u;
    const uint32_t x = wave_scan32(v, lane);
    if (lane == 63u) ws[w] = x;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t j = 0; j < w; ++j) before += ws[j];
    if (i < n) out[i] = before + x - v;
    if (with_total && i + 1u == n) out[n] = before + x;
    carry += ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t first_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl_up64(uint64_t v, uint32_t d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
// inclusive scan across the wave
__device__ inline uint64_t wave_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint64_t y = shfl_up64(v, d);
    if (lane >= d) v += y;
  }
  return v;
}
__device__ inline uint32_t wave_min32(uint32_t v) {
#pragma unroll
  for (uint32_t d = 32; d >= 1u; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
  return v;
}

// ---- the gather, 16 bytes at a time -------------------------------------------------------------
// bytes [s, s + 16) of the 32 bytes lo:hi, s in 0..15
__device__ inline v4u bytes_from(v4u lo, v4u hi, uint32_t s) {
  uint32_t x0 = lo.x, x1 = lo.y, x2 = lo.z, x3 = lo.w, x4 = hi.x, x5 = hi.y, x6 = hi.z, x7 = hi.w;
  if (s & 8u) {
    x0 = x2, x1 = x3, x2 = x4, x3 = x5, x4 = x6, x5 = x7;
  }
  if (s & 4u) {
    x0 = x1, x1 = x2, x2 = x3, x3 = x4, x4 = x5;
  }
  const uint32_t b = (s & 3u) * 8u;
  return v4u{__funnelshift_r(x0, x1, b), __funnelshift_r(x1, x2, b), __funnelshift_r(x2, x3, b),
             __funnelshift_r(x3, x4, b)};
}
__device__ inline uint32_t low_bytes(int32_t k) {  // 0xFF in the k lowest bytes (k clamped to 0..4)
  return k <= 0 ? 0u : k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u;
}
// 0xFF in bytes [k0, k1) of 16
__device__ inline v4u byte_mask(int32_t k0, int32_t k1) {
  return v4u{low_bytes(k1) & ~low_bytes(k0), low_bytes(k1 - 4) & ~low_bytes(k0 - 4),
             low_bytes(k1 - 8) & ~low_bytes(k0 - 8), low_bytes(k1 - 12) & ~low_bytes(k0 - 12)};
}
// data[a, a + 16) for a signed byte position, from two aligned 16-byte loads shifted together;
// bytes no load may fetch (outside [0, lim), lim the buffer's length rounded up to 16) read as
// zero (the callers mask them away)
__device__ inline v4u src16_of(const uint8_t *data, uint64_t lim, int64_t a) {
  const int64_t a0 = a & ~(int64_t)15;
  const uint32_t s = (uint32_t)(a & 15);
  const v4u z{0u, 0u, 0u, 0u};
  const v4u lo = (a0 >= 0 && (uint64_t)a0 < lim) ? *reinterpret_cast<const v4u *>(data + a0) : z;
  const v4u hi = (s != 0u && a0 + 16 >= 0 && (uint64_t)(a0 + 16) < lim) ? *reinterpret_cast<const v4u *>(data + a0 + 16) : z;
  return bytes_from(lo, hi, s);
}

}  // namespace gpd
