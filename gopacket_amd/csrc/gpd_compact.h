// gpd_compact.h — the ordered compaction the hand-offs share (the IPv4 fragment hand-off in
// gpd_kernels.hip, the tcpassembly hand-off in gpd_tcpseg.hip): which items of a batch are kept,
// and the kept items' indices in order.  Three steps, each a kernel of its user's that calls the
// device function here; none waits on another workgroup.
//
//   compact_count   256 lanes per kCompactBlock items: one kept bit per item into 64-bit mask
//                   words (bit l of word w = item 64w + l) and the block's kept count
//   compact_scan    one workgroup of 1024: exclusive scan of the block counts in place, 1,024 at
//                   a time (coalesced); blk[nblk] = the total
//   compact_index   64 lanes per block, one mask word each: the kept items' indices in order
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpd {

// Items per counting workgroup: 8 rounds of 256 lanes.
constexpr uint32_t kCompactBlock = 2048;

__device__ __forceinline__ uint32_t wave_scan32(uint32_t x, uint32_t lane) {  // inclusive
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// Called by the 256 lanes of workgroup blockIdx.x; keep(i) is evaluated for the items i < n of
// the block only.
template <class F>
__device__ __forceinline__ void compact_count(uint32_t n, uint64_t *mask, uint32_t *blk, F keep) {
  __shared__ uint32_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * kCompactBlock;
  uint32_t c = 0;
#pragma unroll 2
  for (uint32_t r = 0; r < kCompactBlock / 256u; ++r) {
    const uint32_t i = base + r * 256u + threadIdx.x;
    const uint64_t m = __ballot(i < n && keep(i));
    if (lane == 0 && base + r * 256u + w * 64u < n) mask[(base + r * 256u) / 64u + w] = m;
    c += (uint32_t)__popcll(m);
  }
  if (lane == 0) wsum[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Called by one workgroup of 1024 lanes.
__device__ __forceinline__ void compact_scan(uint32_t *blk, uint32_t nblk) {
  __shared__ uint32_t wtot[16];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < nblk; c0 += 1024u) {
    const uint32_t k = c0 + t;
    const uint32_t v = k < nblk ? blk[k] : 0u;
    const uint32_t x = wave_scan32(v, lane);
    if (lane == 63u) wtot[w] = x;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t j = 0; j < w; ++j) before += wtot[j];
    if (k < nblk) blk[k] = before + x - v;
    __syncthreads();
    if (t == 1023u) carry = before + x;
    __syncthreads();
  }
  if (t == 0) blk[nblk] = carry;
}

// Called by the 64 lanes of workgroup blockIdx.x, after compact_scan; nitems: the items the
// mask covers.  A lane writes its word's set bits (a wave with no set bit exits at once).
__device__ __forceinline__ void compact_index(const uint32_t *blk, const uint64_t *mask, uint32_t *idx,
                                              uint32_t nitems) {
  const uint32_t lane = threadIdx.x;
  const uint32_t wi = blockIdx.x * (kCompactBlock / 64u) + lane;
  const uint32_t nw = (nitems + 63u) / 64u;
  const uint64_t m = (lane < kCompactBlock / 64u && wi < nw) ? mask[wi] : 0ull;
  if (__ballot(m != 0ull) == 0ull) return;
  const uint32_t v = (uint32_t)__popcll(m), x = wave_scan32(v, lane);
  uint32_t r = blk[blockIdx.x] + x - v;
  for (uint64_t b = m; b; b &= b - 1ull) idx[r++] = wi * 64u + (uint32_t)__builtin_ctzll(b);
}

}  // namespace gpd
