// gpd_radix_sort.h — the device sort the hand-off (gpd_tcpseg.hip), the connection tracker
// (gpd_tcptrack.hip) and the IPv4 reassembly (gpd_ip4reasm.hip) share, one copy for the three: a
// stable LSD radix sort of (key, index) pairs, 8 bits a pass.  Each pass is three launches and no
// kernel waits on another workgroup: passes are separated by launch boundaries only.
//
//   sort_hist_kernel    per workgroup tile of kSortTile pairs: counts per digit, [digit][tile]
//   sort_scan_kernel    one workgroup: exclusive scan of the [digit][tile] counts in place
//   sort_scatter_kernel stable ranks inside the tile: per wave eight ballots give the lanes
//                       with the same digit, the rank is the popcount below the lane, and the
//                       waves' bases are scanned in wave order through LDS.  Where a pair goes is
//                       the caller's Sink: the other pair array, or in the last pass what the user
//                       keeps (the hand-off gathers what the pair stands for, reassembly splits
//                       the pair into its order[] and skey[]).
//
// The kernels have internal linkage: every translation unit that includes this compiles its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gpd_compact.h"

namespace gpd {
namespace {

constexpr uint32_t kSortThreads = 1024;
constexpr uint32_t kSortWaves = kSortThreads / 64u;
constexpr uint32_t kSortRounds = 8;     // pairs per lane
constexpr uint32_t kSortTile = kSortThreads * kSortRounds;  // pairs per workgroup (tcpassembly.SORT_TILE)
constexpr uint32_t kWaveSpan = 64u * kSortRounds;           // consecutive pairs of one wave
constexpr uint32_t kSortScanRound = 16384;                  // [digit][tile] counts the scan takes between barriers

struct SortArgs {
  uint32_t cnt;    // pairs
  uint32_t ntile;  // ceil(cnt / kSortTile)
  uint32_t *hist;  // [256][ntile]
};

// The plain sink: the pair goes to its place in the other array.
struct PairSink {
  uint2 *out;
  __device__ __forceinline__ void operator()(uint32_t pos, uint2 p) const { out[pos] = p; }
};

// The lanes of the wave whose digit equals this lane's (invalid lanes match nobody): eight
// ballots, one per bit.  Called by all 64 lanes.
__device__ __forceinline__ uint64_t match_digit(bool valid, uint32_t d) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < 8u; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(valid && bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// A wave owns kWaveSpan consecutive pairs of its workgroup's tile, lane l those at l, l + 64, ...
__device__ __forceinline__ uint32_t tile_item(uint32_t w, uint32_t lane, uint32_t r) {
  return blockIdx.x * kSortTile + w * kWaveSpan + r * 64u + lane;
}

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(SortArgs A, const uint2 *in, uint32_t shift) {
  __shared__ uint32_t h[256];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  if (t < 256u) h[t] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kSortRounds; ++r) {
    const uint32_t j = tile_item(w, lane, r);
    const bool valid = j < A.cnt;
    const uint32_t d = valid ? (in[j].x >> shift) & 255u : 0u;
    const uint64_t m = match_digit(valid, d);
    if (valid && (m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&h[d], (uint32_t)__popcll(m));
  }
  __syncthreads();
  if (t < 256u) A.hist[t * A.ntile + blockIdx.x] = h[t];
}

// One workgroup: exclusive scan of hist[256 * ntile] in place, sixteen consecutive entries a lane
// a round (16,384 entries between barriers: 2^24 pairs make 2^19 entries, 32 rounds).
__global__ __launch_bounds__(1024) void sort_scan_kernel(SortArgs A) {
  __shared__ uint32_t wtot[16];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint32_t nent = 256u * A.ntile;  // a multiple of 16
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < nent; c0 += kSortScanRound) {
    const uint32_t k = c0 + 16u * t;
    uint4 v[4];
    uint32_t s = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
      v[q] = k < nent ? *reinterpret_cast<const uint4 *>(A.hist + k + 4u * q) : make_uint4(0u, 0u, 0u, 0u);
      s += v[q].x + v[q].y + v[q].z + v[q].w;
    }
    const uint32_t x = wave_scan32(s, lane);
    if (lane == 63u) wtot[w] = x;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t j = 0; j < w; ++j) before += wtot[j];
    uint32_t e = before + x - s;
    if (k < nent) {
#pragma unroll
      for (uint32_t q = 0; q < 4u; ++q) {
        *reinterpret_cast<uint4 *>(A.hist + k + 4u * q) = make_uint4(e, e + v[q].x, e + v[q].x + v[q].y,
                                                                     e + v[q].x + v[q].y + v[q].z);
        e += v[q].x + v[q].y + v[q].z + v[q].w;
      }
    }
    __syncthreads();
    if (t == 1023u) carry = before + x;
    __syncthreads();
  }
}

// Stable scatter of one tile.  base[w][d] ends up as the place of wave w's first pair with digit
// d: the tile's scanned [d][tile] word plus the counts of the waves before it; inside the wave a
// pair's rank is the pairs of its digit in earlier rounds (the leader lane moves the base on)
// plus the matching lanes below it.  sink(pos, pair) puts the pair (or what it stands for) at
// its place.
template <class Sink>
__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(SortArgs A, const uint2 *in, uint32_t shift,
                                                                      Sink sink) {
  __shared__ uint32_t base[kSortWaves][256];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  for (uint32_t k = t; k < kSortWaves * 256u; k += kSortThreads) (&base[0][0])[k] = 0;
  __syncthreads();
  uint2 p[kSortRounds];
  uint32_t below[kSortRounds], tot[kSortRounds];
#pragma unroll
  for (uint32_t r = 0; r < kSortRounds; ++r) {
    const uint32_t j = tile_item(w, lane, r);
    const bool valid = j < A.cnt;
    p[r] = valid ? in[j] : make_uint2(0u, 0u);
    const uint32_t d = (p[r].x >> shift) & 255u;
    const uint64_t m = match_digit(valid, d);
    below[r] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    tot[r] = (valid && below[r] == 0u) ? (uint32_t)__popcll(m) : 0u;  // the digit's leader lane
    if (tot[r]) base[w][d] += tot[r];  // (one leader per digit: no two lanes on one word)
    __builtin_amdgcn_wave_barrier();   // rounds stay in order across the wave's lanes
  }
  __syncthreads();
  if (t < 256u) {
    uint32_t b = A.hist[t * A.ntile + blockIdx.x];
    for (uint32_t k = 0; k < kSortWaves; ++k) {
      const uint32_t c = base[k][t];
      base[k][t] = b;
      b += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kSortRounds; ++r) {
    const bool valid = tile_item(w, lane, r) < A.cnt;
    const uint32_t d = (p[r].x >> shift) & 255u;
    const uint32_t b = base[w][d];  // every lane reads before the leader moves it on
    __builtin_amdgcn_wave_barrier();
    if (tot[r]) base[w][d] = b + tot[r];
    __builtin_amdgcn_wave_barrier();
    if (valid) sink(b + below[r], p[r]);
  }
}

// Passes of the sort for keys in [0, max_key]: ceil(bitlen(max_key) / 8), at least one.
inline uint32_t sort_passes(uint32_t max_key) {
  uint32_t bits = 0;
  for (uint32_t v = max_key; v; v >>= 1) ++bits;
  return std::max(1u, (bits + 7u) / 8u);
}

// The whole sort of cnt pairs in `a` (b: the other array, hist: [256][ntile] words), passes
// 0 .. passes - 2 with the plain sink; the caller launches the last pass with its own sink from
// the returned source array.
inline const uint2 *sort_leading_passes(SortArgs A, uint2 *a, uint2 *b, uint32_t passes, hipStream_t s) {
  uint2 *src = a, *dst = b;
  for (uint32_t p = 0; p + 1 < passes; ++p) {
    hipLaunchKernelGGL(sort_hist_kernel, dim3(A.ntile), dim3(kSortThreads), 0, s, A, src, 8u * p);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, s, A);
    hipLaunchKernelGGL(sort_scatter_kernel<PairSink>, dim3(A.ntile), dim3(kSortThreads), 0, s, A, src, 8u * p,
                       PairSink{dst});
    std::swap(src, dst);
  }
  return src;
}
template <class Sink>
inline void sort_last_pass(SortArgs A, const uint2 *src, uint32_t passes, Sink sink, hipStream_t s) {
  const uint32_t shift = 8u * (passes - 1u);
  hipLaunchKernelGGL(sort_hist_kernel, dim3(A.ntile), dim3(kSortThreads), 0, s, A, src, shift);
  hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(sort_scatter_kernel<Sink>, dim3(A.ntile), dim3(kSortThreads), 0, s, A, src, shift, sink);
}

}  // namespace
}  // namespace gpd
