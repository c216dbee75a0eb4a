// gpd_gather.h — the 16-byte gather the stream stages share, one copy for all three: the IPv4
// reassembly (gpd_ip4reasm.hip: datagram bytes, the new byte store), the stateful assembler
// (gpd_tcpasm.hip: output bytes, the new store) and the stream assembly (gpd_tcpstream.hip: the
// streams' bytes).  This is their bandwidth path.
//
//   GatherPiece     what the two stateful stages hand the gather (16 B); plain C++, so the walk
//                   headers that build pieces also compile without HIP
//   gather_kernel   a wave per 64 consecutive records, whose bytes are one contiguous run of the
//                   output, in 16-byte-aligned output chunks
//   launch_gather   its one launch
//
// What differs between the users is a source object passed by value: how record i is loaded
// from global memory, and the one or two byte arrays the records' bytes lie in.  The kernel has
// internal linkage: every translation unit that includes this compiles its own instantiation.
#pragma once
#include <stdint.h>

namespace gpd {

// One slice a gather copies (16 B): bytes [src, src + len) of source `where` to the output at pos.
struct GatherPiece {
  uint32_t src, len, pos, where;
};

}  // namespace gpd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "gpd_stream_util.h"

namespace gpd {
namespace {

constexpr uint32_t kGatherWaves = 4;  // waves per gather workgroup

// A wave's record as the chunks see it (LDS, 24 bytes).
struct GatherRec {
  uint64_t pos;  // where its bytes start in the output
  int64_t src;   // where they start in its source
  uint32_t len, where;
};
constexpr int64_t kNoSrc = (int64_t)1 << 62;  // a record with no bytes to read: zeros
static_assert(sizeof(GatherPiece) == 16 && sizeof(GatherRec) == 24, "the gather's layouts");

// The N byte arrays of a source object, indexed by GatherRec::where.  lim: len rounded up to 16,
// the end of what a 16-byte load may touch.  A source object derives from this and adds
//   __device__ GatherRec load(uint64_t i) const     record i from global memory (where < N)
template <uint32_t N>
struct GatherBases {
  static constexpr uint32_t kSources = N;
  const uint8_t *base[N];
  uint64_t len[N], lim[N];
  void set(uint32_t w, const uint8_t *b, uint64_t l) {
    base[w] = b;
    len[w] = b ? l : 0;
    lim[w] = (len[w] + 15ull) & ~15ull;
  }
};

// The pieces of the two stateful stages: two sources (their constants name which is which).
struct PieceSource : GatherBases<2> {
  const GatherPiece *pieces;
  __device__ __forceinline__ GatherRec load(uint64_t i) const {
    const v4u a = *reinterpret_cast<const v4u *>(pieces + i);  // src, len, pos, where
    return GatherRec{a.z, (int64_t)a.x, a.y, a.w & 1u};
  }
};

// A wave per 64 consecutive records; their bytes are the contiguous run [P0, P1) of the output.
// The wave owns the 16-byte output chunks that start inside its run.  A chunk is assembled in
// registers from the records it covers — one record for all but the chunks at record borders —
// each two aligned 16-byte source loads shifted together and masked, and leaves as one 16-byte
// non-temporal store.  Records can be 0 to 15 bytes long, so the run's last chunk may reach into
// any number of later waves' records: that chunk, and the output's ragged end, go byte by byte.
// Nothing is read outside [0, lim) of a source, nothing is stored at or past nbytes.
template <class Src>
__global__ __launch_bounds__(64 * kGatherWaves) void gather_kernel(Src S, uint32_t np, uint8_t *out, uint64_t nbytes) {
  __shared__ GatherRec s_rec[kGatherWaves][64];
  constexpr bool two = Src::kSources == 2;
  static_assert(Src::kSources == 1 || two, "one or two sources");
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t r0 = ((uint64_t)blockIdx.x * kGatherWaves + w) * 64u;
  const bool wlive = r0 < np;
  const uint64_t ri = r0 + lane;
  GatherRec q{~0ull, kNoSrc, 0u, 0u};
  if (ri < np) q = S.load(ri);
  s_rec[w][lane] = q;
  __syncthreads();
  if (!wlive) return;
  const uint32_t nl = np - r0 < 64ull ? (uint32_t)(np - r0) : 64u;
  const uint64_t P0 = shfl64(q.pos, 0), P1 = shfl64(q.pos + q.len, (int)nl - 1);
  const GatherRec *rec = s_rec[w];
  const uint64_t c_lo = (P0 + 15ull) >> 4, c_hi = (P1 + 15ull) >> 4;
  const v4u z{0u, 0u, 0u, 0u};
  const uint8_t *base0 = S.base[0], *base1 = S.base[two ? 1 : 0];
  const uint64_t lim0 = S.lim[0], lim1 = S.lim[two ? 1 : 0];
  for (uint64_t c = c_lo + lane; c < c_hi; c += 64ull) {
    const uint64_t cb = c << 4, ce = cb + 16ull;
    if (ce > P1 && P1 < nbytes) {  // reaches into later waves' records: byte by byte
      const uint64_t end = ce < nbytes ? ce : nbytes;
      uint32_t lo = 0;
#pragma unroll
      for (uint32_t step = 32; step >= 1u; step >>= 1)
        if (rec[lo + step].pos <= cb) lo += step;
      uint64_t k = r0 + lo, x = cb;
      while (x < end && k < np) {
        const GatherRec R = S.load(k);
        if (R.pos > x) break;  // (cannot happen: the records' bytes are back to back)
        if (R.pos + R.len <= x) {
          ++k;
          continue;
        }
        const uint32_t wh = two ? R.where : 0u;
        const uint64_t sa = (uint64_t)R.src + (x - R.pos);  // (kNoSrc: past every len)
        out[x] = sa < S.len[wh] ? S.base[wh][sa] : (uint8_t)0;
        ++x;
      }
      continue;
    }
    const uint64_t end = ce < P1 ? ce : P1;  // (end < ce: P1 == nbytes, the output's ragged end)
    v4u V = z;
    uint64_t x = cb;
    while (x < end) {
      uint32_t lo = 0;  // the last record with pos <= x: the one x lies in
#pragma unroll
      for (uint32_t step = 32; step >= 1u; step >>= 1)
        if (rec[lo + step].pos <= x) lo += step;
      const GatherRec t = rec[lo];
      const uint64_t qe = t.pos + t.len;
      if (qe <= x) break;  // (cannot happen: x < P1)
      const uint64_t pe = qe < end ? qe : end;
      const int32_t k0 = (int32_t)(x - cb), k1 = (int32_t)(pe - cb);
      // (two sources: the bases stay in scalar registers, indexing S.base by lane would be a load
      // per chunk; one source: no select at all)
      const bool hi = two && t.where;
      V |= src16_of(hi ? base1 : base0, hi ? lim1 : lim0, t.src + (int64_t)(x - t.pos) - k0) & byte_mask(k0, k1);
      x = pe;
    }
    if (end == ce) {
      __builtin_nontemporal_store(V, reinterpret_cast<v4u *>(out + cb));
    } else {
      const uint32_t wds[4] = {V.x, V.y, V.z, V.w};
      const uint32_t vend = (uint32_t)(end - cb);
#pragma unroll
      for (uint32_t b = 0; b < 16u; ++b)
        if (b < vend) out[cb + b] = (uint8_t)(wds[b >> 2] >> ((b & 3u) * 8u));
    }
  }
}

// The gather of np records into out[0, nbytes).  Nothing to do, nothing launched.
template <class Src>
inline void launch_gather(const Src &S, uint32_t np, uint8_t *out, uint64_t nbytes, hipStream_t s) {
  if (!np || !nbytes) return;
  const uint32_t nwave = (np + 63u) / 64u;
  hipLaunchKernelGGL(gather_kernel<Src>, dim3((nwave + kGatherWaves - 1u) / kGatherWaves), dim3(64 * kGatherWaves), 0, s,
                     S, np, out, nbytes);
}

}  // namespace
}  // namespace gpd
#endif  // __HIPCC__
