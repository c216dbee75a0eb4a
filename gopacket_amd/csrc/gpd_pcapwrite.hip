// gpd_pcapwrite.hip — the kept packets of a device batch as a pcap stream (pcapgo.Writer,
// pcapgo/write.go:80-129) or as a new dense batch: include/gpd_pcapwrite.h.
//
// A stream compaction over variable-length records.  Packet i takes a slot of 16 + caplen bytes
// (pcap form) or round_up(caplen, 16) bytes (batch form) when it is kept and lies before the
// first kept packet WritePacket would reject, else 0; the slots' exclusive prefix sum (u64) is
// where each record goes.  Four launches, none of which waits for another workgroup:
//
//   pw_bad_kernel    the first kept packet with caplen > Length: atomicMin on one device word
//   pw_sum_kernel    a 1024-thread workgroup per kScanBlock packets: per-wave slot sums (as
//                    exclusive prefixes inside the block), kept counts, first kept index; the
//                    block's totals
//   pw_scan_kernel   one workgroup: the block totals' exclusive scan in place, for each block the
//                    first kept packet of any later block, and the result words the host reads
//   pw_copy_kernel   a wave per 64 consecutive packets, whose records are one contiguous run
//                    [P0, P1) of the output.  Lanes walk the run in 16-byte aligned output
//                    chunks; a chunk is put together in registers from the header words and the
//                    source bytes of the (at most two) records it overlaps, found by a 6-step
//                    binary search over the wave's 64 positions in LDS, and leaves as one
//                    aligned non-temporal 16-byte store.  A wave owns the chunks that START in
//                    its run: the chunk hanging over P1 is completed with the first bytes of the
//                    next kept record's header (at most 15, so they never reach its data; that
//                    record is found through the first-kept indices, not by walking), and the
//                    chunk hanging into P0 belongs to the wave before.  Only the stream's last
//                    chunk can be partial; it is written with byte stores.  The file header
//                    travels as kernel arguments and is written by the wave whose run starts the
//                    records.
//
// Source bytes are read with 16-byte loads at 16-byte steps from `data`, the two that cover an
// unaligned 16-byte span shifted together; a load is issued only where it starts inside
// [0, round_up(data_len, 16)), which is all the batch contract promises, and every byte a
// record needs lies inside it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "gpd_internal.h"
#include "../../include/gpd_pcapwrite.h"

namespace gpd {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kScanBlock = 1024;               // packets per pw_sum_kernel workgroup
constexpr uint32_t kScanWaves = kScanBlock / 64u;   // its waves, one per 64 packets
#ifndef GPD_PW_COPY_WAVES
#define GPD_PW_COPY_WAVES 4  // (A/B builds override it)
#endif
constexpr uint32_t kCopyWaves = GPD_PW_COPY_WAVES;  // waves per pw_copy_kernel workgroup
constexpr uint32_t kFileHeader = 24;

struct WrArgs {
  const uint8_t *data;
  uint32_t dlen;            // data_len (32-bit, as the decode reads it)
  uint64_t lim;             // round_up(data_len, 16): no load starts at or beyond it
  const uint32_t *offset, *caplen;
  uint32_t n;
  const uint64_t *ts;       // pcap form
  const uint32_t *wirelen;  // may be NULL
  const uint8_t *keep;      // may be NULL
  uint32_t scaler;          // 1000, or 1 (GPD_PCAPW_NANOS)
  uint32_t base0;           // bytes in front of the first record: 0, or 24 (the file header) ...
  uint32_t fh[6];           // ... which is these words
  uint8_t *out;
  uint32_t *o_off, *o_len, *o_idx;  // batch form (o_idx may be NULL)
  // scratch of the context
  uint64_t *res;            // [0] stream bytes, [1] records, [2] bad index, [3] its caplen | Length << 32
  uint32_t *badw;           // the first rejected kept packet (kNone: none)
  uint64_t *bsum, *wsum;    // per block: slot bytes -> exclusive prefix; per wave: prefix inside its block
  uint32_t *bcnt, *wcnt;    // the same for the kept counts
  uint32_t *bfirst, *wfirst;  // first kept packet of the block / wave (kNone: none)
  uint32_t *bnext;          // first kept packet of any later block
  uint32_t nblk, nwave;
};

__device__ inline uint64_t shfl_up64(uint64_t v, uint32_t d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
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

// Is packet i written, and where do its bytes lie (clamped to the buffer as the decode does)?
__device__ inline bool kept(const WrArgs &A, uint32_t i, uint32_t bad, uint32_t &off, uint32_t &len) {
  off = len = 0;
  if (i >= A.n || i >= bad) return false;
  if (A.keep && A.keep[i] == 0) return false;
  off = min(A.offset[i], A.dlen);
  len = min(A.caplen[i], A.dlen - off);
  return true;
}
template <bool PCAP>
__device__ inline uint64_t slot_bytes(uint32_t len) {
  return PCAP ? 16ull + len : ((uint64_t)len + 15ull) & ~15ull;
}

// write.go:121-123 over the kept packets: the lowest index wins.
__global__ __launch_bounds__(256) void pw_bad_kernel(WrArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t off = 0, len = 0;
  const bool k = i64 < A.n && kept(A, (uint32_t)i64, kNone, off, len);
  const uint64_t m = __ballot(k && len > A.wirelen[(uint32_t)i64]);
  if (m != 0ull && lane == 0) atomicMin(A.badw, (uint32_t)i64 - lane + (uint32_t)__builtin_ctzll(m));
}

template <bool PCAP>
__global__ __launch_bounds__(1024) void pw_sum_kernel(WrArgs A) {
  __shared__ uint64_t s_sum[kScanWaves];
  __shared__ uint32_t s_cnt[kScanWaves], s_first[kScanWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t gw = blockIdx.x * kScanWaves + w;
  const uint64_t i64 = (uint64_t)gw * 64u + lane;
  const uint32_t bad = *A.badw;
  uint32_t off = 0, len = 0;
  const bool k = i64 < A.n && kept(A, (uint32_t)i64, bad, off, len);
  const uint64_t incl = wave_scan64(k ? slot_bytes<PCAP>(len) : 0ull, lane);
  const uint64_t m = __ballot(k);
  if (lane == 63u) {
    s_sum[w] = incl;
    s_cnt[w] = (uint32_t)__popcll(m);
    s_first[w] = m ? gw * 64u + (uint32_t)__builtin_ctzll(m) : kNone;
  }
  __syncthreads();
  if (lane == 0 && gw < A.nwave) {
    uint64_t s = 0;
    uint32_t c = 0;
    for (uint32_t j = 0; j < w; ++j) {
      s += s_sum[j];
      c += s_cnt[j];
    }
    A.wsum[gw] = s;
    A.wcnt[gw] = c;
    A.wfirst[gw] = s_first[w];
  }
  if (threadIdx.x == 0) {
    uint64_t s = 0;
    uint32_t c = 0, f = kNone;
    for (uint32_t j = 0; j < kScanWaves; ++j) {
      s += s_sum[j];
      c += s_cnt[j];
      f = min(f, s_first[j]);
    }
    A.bsum[blockIdx.x] = s;
    A.bcnt[blockIdx.x] = c;
    A.bfirst[blockIdx.x] = f;
  }
}

// One workgroup, 1024 block totals at a time: forwards the exclusive scans (with a carry), then
// backwards the first kept packet of any later block; last the result words.
__global__ __launch_bounds__(1024) void pw_scan_kernel(WrArgs A) {
  __shared__ uint64_t wtot[16];
  __shared__ uint32_t wcnt[16], wmin[16];
  __shared__ uint64_t carry;
  __shared__ uint32_t ccarry, mcarry;
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  if (t == 0) {
    carry = 0;
    ccarry = 0;
    mcarry = kNone;
  }
  __syncthreads();
  const uint32_t nchunk = (A.nblk + 1023u) / 1024u;
  for (uint32_t c = 0; c < nchunk; ++c) {
    const uint32_t k = c * 1024u + t;
    const uint64_t v = k < A.nblk ? A.bsum[k] : 0ull;
    const uint32_t vc = k < A.nblk ? A.bcnt[k] : 0u;
    const uint64_t x = wave_scan64(v, lane);
    const uint32_t xc = (uint32_t)wave_scan64(vc, lane);
    if (lane == 63u) {
      wtot[w] = x;
      wcnt[w] = xc;
    }
    __syncthreads();
    uint64_t before = carry;
    uint32_t cbefore = ccarry;
    for (uint32_t j = 0; j < w; ++j) {
      before += wtot[j];
      cbefore += wcnt[j];
    }
    if (k < A.nblk) {
      A.bsum[k] = before + x - v;
      A.bcnt[k] = cbefore + xc - vc;
    }
    __syncthreads();
    if (t == 1023u) {
      carry = before + x;
      ccarry = cbefore + xc;
    }
    __syncthreads();
  }
  for (uint32_t c = nchunk; c-- > 0u;) {
    const uint32_t k = c * 1024u + t;
    uint32_t x = k < A.nblk ? A.bfirst[k] : kNone;  // -> min over lanes >= lane
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t y = __shfl_down(x, d, 64);
      if (lane + d < 64u) x = min(x, y);
    }
    const uint32_t y1 = __shfl_down(x, 1, 64);
    uint32_t after = lane < 63u ? y1 : kNone;  // min over lanes > lane
    if (lane == 0) wmin[w] = x;
    __syncthreads();
    after = min(after, mcarry);
    for (uint32_t j = w + 1; j < 16u; ++j) after = min(after, wmin[j]);
    if (k < A.nblk) A.bnext[k] = after;
    __syncthreads();
    if (t == 0) {
      uint32_t mm = mcarry;
      for (uint32_t j = 0; j < 16u; ++j) mm = min(mm, wmin[j]);
      mcarry = mm;
    }
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t bad = *A.badw;
    A.res[0] = (uint64_t)A.base0 + carry;
    A.res[1] = ccarry;
    A.res[2] = bad == kNone ? ~0ull : (uint64_t)bad;
    uint64_t lens = 0;
    if (bad != kNone) {
      uint32_t off = 0, len = 0;
      (void)kept(A, bad, kNone, off, len);
      lens = (uint64_t)len | ((uint64_t)(A.wirelen ? A.wirelen[bad] : len) << 32);
    }
    A.res[3] = lens;
  }
}

// ---- 16 bytes at a time -----------------------------------------------------------------------
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
// data[a, a + 16) for a signed byte position; bytes no load may fetch read as zero (the callers
// mask them away: they are never a record's)
__device__ inline v4u src16(const WrArgs &A, int64_t a) {
  const int64_t a0 = a & ~(int64_t)15;
  const uint32_t s = (uint32_t)(a & 15);
  const v4u z{0u, 0u, 0u, 0u};
#ifdef GPD_PW_NT_LOADS  // (A/B)
#define PW_LD(p) __builtin_nontemporal_load(reinterpret_cast<const v4u *>(p))
#else
#define PW_LD(p) (*reinterpret_cast<const v4u *>(p))
#endif
  const v4u lo = (a0 >= 0 && (uint64_t)a0 < A.lim) ? PW_LD(A.data + a0) : z;
  const v4u hi = (s != 0u && a0 + 16 >= 0 && (uint64_t)(a0 + 16) < A.lim) ? PW_LD(A.data + a0 + 16) : z;
  return bytes_from(lo, hi, s);
}

struct Rec {       // a wave's packet as the chunks see it (LDS, 32 bytes)
  uint64_t pos;    // where its record starts in the output
  uint32_t off, len;
  uint32_t h[4];   // the pcap record header
};

template <bool PCAP>
__global__ __launch_bounds__(64 * kCopyWaves) void pw_copy_kernel(WrArgs A) {
  __shared__ Rec s_rec[kCopyWaves][64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t gw = blockIdx.x * kCopyWaves + w;
  const bool live = gw < A.nwave;
  const uint32_t blk = gw / kScanWaves;
  const uint64_t i64 = (uint64_t)gw * 64u + lane;
  const uint32_t i = (uint32_t)i64;
  const uint32_t bad = *A.badw;
  uint32_t off = 0, len = 0;
  const bool k = live && i64 < A.n && kept(A, i, bad, off, len);
  const uint64_t km = __ballot(k);
  const uint64_t sz = k ? slot_bytes<PCAP>(len) : 0ull;
  const uint64_t incl = wave_scan64(sz, lane);
  const uint64_t total = shfl64(incl, 63);
  const uint64_t P0 = live ? (uint64_t)A.base0 + A.bsum[blk] + A.wsum[gw] : 0ull;
  const uint64_t P1 = P0 + total;
  Rec r;
  r.pos = P0 + incl - sz;
  r.off = off;
  r.len = len;
  r.h[0] = r.h[1] = r.h[2] = r.h[3] = 0;
  if (k) {
    if (PCAP) {
      const uint64_t ts = A.ts[i];
      r.h[0] = (uint32_t)(ts / 1000000000ull);
      r.h[1] = (uint32_t)(ts % 1000000000ull) / A.scaler;
      r.h[2] = len;
      r.h[3] = A.wirelen ? A.wirelen[i] : len;
    } else {
      const uint32_t j = A.bcnt[blk] + A.wcnt[gw] + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
      A.o_off[j] = (uint32_t)r.pos;
      A.o_len[j] = len;
      if (A.o_idx) A.o_idx[j] = i;
    }
  }
  s_rec[w][lane] = r;
  __syncthreads();
  if (total == 0ull) return;  // nothing of this wave's is kept
  const Rec *rec = s_rec[w];

  // The header of the kept record that follows the run: its first bytes complete the last chunk.
  v4u Hn{0u, 0u, 0u, 0u};
  bool has_next = false;
  if (PCAP && (P1 & 15ull)) {
    const uint32_t g = blk * kScanWaves + lane;
    uint32_t nx = (lane < kScanWaves && g > gw && g < A.nwave) ? A.wfirst[g] : kNone;
    nx = wave_min32(nx);
    if (nx == kNone) nx = A.bnext[blk];
    if (nx != kNone) {
      uint32_t noff, nlen;
      (void)kept(A, nx, bad, noff, nlen);
      const uint64_t ts = A.ts[nx];
      Hn = v4u{(uint32_t)(ts / 1000000000ull), (uint32_t)(ts % 1000000000ull) / A.scaler, nlen,
               A.wirelen ? A.wirelen[nx] : nlen};
      has_next = true;
    }
  }

  const bool first = PCAP && P0 == (uint64_t)A.base0;  // this run starts the records
  const uint64_t c_lo = first ? 0ull : (P0 + 15ull) >> 4, c_hi = (P1 + 15ull) >> 4;
  const uint64_t nch = c_hi - c_lo;
  const v4u z{0u, 0u, 0u, 0u};
  for (uint64_t it = 0; it * 64ull < nch; ++it) {
    const uint64_t c = c_lo + it * 64ull + lane;
    if (c >= c_hi) break;  // (the last round's upper lanes)
    const uint64_t cb = c << 4, ce = cb + 16ull;
    v4u V = z;
    uint64_t x = cb;
    if (PCAP && cb < P0) {  // the file header's 24 bytes: chunk 0, and bytes 0..7 of chunk 1
      V = cb == 0ull ? v4u{A.fh[0], A.fh[1], A.fh[2], A.fh[3]} : v4u{A.fh[4], A.fh[5], 0u, 0u};
      x = ce < P0 ? ce : P0;
    }
#pragma unroll
    for (int rnd = 0; rnd < (PCAP ? 2 : 1); ++rnd) {  // records are >= 16 bytes: at most two
      if (x >= (ce < P1 ? ce : P1)) break;
      uint32_t lo = 0;  // the last packet with pos <= x: the record x lies in
#pragma unroll
      for (uint32_t step = 32; step >= 1u; step >>= 1)
        if (rec[lo + step].pos <= x) lo += step;
      const Rec q = rec[lo];
      const int64_t d = (int64_t)(cb - q.pos);  // the chunk's first byte, in the record's bytes
      if (PCAP) {
        const v4u H{q.h[0], q.h[1], q.h[2], q.h[3]};
        if (d < 16) V |= d >= 0 ? bytes_from(H, z, (uint32_t)d) : bytes_from(z, H, (uint32_t)(16 + d));
        const int64_t e = 16 + (int64_t)q.len - d;  // the record's end, in the chunk's bytes
        const int64_t k0 = d < 16 ? 16 - d : 0, k1 = e < 16 ? e : 16;
        if (k1 > k0) V |= src16(A, (int64_t)q.off + d - 16) & byte_mask((int32_t)k0, (int32_t)k1);
        x = q.pos + 16ull + q.len;
      } else {  // a 16-aligned slot: its bytes, then zeros
        const int64_t e = (int64_t)q.len - d, k1 = e < 16 ? e : 16;
        if (k1 > 0) V |= src16(A, (int64_t)q.off + d) & byte_mask(0, (int32_t)k1);
        x = ce;
      }
    }
    uint32_t vend = 16;
    if (PCAP && x < ce) {  // x == P1
      if (has_next) V |= bytes_from(z, Hn, (uint32_t)(ce - x));
      else vend = (uint32_t)(x - cb);
    }
    if (vend == 16u) {
#ifdef GPD_PW_PLAIN_STORES  // (A/B)
      *reinterpret_cast<v4u *>(A.out + cb) = V;
#else
      __builtin_nontemporal_store(V, reinterpret_cast<v4u *>(A.out + cb));
#endif
    } else {  // the stream's ragged end
      const uint32_t wds[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
      for (uint32_t b = 0; b < 16u; ++b)
        if (b < vend) A.out[cb + b] = (uint8_t)(wds[b >> 2] >> ((b & 3u) * 8u));
    }
  }
}

// A stream of nothing but the file header.
__global__ __launch_bounds__(64) void pw_head_kernel(WrArgs A) {
  const uint32_t t = threadIdx.x;
  if (t < kFileHeader) A.out[t] = (uint8_t)(A.fh[t >> 2] >> ((t & 3u) * 8u));
}

void file_header_words(uint32_t flags, uint32_t snaplen, uint32_t linktype, uint32_t w[6]) {
  w[0] = (flags & GPD_PCAPW_NANOS) ? 0xA1B23C4Du : 0xA1B2C3D4u;  // write.go:82-86
  w[1] = 2u | (4u << 16);                                        // versionMajor, versionMinor
  w[2] = w[3] = 0;                                               // timezone, sigfigs
  w[4] = snaplen;
  w[5] = linktype;
}

// The context's scratch carved into A's arrays, then the scan; res[4] back on the host.
template <bool PCAP>
int scan(gpd_ctx *ctx, const char *who, WrArgs &A, hipStream_t s, uint64_t res[4]) {
  A.nblk = (A.n + kScanBlock - 1u) / kScanBlock;
  A.nwave = (uint32_t)(((uint64_t)A.n + 63u) / 64u);
  const size_t bytes = 64 + (size_t)A.nblk * (8 + 3 * 4) + (size_t)A.nwave * (8 + 2 * 4) + 64;
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 11, bytes));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.res = reinterpret_cast<uint64_t *>(base);
  A.badw = reinterpret_cast<uint32_t *>(base + 32);
  A.bsum = reinterpret_cast<uint64_t *>(base + 64);
  A.wsum = A.bsum + A.nblk;
  A.bcnt = reinterpret_cast<uint32_t *>(A.wsum + A.nwave);
  A.bfirst = A.bcnt + A.nblk;
  A.bnext = A.bfirst + A.nblk;
  A.wcnt = A.bnext + A.nblk;
  A.wfirst = A.wcnt + A.nwave;
  GPD_TRY(hipMemsetAsync(base, 0xFF, 64, s));
  if (PCAP && A.wirelen) hipLaunchKernelGGL(pw_bad_kernel, dim3((A.n + 255u) / 256u), dim3(256), 0, s, A);
  hipLaunchKernelGGL(pw_sum_kernel<PCAP>, dim3(A.nblk), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(pw_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  GPD_TRY(hipGetLastError());
  GPD_TRY(hipMemcpyAsync(res, A.res, 32, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}

int check_in(const char *who, gpd_ctx *ctx, const gpd_batch *in) {
  if (!ctx || !in) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  if (in->n > 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 256)", who, (unsigned long long)in->n);
  if (in->n && (!in->data || !in->offset || !in->caplen))
    return set_error(GPD_ERR_INVALID, "%s: batch data/offset/caplen must be non-NULL", who);
  if (in->data_len >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: data_len %llu outside the 32-bit offset range", who,
                     (unsigned long long)in->data_len);
  return GPD_OK;
}

void fill_in(WrArgs &A, const gpd_batch *in, const uint8_t *keep) {
  A.data = in->data;
  A.dlen = (uint32_t)in->data_len;
  A.lim = (in->data_len + 15ull) & ~15ull;
  A.offset = in->offset;
  A.caplen = in->caplen;
  A.n = (uint32_t)in->n;
  A.keep = keep;
}

}  // namespace
}  // namespace gpd

extern "C" {

int gpd_pcap_file_header(uint32_t flags, uint32_t snaplen, uint32_t linktype, uint8_t out[24]) {
  if (!out) return gpd::set_error(GPD_ERR_INVALID, "gpd_pcap_file_header: null out");
  if (flags & ~(GPD_PCAPW_NANOS | GPD_PCAPW_FILE_HEADER))
    return gpd::set_error(GPD_ERR_INVALID, "gpd_pcap_file_header: unknown flags 0x%x", flags);
  uint32_t w[6];
  gpd::file_header_words(flags, snaplen, linktype, w);
  for (int k = 0; k < 24; k++) out[k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));  // little-endian
  return GPD_OK;
}

int gpd_pcap_write(gpd_ctx *ctx, const gpd_batch *in, const uint64_t *ts_ns, const uint32_t *wirelen,
                   const uint8_t *keep, uint32_t flags, uint32_t snaplen, uint32_t linktype,
                   uint8_t *out, uint64_t out_cap,
                   uint64_t *n_written, uint64_t *bytes, uint64_t *bad_index, void *stream) {
  using namespace gpd;
  const char *who = "gpd_pcap_write";
  int rc = check_in(who, ctx, in);
  if (rc) return rc;
  if (!n_written || !bytes || !bad_index) return set_error(GPD_ERR_INVALID, "%s: null result pointer", who);
  *n_written = 0;
  *bytes = 0;
  *bad_index = ~0ull;
  if (flags & ~(GPD_PCAPW_NANOS | GPD_PCAPW_FILE_HEADER))
    return set_error(GPD_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (in->n && !ts_ns)
    return set_error(GPD_ERR_INVALID, "%s: ts_ns is required (a zero Timestamp's time.Now() is the caller's)", who);
  if ((!out && out_cap) || ((uintptr_t)out & 15u))
    return set_error(GPD_ERR_INVALID, "%s: out must be a 16-byte aligned buffer of out_cap bytes", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  WrArgs A{};
  fill_in(A, in, keep);
  A.ts = ts_ns;
  A.wirelen = wirelen;
  A.scaler = (flags & GPD_PCAPW_NANOS) ? 1u : 1000u;
  A.base0 = (flags & GPD_PCAPW_FILE_HEADER) ? kFileHeader : 0u;
  file_header_words(flags, snaplen, linktype, A.fh);
  A.out = out;
  uint64_t res[4] = {A.base0, 0, ~0ull, 0};
  if (A.n) {
    rc = scan<true>(ctx, who, A, s, res);
    if (rc) return rc;
  }
  *bytes = res[0];
  *n_written = res[1];
  *bad_index = res[2];
  if (out || out_cap) {
    if (res[0] > out_cap)
      return set_error(GPD_ERR_INVALID, "%s: the stream takes %llu bytes (%llu records), out_cap is %llu", who,
                       (unsigned long long)res[0], (unsigned long long)res[1], (unsigned long long)out_cap);
    if (res[1]) {
      hipLaunchKernelGGL(pw_copy_kernel<true>, dim3((A.nwave + kCopyWaves - 1u) / kCopyWaves),
                         dim3(64 * kCopyWaves), 0, s, A);
      GPD_TRY(hipGetLastError());
    } else if (A.base0) {
      hipLaunchKernelGGL(pw_head_kernel, dim3(1), dim3(64), 0, s, A);
      GPD_TRY(hipGetLastError());
    }
  }
  if (res[2] != ~0ull)
    return set_error(GPD_ERR_PCAP, "invalid capture info (packet %llu: capture length %u, length %u):  capture length > length",
                     (unsigned long long)res[2], (uint32_t)res[3], (uint32_t)(res[3] >> 32));
  return GPD_OK;
}

int gpd_batch_select(gpd_ctx *ctx, const gpd_batch *in, const uint8_t *keep,
                     uint8_t *out_data, uint64_t out_cap, uint32_t *out_offset, uint32_t *out_caplen,
                     uint32_t *out_index, uint64_t max_out, uint64_t *n_out, uint64_t *bytes, void *stream) {
  using namespace gpd;
  const char *who = "gpd_batch_select";
  int rc = check_in(who, ctx, in);
  if (rc) return rc;
  if (!n_out || !bytes) return set_error(GPD_ERR_INVALID, "%s: null result pointer", who);
  *n_out = 0;
  *bytes = 0;
  const bool sizing = !out_data && !out_cap;
  if (!sizing && (!out_data || ((uintptr_t)out_data & 15u)))
    return set_error(GPD_ERR_INVALID, "%s: out_data must be a 16-byte aligned buffer of out_cap bytes", who);
  if (in->n == 0) return GPD_OK;
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  WrArgs A{};
  fill_in(A, in, keep);
  A.out = out_data;
  A.o_off = out_offset;
  A.o_len = out_caplen;
  A.o_idx = out_index;
  uint64_t res[4];
  rc = scan<false>(ctx, who, A, s, res);
  if (rc) return rc;
  *bytes = res[0];
  *n_out = res[1];
  if (res[0] >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: the kept packets take %llu bytes, beyond the 32-bit offset range", who,
                     (unsigned long long)res[0]);
  if (sizing) return GPD_OK;
  if (res[0] > out_cap || res[1] > max_out)
    return set_error(GPD_ERR_INVALID, "%s: %llu packets in %llu bytes, out_cap is %llu and max_out %llu", who,
                     (unsigned long long)res[1], (unsigned long long)res[0], (unsigned long long)out_cap,
                     (unsigned long long)max_out);
  if (res[1] == 0) return GPD_OK;
  if (!out_offset || !out_caplen) return set_error(GPD_ERR_INVALID, "%s: null out_offset / out_caplen", who);
  hipLaunchKernelGGL(pw_copy_kernel<false>, dim3((A.nwave + kCopyWaves - 1u) / kCopyWaves), dim3(64 * kCopyWaves),
                     0, s, A);
  GPD_TRY(hipGetLastError());
  return GPD_OK;
}

}  // extern "C"
