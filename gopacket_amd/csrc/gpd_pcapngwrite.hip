// gpd_pcapngwrite.hip — the blocks of a pcapng stream (pcapgo.NgWriter, pcapgo/ngwrite.go):
// section, interface and statistics blocks built on the host, and the kept packets of a device
// batch as enhanced packet blocks built on the device: include/gpd_pcapngwrite.h.
//
// The device part is the stream compaction of gpd_pcapwrite.hip over another record form.
// Packet i takes 32 + round_up(caplen, 4) bytes when it is kept and lies before the first kept
// packet WritePacket would reject, else 0; the sizes' exclusive prefix sum (u64) is where each
// record goes.  Four launches, none of which waits for another workgroup:
//
//   ngw_bad_kernel   the first kept packet with ifindex >= n_ifaces or caplen > Length: atomicMin
//                    on one device word (which of the two it failed is read off that packet
//                    afterwards, the interface check first as in ngwrite.go:357-365)
//   ngw_sum_kernel   a 1024-thread workgroup per kScanBlock packets: per-wave record sums (as
//                    exclusive prefixes inside the block), first kept index; the block's totals
//   ngw_scan_kernel  one workgroup: the block totals' exclusive scan in place, for each block the
//                    first kept packet of any later block, and the result words the host reads
//   ngw_copy_kernel  a wave per 64 consecutive packets, whose records are one contiguous run
//                    [P0, P1) of the output.  Lanes walk the run in 16-byte aligned output
//                    chunks.  The prefix and every record are multiples of 4 bytes, so each of a
//                    chunk's four words belongs to one record and is a header word, a data word
//                    (its tail bytes zero where the padding starts) or the trailer; a record is
//                    at least 32 bytes, so a chunk overlaps at most two, found by a 6-step binary
//                    search over the wave's 64 positions in LDS.  The chunk leaves as one aligned
//                    non-temporal 16-byte store.  A wave owns the chunks that START in its run:
//                    the chunk hanging over P1 is completed with the first words of the next kept
//                    record's header (at most 12 bytes of its 28, so they never reach its data;
//                    that record is found through the first-kept indices, not by walking), and
//                    the chunk hanging into P0 belongs to the wave before.  Only the stream's
//                    last chunk can be partial; it is written with word stores.
//
// The prefix (host bytes) is staged into the context's scratch ahead of the scan, whose
// synchronisation also ends the caller's obligation to keep it, and copied to `out` device to
// device ahead of the copy kernel.  The chunk in which the prefix ends and the records begin is
// the first run's: the (at most three) prefix words in it travel as kernel arguments.
//
// Source bytes are read with 16-byte loads at 16-byte steps from `data`, the two that cover an
// unaligned 16-byte span shifted together; a load is issued only where it starts inside
// [0, round_up(data_len, 16)), which is all the batch contract promises, and every byte a
// record needs lies inside it.
#include <hip/hip_runtime.h>

#include <cstring>

#include "gpd_internal.h"
#include "../../include/gpd_pcapngwrite.h"

namespace gpd {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kScanBlock = 1024;               // packets per ngw_sum_kernel workgroup
constexpr uint32_t kScanWaves = kScanBlock / 64u;   // its waves, one per 64 packets
constexpr uint32_t kCopyWaves = 4;                  // waves per ngw_copy_kernel workgroup
constexpr uint32_t kHead = 28;                      // bytes of a record in front of its data
constexpr uint32_t kEnhanced = GPD_PCAPNG_BLOCK_ENHANCED;

struct NgwArgs {
  const uint8_t *data;
  uint32_t dlen;            // data_len (32-bit, as the decode reads it)
  uint64_t lim;             // round_up(data_len, 16): no load starts at or beyond it
  const uint32_t *offset, *caplen;
  uint32_t n;
  const uint64_t *ts;
  const uint32_t *wirelen;  // may be NULL
  const uint32_t *ifindex;  // may be NULL
  const uint8_t *keep;      // may be NULL
  uint32_t n_ifaces;
  uint32_t base0;           // bytes in front of the first record (the prefix) ...
  uint32_t pt[3];           // ... whose words in the chunk it ends in are these
  uint8_t *out;
  // scratch of the context
  uint64_t *res;            // [0] stream bytes, [1] records, [2] bad index, [3] its caplen | Length << 32,
                            // [4] its interface index
  uint32_t *badw;           // the first rejected kept packet (kNone: none)
  uint64_t *bsum, *wsum;    // per block: record bytes -> exclusive prefix; per wave: prefix inside its block
  uint32_t *bcnt;           // per block: kept packets
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
__device__ inline bool kept(const NgwArgs &A, uint32_t i, uint32_t bad, uint32_t &off, uint32_t &len) {
  off = len = 0;
  if (i >= A.n || i >= bad) return false;
  if (A.keep && A.keep[i] == 0) return false;
  off = min(A.offset[i], A.dlen);
  len = min(A.caplen[i], A.dlen - off);
  return true;
}
__device__ inline uint32_t pad4(uint32_t len) { return (len + 3u) & ~3u; }
__device__ inline uint64_t rec_bytes(uint32_t len) { return 32ull + (((uint64_t)len + 3ull) & ~3ull); }
// the block's total length field, in 32 bits as ngwrite.go:367-369 computes it
__device__ inline uint32_t rec_total(uint32_t len) { return 32u + pad4(len); }

// ngwrite.go:357-359 and :363-365 over the kept packets: the lowest index wins.
__global__ __launch_bounds__(256) void ngw_bad_kernel(NgwArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t i = (uint32_t)i64;
  uint32_t off = 0, len = 0;
  const bool k = i64 < A.n && kept(A, i, kNone, off, len);
  const bool rej = k && ((A.ifindex ? A.ifindex[i] : 0u) >= A.n_ifaces || (A.wirelen && len > A.wirelen[i]));
  const uint64_t m = __ballot(rej);
  if (m != 0ull && lane == 0) atomicMin(A.badw, i - lane + (uint32_t)__builtin_ctzll(m));
}

__global__ __launch_bounds__(1024) void ngw_sum_kernel(NgwArgs A) {
  __shared__ uint64_t s_sum[kScanWaves];
  __shared__ uint32_t s_cnt[kScanWaves], s_first[kScanWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t gw = blockIdx.x * kScanWaves + w;
  const uint64_t i64 = (uint64_t)gw * 64u + lane;
  const uint32_t bad = *A.badw;
  uint32_t off = 0, len = 0;
  const bool k = i64 < A.n && kept(A, (uint32_t)i64, bad, off, len);
  const uint64_t incl = wave_scan64(k ? rec_bytes(len) : 0ull, lane);
  const uint64_t m = __ballot(k);
  if (lane == 63u) {
    s_sum[w] = incl;
    s_cnt[w] = (uint32_t)__popcll(m);
    s_first[w] = m ? gw * 64u + (uint32_t)__builtin_ctzll(m) : kNone;
  }
  __syncthreads();
  if (lane == 0 && gw < A.nwave) {
    uint64_t s = 0;
    for (uint32_t j = 0; j < w; ++j) s += s_sum[j];
    A.wsum[gw] = s;
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

// One workgroup, 1024 block totals at a time: forwards the exclusive scan (with a carry), then
// backwards the first kept packet of any later block; last the result words.
__global__ __launch_bounds__(1024) void ngw_scan_kernel(NgwArgs A) {
  __shared__ uint64_t wtot[16], wcnt[16];
  __shared__ uint32_t wmin[16];
  __shared__ uint64_t carry, ccarry;
  __shared__ uint32_t mcarry;
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
    const uint64_t vc = k < A.nblk ? A.bcnt[k] : 0ull;
    const uint64_t x = wave_scan64(v, lane);
    const uint64_t xc = wave_scan64(vc, lane);
    if (lane == 63u) {
      wtot[w] = x;
      wcnt[w] = xc;
    }
    __syncthreads();
    uint64_t before = carry, cbefore = ccarry;
    for (uint32_t j = 0; j < w; ++j) {
      before += wtot[j];
      cbefore += wcnt[j];
    }
    if (k < A.nblk) A.bsum[k] = before + x - v;
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
    uint64_t lens = 0, ifx = 0;
    if (bad != kNone) {
      uint32_t off = 0, len = 0;
      (void)kept(A, bad, kNone, off, len);
      lens = (uint64_t)len | ((uint64_t)(A.wirelen ? A.wirelen[bad] : len) << 32);
      ifx = A.ifindex ? A.ifindex[bad] : 0u;
    }
    A.res[3] = lens;
    A.res[4] = ifx;
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
// words [s, s + 4) of the 8 words lo:hi, s in 0..3
__device__ inline v4u words_from(v4u lo, v4u hi, uint32_t s) {
  uint32_t x0 = lo.x, x1 = lo.y, x2 = lo.z, x3 = lo.w, x4 = hi.x, x5 = hi.y, x6 = hi.z;
  if (s & 2u) {
    x0 = x2, x1 = x3, x2 = x4, x3 = x5, x4 = x6;
  }
  if (s & 1u) {
    x0 = x1, x1 = x2, x2 = x3, x3 = x4;
  }
  return v4u{x0, x1, x2, x3};
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
__device__ inline v4u src16(const NgwArgs &A, int64_t a) {
  const int64_t a0 = a & ~(int64_t)15;
  const uint32_t s = (uint32_t)(a & 15);
  const v4u z{0u, 0u, 0u, 0u};
  const v4u lo = (a0 >= 0 && (uint64_t)a0 < A.lim) ? *reinterpret_cast<const v4u *>(A.data + a0) : z;
  const v4u hi = (s != 0u && a0 + 16 >= 0 && (uint64_t)(a0 + 16) < A.lim)
                     ? *reinterpret_cast<const v4u *>(A.data + a0 + 16) : z;
  return bytes_from(lo, hi, s);
}

struct Rec {       // a wave's packet as the chunks see it (LDS, 32 bytes)
  uint64_t pos;    // where its record starts in the output
  uint32_t off, len;
  uint32_t ifx, ts_hi, ts_lo, wl;  // header words 2, 3, 4 and 6 (0 and 1 follow from len, 5 is len)
};

__global__ __launch_bounds__(64 * kCopyWaves) void ngw_copy_kernel(NgwArgs A) {
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
  const uint64_t sz = k ? rec_bytes(len) : 0ull;
  const uint64_t incl = wave_scan64(sz, lane);
  const uint64_t total = shfl64(incl, 63);
  const uint64_t P0 = live ? (uint64_t)A.base0 + A.bsum[blk] + A.wsum[gw] : 0ull;
  const uint64_t P1 = P0 + total;
  Rec r;
  r.pos = P0 + incl - sz;
  r.off = off;
  r.len = len;
  r.ifx = r.ts_hi = r.ts_lo = r.wl = 0;
  if (k) {
    const uint64_t ts = A.ts[i];
    r.ifx = A.ifindex ? A.ifindex[i] : 0u;
    r.ts_hi = (uint32_t)(ts >> 32);
    r.ts_lo = (uint32_t)ts;
    r.wl = A.wirelen ? A.wirelen[i] : len;
  }
  s_rec[w][lane] = r;
  __syncthreads();
  if (total == 0ull) return;  // nothing of this wave's is kept
  const Rec *rec = s_rec[w];

  // The header of the kept record that follows the run: its first words complete the last chunk.
  v4u Hn{0u, 0u, 0u, 0u};
  bool has_next = false;
  if (P1 & 15ull) {
    const uint32_t g = blk * kScanWaves + lane;
    uint32_t nx = (lane < kScanWaves && g > gw && g < A.nwave) ? A.wfirst[g] : kNone;
    nx = wave_min32(nx);
    if (nx == kNone) nx = A.bnext[blk];
    if (nx != kNone) {
      uint32_t noff, nlen;
      (void)kept(A, nx, bad, noff, nlen);
      Hn = v4u{kEnhanced, rec_total(nlen), A.ifindex ? A.ifindex[nx] : 0u, 0u};  // (12 bytes at most)
      has_next = true;
    }
  }

  // The run that starts the records also owns the chunk the prefix ends in.
  const bool first = P0 == (uint64_t)A.base0;
  const uint64_t c_lo = first ? P0 >> 4 : (P0 + 15ull) >> 4, c_hi = (P1 + 15ull) >> 4;
  const uint64_t nch = c_hi - c_lo;
  const v4u z{0u, 0u, 0u, 0u};
  for (uint64_t it = 0; it * 64ull < nch; ++it) {
    const uint64_t c = c_lo + it * 64ull + lane;
    if (c >= c_hi) break;  // (the last round's upper lanes)
    const uint64_t cb = c << 4, ce = cb + 16ull;
    v4u V = z;
    uint64_t x = cb;
    if (cb < P0) {  // the prefix's last words (first run only; the words from P0 on are zero in pt)
      V = v4u{A.pt[0], A.pt[1], A.pt[2], 0u};
      x = P0;
    }
#pragma unroll
    for (int rnd = 0; rnd < 2; ++rnd) {  // records are >= 32 bytes: at most two
      if (x >= (ce < P1 ? ce : P1)) break;
      uint32_t lo = 0;  // the last packet with pos <= x: the record x lies in
#pragma unroll
      for (uint32_t step = 32; step >= 1u; step >>= 1)
        if (rec[lo + step].pos <= x) lo += step;
      const Rec q = rec[lo];
      const int64_t d = (int64_t)(cb - q.pos);  // the chunk's first byte, in the record's bytes (a multiple of 4)
      const uint32_t tot = rec_total(q.len);
      if (d < (int64_t)kHead) {  // header words
        const v4u H0{kEnhanced, tot, q.ifx, q.ts_hi}, H1{q.ts_lo, q.len, q.wl, 0u};
        V |= d < 0 ? words_from(z, H0, (uint32_t)(16 + d) >> 2)
                   : d < 16 ? words_from(H0, H1, (uint32_t)d >> 2) : words_from(H1, z, (uint32_t)(d - 16) >> 2);
      }
      const int64_t e = (int64_t)kHead + (int64_t)q.len - d;  // the data's end, in the chunk's bytes
      const int64_t k0 = d < (int64_t)kHead ? (int64_t)kHead - d : 0, k1 = e < 16 ? e : 16;
      if (k1 > k0) V |= src16(A, (int64_t)q.off + d - (int64_t)kHead) & byte_mask((int32_t)k0, (int32_t)k1);
      const int64_t tj = (int64_t)kHead + (int64_t)pad4(q.len) - d;  // the trailer, in the chunk's bytes
      V.x |= tj == 0 ? tot : 0u;
      V.y |= tj == 4 ? tot : 0u;
      V.z |= tj == 8 ? tot : 0u;
      V.w |= tj == 12 ? tot : 0u;
      x = q.pos + rec_bytes(q.len);
    }
    uint32_t vend = 16;
    if (x < ce) {  // x == P1
      if (has_next) V |= words_from(z, Hn, (uint32_t)(ce - x) >> 2);
      else vend = (uint32_t)(x - cb);
    }
    if (vend == 16u) {
      __builtin_nontemporal_store(V, reinterpret_cast<v4u *>(A.out + cb));
    } else {  // the stream's ragged end: one to three words
      uint32_t *o = reinterpret_cast<uint32_t *>(A.out + cb);
      o[0] = V.x;
      if (vend > 4u) o[1] = V.y;
      if (vend > 8u) o[2] = V.z;
    }
  }
}

// The context's scratch carved into A's arrays and the prefix's staging copy; the scan when
// there are packets; res[5] back on the host.  Synchronises `s`, after which `prefix` is free.
int scan(gpd_ctx *ctx, const char *who, NgwArgs &A, const uint8_t *prefix, bool stage, uint8_t **staged,
         hipStream_t s, uint64_t res[5]) {
  A.nblk = (A.n + kScanBlock - 1u) / kScanBlock;
  A.nwave = (uint32_t)(((uint64_t)A.n + 63u) / 64u);
  const size_t arrays = ((size_t)A.nblk * (8 + 3 * 4) + (size_t)A.nwave * (8 + 4) + 15u) & ~(size_t)15;
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 11, 64 + arrays + (stage ? A.base0 : 0u) + 64));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.res = reinterpret_cast<uint64_t *>(base);
  A.badw = reinterpret_cast<uint32_t *>(base + 48);
  A.bsum = reinterpret_cast<uint64_t *>(base + 64);
  A.wsum = A.bsum + A.nblk;
  A.bcnt = reinterpret_cast<uint32_t *>(A.wsum + A.nwave);
  A.bfirst = A.bcnt + A.nblk;
  A.bnext = A.bfirst + A.nblk;
  A.wfirst = A.bnext + A.nblk;
  *staged = base + 64 + arrays;
  if (stage && A.base0) GPD_TRY(hipMemcpyAsync(*staged, prefix, A.base0, hipMemcpyHostToDevice, s));
  if (A.n) {
    GPD_TRY(hipMemsetAsync(base, 0xFF, 64, s));
    if (A.wirelen || A.ifindex || A.n_ifaces == 0)
      hipLaunchKernelGGL(ngw_bad_kernel, dim3((A.n + 255u) / 256u), dim3(256), 0, s, A);
    hipLaunchKernelGGL(ngw_sum_kernel, dim3(A.nblk), dim3(1024), 0, s, A);
    hipLaunchKernelGGL(ngw_scan_kernel, dim3(1), dim3(1024), 0, s, A);
    GPD_TRY(hipGetLastError());
    GPD_TRY(hipMemcpyAsync(res, A.res, 40, hipMemcpyDeviceToHost, s));
  }
  if (A.n || (stage && A.base0)) GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}

// ---- the host-built blocks --------------------------------------------------------------------
// A block under construction: counts always, writes when there is a buffer.
struct Sink {
  uint8_t *p;
  uint64_t n = 0;
  explicit Sink(uint8_t *out) : p(out) {}
  void bytes(const uint8_t *src, size_t k) {  // src NULL: zeros
    if (p && k) {
      if (src) std::memcpy(p + n, src, k);
      else std::memset(p + n, 0, k);
    }
    n += k;
  }
  void u16(uint16_t v) {
    const uint8_t b[2] = {(uint8_t)v, (uint8_t)(v >> 8)};
    bytes(b, 2);
  }
  void u32(uint32_t v) {
    const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    bytes(b, 4);
  }
  // writeOptions :125-150 for a string or []byte value, with `lead` zero bytes in front
  void opt_str(uint16_t code, const uint8_t *s, uint32_t len, uint32_t lead = 0) {
    const uint32_t k = len + lead;
    u16(code);
    u16((uint16_t)k);
    bytes(nullptr, lead);
    bytes(s, len);
    bytes(nullptr, (4u - (k & 3u)) & 3u);
  }
  void opt_time(uint16_t code, uint64_t ts) {  // :151-157: high word first
    u16(code);
    u16(8);
    u32((uint32_t)(ts >> 32));
    u32((uint32_t)ts);
  }
  void opt_u64(uint16_t code, uint64_t v) {  // :158-162
    u16(code);
    u16(8);
    u32((uint32_t)v);
    u32((uint32_t)(v >> 32));
  }
  void opt_u8(uint16_t code, uint8_t v) {  // :168-173: one byte stored in four
    u16(code);
    u16(1);
    u32(v);
  }
};

// A string of the struct as (pointer or NULL for zeros, length); false when it lies outside strs
// or is too long for an option.
bool str_of(const gpd_pcapng_str &s, const uint8_t *strs, uint64_t strs_len, uint32_t max_len, const uint8_t **p) {
  *p = nullptr;
  if (s.len == 0) return true;
  if (s.len > max_len) return false;
  if (s.off == ~0ull) return true;
  if (!strs || s.off > strs_len || s.len > strs_len - s.off) return false;
  *p = strs + s.off;
  return true;
}

// Runs `emit` to size the block and, when there is a buffer that holds it, again to write it.
template <class F>
int build_block(const char *who, uint8_t *out, uint64_t out_cap, uint64_t *len, F emit) {
  Sink count(nullptr);
  emit(count);
  *len = count.n;
  if (!out) {
    if (out_cap) return set_error(GPD_ERR_INVALID, "%s: null out with out_cap %llu", who, (unsigned long long)out_cap);
    return GPD_OK;
  }
  if (count.n > out_cap)
    return set_error(GPD_ERR_INVALID, "%s: the block takes %llu bytes, out_cap is %llu", who,
                     (unsigned long long)count.n, (unsigned long long)out_cap);
  Sink w(out);
  emit(w);
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

}  // namespace
}  // namespace gpd

extern "C" {

int gpd_pcapng_section_block(const gpd_pcapng_section_info *info, const uint8_t *strs, uint64_t strs_len,
                             uint8_t *out, uint64_t out_cap, uint64_t *len) {
  using namespace gpd;
  const char *who = "gpd_pcapng_section_block";
  if (!info || !len) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *len = 0;
  if (info->big_endian)
    return set_error(GPD_ERR_INVALID, "%s: a big-endian section is not written (NgWriter is little-endian only)", who);
  // ngwrite.go:191-210: application, comment, hardware, OS
  const gpd_pcapng_str *s[4] = {&info->application, &info->comment, &info->hardware, &info->os};
  const uint16_t code[4] = {4, 1, 2, 3};
  const uint8_t *p[4];
  for (int k = 0; k < 4; k++)
    if (!str_of(*s[k], strs, strs_len, 65535u, &p[k]))
      return set_error(GPD_ERR_INVALID, "%s: a string lies outside strs or is longer than 65535 bytes", who);
  return build_block(who, out, out_cap, len, [&](Sink &b) {
    uint32_t opts = 0;
    for (int k = 0; k < 4; k++)
      if (s[k]->len) opts += 4u + ((s[k]->len + 3u) & ~3u);
    if (opts) opts += 4;
    const uint32_t total = opts + 24u + 4u;
    b.u32(GPD_PCAPNG_BLOCK_SECTION);
    b.u32(total);
    b.u32(GPD_PCAPNG_BYTE_ORDER);
    b.u16(1);  // ngVersionMajor, ngVersionMinor
    b.u16(0);
    b.u32(0xFFFFFFFFu);  // section length: unspecified
    b.u32(0xFFFFFFFFu);
    for (int k = 0; k < 4; k++)
      if (s[k]->len) b.opt_str(code[k], p[k], s[k]->len);
    if (opts) b.u32(0);  // end of options
    b.u32(total);
  });
}

int gpd_pcapng_interface_block(const gpd_pcapng_iface *intf, const uint8_t *strs, uint64_t strs_len,
                               uint8_t *out, uint64_t out_cap, uint64_t *len) {
  using namespace gpd;
  const char *who = "gpd_pcapng_interface_block";
  if (!intf || !len) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *len = 0;
  // ngwrite.go:243-267: name, comment, description, filter (a zero byte in front), OS
  const gpd_pcapng_str *s[5] = {&intf->name, &intf->comment, &intf->description, &intf->filter, &intf->os};
  const uint16_t code[5] = {2, 1, 3, 11, 12};
  const uint32_t lead[5] = {0, 0, 0, 1, 0};
  const uint8_t *p[5];
  for (int k = 0; k < 5; k++)
    if (!str_of(*s[k], strs, strs_len, 65535u - lead[k], &p[k]))
      return set_error(GPD_ERR_INVALID, "%s: a string lies outside strs or is too long for a 16-bit option length", who);
  return build_block(who, out, out_cap, len, [&](Sink &b) {
    uint32_t opts = 0;
    for (int k = 0; k < 5; k++)
      if (s[k]->len) opts += 4u + ((s[k]->len + lead[k] + 3u) & ~3u);
    if (intf->ts_offset) opts += 12;
    opts += 8 + 4;  // if_tsresol, end of options
    const uint32_t total = opts + 16u + 4u;
    b.u32(GPD_PCAPNG_BLOCK_INTERFACE);
    b.u32(total);
    b.u16((uint16_t)intf->linktype);
    b.u16(0);  // reserved
    b.u32(intf->snaplen);
    for (int k = 0; k < 5; k++)
      if (s[k]->len) b.opt_str(code[k], p[k], s[k]->len, lead[k]);
    if (intf->ts_offset) b.opt_u64(14, intf->ts_offset);
    b.opt_u8(9, 9);  // :273-274: nanoseconds, whatever the interface says
    b.u32(0);        // end of options
    b.u32(total);
  });
}

int gpd_pcapng_stats_block(int64_t intf, uint32_t n_ifaces, const gpd_pcapng_stats *stats,
                           uint8_t *out, uint64_t out_cap, uint64_t *len) {
  using namespace gpd;
  const char *who = "gpd_pcapng_stats_block";
  if (!stats || !len) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *len = 0;
  if (intf < 0 || intf >= (int64_t)n_ifaces)  // ngwrite.go:302-304
    return set_error(GPD_ERR_PCAP, "Can't send statistics for non existent interface %lld; have only %u interfaces",
                     (long long)intf, n_ifaces);
  return build_block(who, out, out_cap, len, [&](Sink &b) {
    const bool dropped = stats->packets_dropped != GPD_PCAPNG_NO_VALUE64;
    const bool received = stats->packets_received != GPD_PCAPNG_NO_VALUE64;
    uint32_t opts = 12u * ((stats->has_start_time != 0) + (stats->has_end_time != 0) + dropped + received);
    if (opts) opts += 4;
    const uint32_t total = opts + 24u;
    const uint64_t ts = stats->has_last_update ? stats->last_update : 0ull;  // :332-335
    b.u32(GPD_PCAPNG_BLOCK_STATS);
    b.u32(total);
    b.u32((uint32_t)intf);
    b.u32((uint32_t)(ts >> 32));
    b.u32((uint32_t)ts);
    if (stats->has_start_time) b.opt_time(2, stats->start_time);
    if (stats->has_end_time) b.opt_time(3, stats->end_time);
    if (dropped) b.opt_u64(5, stats->packets_dropped);
    if (received) b.opt_u64(4, stats->packets_received);
    if (opts) b.u32(0);  // end of options
    b.u32(total);
  });
}

int gpd_pcapng_write(gpd_ctx *ctx, const gpd_batch *in, const uint64_t *ts_ns, const uint32_t *wirelen,
                     const uint32_t *ifindex, uint32_t n_ifaces, const uint8_t *keep,
                     const uint8_t *prefix, uint32_t prefix_len, uint8_t *out, uint64_t out_cap,
                     uint64_t *n_written, uint64_t *bytes, uint64_t *bad_index, uint32_t *bad_reason,
                     void *stream) {
  using namespace gpd;
  const char *who = "gpd_pcapng_write";
  int rc = check_in(who, ctx, in);
  if (rc) return rc;
  if (!n_written || !bytes || !bad_index || !bad_reason)
    return set_error(GPD_ERR_INVALID, "%s: null result pointer", who);
  *n_written = 0;
  *bytes = 0;
  *bad_index = ~0ull;
  *bad_reason = GPD_PCAPNGW_BAD_NONE;
  if (in->n && !ts_ns) return set_error(GPD_ERR_INVALID, "%s: ts_ns is required", who);
  if ((prefix_len & 3u) || prefix_len > GPD_PCAPNGW_MAX_PREFIX || (!prefix && prefix_len))
    return set_error(GPD_ERR_INVALID, "%s: prefix must hold prefix_len bytes, a multiple of 4 and at most %u (got %u)",
                     who, GPD_PCAPNGW_MAX_PREFIX, prefix_len);
  if ((!out && out_cap) || ((uintptr_t)out & 15u))
    return set_error(GPD_ERR_INVALID, "%s: out must be a 16-byte aligned buffer of out_cap bytes", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  NgwArgs A{};
  A.data = in->data;
  A.dlen = (uint32_t)in->data_len;
  A.lim = (in->data_len + 15ull) & ~15ull;
  A.offset = in->offset;
  A.caplen = in->caplen;
  A.n = (uint32_t)in->n;
  A.keep = keep;
  A.ts = ts_ns;
  A.wirelen = wirelen;
  A.ifindex = ifindex;
  A.n_ifaces = n_ifaces;
  A.base0 = prefix_len;
  if (prefix_len & 15u) std::memcpy(A.pt, prefix + (prefix_len & ~15u), prefix_len & 15u);
  A.out = out;
  uint64_t res[5] = {A.base0, 0, ~0ull, 0, 0};
  uint8_t *staged = nullptr;
  if (A.n || (out && A.base0)) {
    rc = scan(ctx, who, A, prefix, out != nullptr, &staged, s, res);
    if (rc) return rc;
  }
  *bytes = res[0];
  *n_written = res[1];
  *bad_index = res[2];
  if (out || out_cap) {
    if (res[0] > out_cap)
      return set_error(GPD_ERR_INVALID, "%s: the stream takes %llu bytes (%llu records), out_cap is %llu", who,
                       (unsigned long long)res[0], (unsigned long long)res[1], (unsigned long long)out_cap);
    if (A.base0) GPD_TRY(hipMemcpyAsync(out, staged, A.base0, hipMemcpyDeviceToDevice, s));
    if (res[1]) {
      hipLaunchKernelGGL(ngw_copy_kernel, dim3((A.nwave + kCopyWaves - 1u) / kCopyWaves), dim3(64 * kCopyWaves),
                         0, s, A);
      GPD_TRY(hipGetLastError());
    }
  }
  if (res[2] != ~0ull) {
    if ((uint32_t)res[4] >= n_ifaces) {  // ngwrite.go:357-359 comes first
      *bad_reason = GPD_PCAPNGW_BAD_IFACE;
      return set_error(GPD_ERR_PCAP, "Can't send statistics for non existent interface %u; have only %u interfaces",
                       (uint32_t)res[4], n_ifaces);
    }
    *bad_reason = GPD_PCAPNGW_BAD_LENGTH;
    return set_error(GPD_ERR_PCAP, "invalid capture info (packet %llu: capture length %u, length %u):  capture length > length",
                     (unsigned long long)res[2], (uint32_t)res[3], (uint32_t)(res[3] >> 32));
  }
  return GPD_OK;
}

}  // extern "C"
