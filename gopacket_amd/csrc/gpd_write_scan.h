// gpd_write_scan.h — the stream compaction over variable-length records the two writers share
// (gpd_pcapwrite.hip: the pcap stream and the batch selection; gpd_pcapngwrite.hip: the pcapng
// stream), one copy for the three record forms.  Packet i takes Form::size(caplen) bytes when it
// is kept and lies before the first kept packet the writer would reject, else 0; the sizes'
// exclusive prefix sum (u64) is where each record goes.  Four launches, none of which waits for
// another workgroup:
//
//   bad_kernel<Form>   the first kept packet that Form::rejects: atomicMin on one device word
//   sum_kernel<Form>   a 1024-thread workgroup per kScanBlock packets: per-wave record sums (as
//                      exclusive prefixes inside the block), kept counts, first kept index; the
//                      block's totals
//   scan_kernel        one workgroup: the block totals' exclusive scans in place, for each block
//                      the first kept packet of any later block, and the five result words the
//                      host reads
//   copy_kernel<Form>  a wave per 64 consecutive packets, whose records are one contiguous run
//                      [P0, P1) of the output.  Lanes walk the run in 16-byte aligned output
//                      chunks; a chunk is put together in registers from the (at most
//                      Form::kMaxRecs) records it overlaps, each found by a 6-step binary search
//                      over the wave's 64 positions in LDS and ORed in by Form::place, and leaves
//                      as one aligned non-temporal 16-byte store.  A wave owns the chunks that
//                      START in its run.  The chunk hanging over P1 is completed with the first
//                      bytes of the next kept record's header: at most 15 (pcap) or 12 (pcapng), so
//                      they never reach its data; that record is found through the first-kept
//                      indices, not by walking.  The chunk hanging into P0 belongs to the wave
//                      before.  Only the stream's last chunk can be partial: Form::store_tail.
//
// Source bytes are read through src16_of (gpd_stream_util.h): no load starts outside [0, lim),
// lim = round_up(data_len, 16), which is all the batch contract promises, and every byte a record
// needs lies inside it.  No byte of `out` at or beyond the stream's length (*bytes) is stored.
//
// What a form supplies is listed at copy_kernel.  Everything here has internal linkage: each of
// the two translation units compiles its own, and links alone with three stubs
// (tests/c/pcapwrite_errpath.cpp, tests/c/pcapngwrite_errpath.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpd_internal.h"
#include "gpd_stream_util.h"

namespace gpd {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kScanBlock = 1024;               // packets per sum_kernel workgroup
constexpr uint32_t kScanWaves = kScanBlock / 64u;   // its waves, one per 64 packets
constexpr uint32_t kCopyWaves = 4;                  // waves per copy_kernel workgroup

// One argument struct for the three forms; a form leaves what it does not use zero (a few unused
// kernel-argument words per launch).  The pcapng-only fields come last, so the fields of the pcap
// forms, whose kernels are the sensitive ones to the order, lie where they always did.
struct WriteArgs {
  const uint8_t *data;
  uint32_t dlen;            // data_len (32-bit, as the decode reads it)
  uint64_t lim;             // round_up(data_len, 16): no load starts at or beyond it
  const uint32_t *offset, *caplen;
  uint32_t n;
  const uint64_t *ts;       // stream forms
  const uint32_t *wirelen;  // stream forms; may be NULL
  const uint8_t *keep;      // may be NULL
  uint32_t scaler;          // pcap: 1000, or 1 (GPD_PCAPW_NANOS)
  uint32_t base0;           // bytes in front of the first record: the file header or the prefix
  uint32_t fh[6];           // pcap: the file header's words; pcapng: [0..2] the prefix's words in the
                            // chunk it ends in
  uint8_t *out;
  uint32_t *o_off, *o_len, *o_idx;  // batch form (o_idx may be NULL)
  // scratch of the context
  uint64_t *res;            // [0] stream bytes, [1] records, [2] bad index, [3] its caplen | Length << 32,
                            // [4] its interface index (0 without an array)
  uint32_t *badw;           // the first rejected kept packet (kNone: none)
  uint64_t *bsum, *wsum;    // per block: record bytes -> exclusive prefix; per wave: prefix inside its block
  uint32_t *bcnt, *wcnt;    // the same for the kept counts
  uint32_t *bfirst, *wfirst;  // first kept packet of the block / wave (kNone: none)
  uint32_t *bnext;          // first kept packet of any later block
  uint32_t nblk, nwave;
  const uint32_t *ifindex;  // pcapng; may be NULL
  uint32_t n_ifaces;        // pcapng
};
using WriteKernel = void (*)(WriteArgs);

// Is packet i written, and where do its bytes lie (clamped to the buffer as the decode does)?
__device__ inline bool kept(const WriteArgs &A, uint32_t i, uint32_t bad, uint32_t &off, uint32_t &len) {
  off = len = 0;
  if (i >= A.n || i >= bad) return false;
  if (A.keep && A.keep[i] == 0) return false;
  off = min(A.offset[i], A.dlen);
  len = min(A.caplen[i], A.dlen - off);
  return true;
}

// The writer's rejections over the kept packets: the lowest index wins.
template <class Form>
__global__ __launch_bounds__(256) void bad_kernel(WriteArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t i = (uint32_t)i64;
  uint32_t off = 0, len = 0;
  const bool k = i64 < A.n && kept(A, i, kNone, off, len);
  const uint64_t m = __ballot(k && Form::rejects(A, i, len));
  if (m != 0ull && lane == 0) atomicMin(A.badw, i - lane + (uint32_t)__builtin_ctzll(m));
}

template <class Form>
__global__ __launch_bounds__(1024) void sum_kernel(WriteArgs A) {
  __shared__ uint64_t s_sum[kScanWaves];
  __shared__ uint32_t s_cnt[kScanWaves], s_first[kScanWaves];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t gw = blockIdx.x * kScanWaves + w;
  const uint64_t i64 = (uint64_t)gw * 64u + lane;
  const uint32_t bad = *A.badw;
  uint32_t off = 0, len = 0;
  const bool k = i64 < A.n && kept(A, (uint32_t)i64, bad, off, len);
  const uint64_t incl = wave_scan64(k ? Form::size(len) : 0ull, lane);
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
    if (Form::kIndexed) A.wcnt[gw] = c;  // (nobody else reads it, and c folds away)
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
// backwards the first kept packet of any later block; last the result words.  The kept counts are
// scanned in 32 bits: check_in bounds n by 2^32 - 256, so their sum fits.
__global__ __launch_bounds__(1024) void scan_kernel(WriteArgs A) {
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
    const uint32_t xc = wave_scan32(vc, lane);
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

struct WriteRec {  // a wave's packet as the chunks see it (LDS, 32 bytes)
  uint64_t pos;    // where its record starts in the output
  uint32_t off, len;
  uint32_t f[4];   // the form's own words (Form::fields)
};

// A form is a struct of static members:
//   size(len)                 the record's bytes
//   rejects(A, i, len)        bad_kernel's test of kept packet i (stream forms)
//   fields(A, i, len, f)      the form's 16 bytes of packet i's LDS record
//   kIndexed                  kept records get per-record output indices (o_off, o_len, o_idx)
//   kRunEndsInChunk           a run can end inside a chunk; where it cannot, none of next_head,
//                             span and store_tail is needed and the code for them is not compiled
//   next_head(A, nx, nlen)    the first header words of kept packet nx, the record after the run
//   span(lo, hi, s)           bytes [s, s + 16) of lo:hi at the form's granularity
//   first_chunk(P0)           the chunk at which the run that starts the records begins
//   kLeads, lead(A, cb, ce, P0, V)   that run's chunks can start in front of P0: what lies there
//                             goes into V, and the position up to which the chunk is then filled
//                             is returned (kept a branch: as selects it would run for every chunk)
//   kMaxRecs                  records a chunk can overlap
//   place(A, q, d, V)         ORs record q's share into the chunk that starts at byte d of the
//                             record (d < 0: the record starts inside the chunk); returns the
//                             record's end in the output
//   store_tail(p, V, vend)    the stream's ragged last chunk: bytes [0, vend) of V to p
template <class Form>
__global__ __launch_bounds__(64 * kCopyWaves) void copy_kernel(WriteArgs A) {
  __shared__ WriteRec s_rec[kCopyWaves][64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t gw = blockIdx.x * kCopyWaves + w;
  const bool live = gw < A.nwave;
  const uint32_t blk = gw / kScanWaves;
  const uint64_t i64 = (uint64_t)gw * 64u + lane;
  const uint32_t i = (uint32_t)i64;
  const uint32_t bad = *A.badw;
  uint32_t off = 0, len = 0;
  const bool k = live && i64 < A.n && kept(A, i, bad, off, len);
  const uint64_t km = Form::kIndexed ? __ballot(k) : 0ull;
  const uint64_t sz = k ? Form::size(len) : 0ull;
  const uint64_t incl = wave_scan64(sz, lane);
  const uint64_t total = shfl64(incl, 63);
  const uint64_t P0 = live ? (uint64_t)A.base0 + A.bsum[blk] + A.wsum[gw] : 0ull;
  const uint64_t P1 = P0 + total;
  WriteRec r;
  r.pos = P0 + incl - sz;
  r.off = off;
  r.len = len;
  r.f[0] = r.f[1] = r.f[2] = r.f[3] = 0;
  if (k) {
    Form::fields(A, i, len, r.f);
    if (Form::kIndexed) {
      const uint32_t j = A.bcnt[blk] + A.wcnt[gw] + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
      A.o_off[j] = (uint32_t)r.pos;
      A.o_len[j] = len;
      if (A.o_idx) A.o_idx[j] = i;
    }
  }
  s_rec[w][lane] = r;
  __syncthreads();
  if (total == 0ull) return;  // nothing of this wave's is kept
  const WriteRec *rec = s_rec[w];

  // The header of the kept record that follows the run: its first bytes complete the last chunk.
  v4u Hn{0u, 0u, 0u, 0u};
  bool has_next = false;
  if constexpr (Form::kRunEndsInChunk) {
    if (P1 & 15ull) {
      const uint32_t g = blk * kScanWaves + lane;
      uint32_t nx = (lane < kScanWaves && g > gw && g < A.nwave) ? A.wfirst[g] : kNone;
      nx = wave_min32(nx);
      if (nx == kNone) nx = A.bnext[blk];
      if (nx != kNone) {
        uint32_t noff, nlen;
        (void)kept(A, nx, bad, noff, nlen);
        Hn = Form::next_head(A, nx, nlen);
        has_next = true;
      }
    }
  }

  // The run that starts the records also owns what lies in front of them in their first chunk.
  const bool first = P0 == (uint64_t)A.base0;
  const uint64_t c_lo = first ? Form::first_chunk(P0) : (P0 + 15ull) >> 4, c_hi = (P1 + 15ull) >> 4;
  const uint64_t nch = c_hi - c_lo;
  const v4u z{0u, 0u, 0u, 0u};
  for (uint64_t it = 0; it * 64ull < nch; ++it) {
    const uint64_t c = c_lo + it * 64ull + lane;
    if (c >= c_hi) break;  // (the last round's upper lanes)
    const uint64_t cb = c << 4, ce = cb + 16ull;
    v4u V = z;
    uint64_t x = cb;
    if constexpr (Form::kLeads) {
      if (__builtin_expect(cb < P0, 0)) x = Form::lead(A, cb, ce, P0, V);  // (first run only)
    }
#pragma unroll
    for (uint32_t rnd = 0; rnd < Form::kMaxRecs; ++rnd) {
      if (x >= (ce < P1 ? ce : P1)) break;
      uint32_t lo = 0;  // the last packet with pos <= x: the record x lies in
#pragma unroll
      for (uint32_t step = 32; step >= 1u; step >>= 1)
        if (rec[lo + step].pos <= x) lo += step;
      const WriteRec q = rec[lo];
      x = Form::place(A, q, (int64_t)(cb - q.pos), V);
    }
    uint32_t vend = 16;
    if constexpr (Form::kRunEndsInChunk) {
      if (x < ce) {  // x == P1
        if (has_next) V |= Form::span(z, Hn, (uint32_t)(ce - x));
        else vend = (uint32_t)(x - cb);
      }
    }
    if (vend == 16u) {
      __builtin_nontemporal_store(V, reinterpret_cast<v4u *>(A.out + cb));
    } else if constexpr (Form::kRunEndsInChunk) {
      Form::store_tail(A.out + cb, V, vend);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
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

void fill_in(WriteArgs &A, const gpd_batch *in, const uint8_t *keep) {
  A.data = in->data;
  A.dlen = (uint32_t)in->data_len;
  A.lim = (in->data_len + 15ull) & ~15ull;
  A.offset = in->offset;
  A.caplen = in->caplen;
  A.n = (uint32_t)in->n;
  A.keep = keep;
}

// The context's scratch (slot 11) carved into A's arrays, with `tail` more bytes behind them at
// *tail_dev (16-aligned) into which `tail_src` (host) is copied; with packets, the scan (`bad`
// may be NULL: no rejection to look for) and res[5] back on the host.  Synchronises `s` when it
// queued anything, after which `tail_src` is free.
int carve_and_scan(gpd_ctx *ctx, const char *who, WriteArgs &A, WriteKernel bad, WriteKernel sum,
                   const uint8_t *tail_src, size_t tail, uint8_t **tail_dev, hipStream_t s, uint64_t res[5]) {
  A.nblk = (A.n + kScanBlock - 1u) / kScanBlock;
  A.nwave = (uint32_t)(((uint64_t)A.n + 63u) / 64u);
  const size_t arrays = up16((size_t)A.nblk * (8 + 3 * 4) + (size_t)A.nwave * (8 + 2 * 4));
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 11, 64 + arrays + tail + 64));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.res = reinterpret_cast<uint64_t *>(base);
  A.badw = reinterpret_cast<uint32_t *>(base + 48);
  A.bsum = reinterpret_cast<uint64_t *>(base + 64);
  A.wsum = A.bsum + A.nblk;
  A.bcnt = reinterpret_cast<uint32_t *>(A.wsum + A.nwave);
  A.bfirst = A.bcnt + A.nblk;
  A.bnext = A.bfirst + A.nblk;
  A.wcnt = A.bnext + A.nblk;
  A.wfirst = A.wcnt + A.nwave;
  if (tail_dev) *tail_dev = base + 64 + arrays;
  if (tail) GPD_TRY(hipMemcpyAsync(base + 64 + arrays, tail_src, tail, hipMemcpyHostToDevice, s));
  if (A.n) {
    GPD_TRY(hipMemsetAsync(base, 0xFF, 64, s));
    if (bad) hipLaunchKernelGGL(bad, dim3((A.n + 255u) / 256u), dim3(256), 0, s, A);
    hipLaunchKernelGGL(sum, dim3(A.nblk), dim3(1024), 0, s, A);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, A);
    GPD_TRY(hipGetLastError());
    GPD_TRY(hipMemcpyAsync(res, A.res, 40, hipMemcpyDeviceToHost, s));
  }
  if (A.n || tail) GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}

// The stream forms' capacity check (res as carve_and_scan left it).
int check_stream_cap(const char *who, const uint64_t res[5], uint64_t out_cap) {
  if (res[0] > out_cap)
    return set_error(GPD_ERR_INVALID, "%s: the stream takes %llu bytes (%llu records), out_cap is %llu", who,
                     (unsigned long long)res[0], (unsigned long long)res[1], (unsigned long long)out_cap);
  return GPD_OK;
}

}  // namespace
}  // namespace gpd
