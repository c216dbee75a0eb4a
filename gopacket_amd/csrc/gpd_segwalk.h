// gpd_segwalk.h — the segmented walk of a capture chunk in HBM, once, for the formats whose
// records chain by a length field (gpd_pcapwalk.hip: pcap records, gpd_ngwalk.hip: pcapng
// blocks).  Device code only; the two .hip files include it and wrap the bodies in kernels.
//
//   seg_walk_body    one lane per kPwSeg bytes of the chunk.  The segment holding the chunk's
//                    entry (the first header, handed on by the previous chunk) walks from it;
//                    every later segment starts speculatively at F::speculate's choice, if any,
//                    and walks while headers start inside the segment: start, exit (the first
//                    header at or past the segment's end, or the one that stopped it), packet
//                    count, and the stop kind (0: none);
//   seg_stitch_body  one workgroup: the true walk runs through the segments exactly when every
//                    segment that found a start begins where the previous such segment's walk
//                    left off, and every segment that found none is jumped by it.  A segment the
//                    true walk enters elsewhere is walked again from there, for up to
//                    F::kFixRounds rounds.  The first segment on the true walk that stopped ends
//                    it.  Then the counts' prefix sums are the packets' indices, the last exit is
//                    where the next chunk's walk starts, and the chunk's packet count goes to the
//                    control block (for the decode launch and the host);
//   seg_fill_body    one lane per segment again: its packets' data offsets (relative to the
//                    chunk) and capture lengths, at their indices.
//
// A format F supplies
//   Args                      SegArgs plus what its steps need
//   step(A, p, off, cap, next)  the record or block at p: 0 skipped and 1 a packet (off, cap),
//                             both setting `next`; or a stop kind — the PwCtl::status bit it
//                             sets — for a header the device does not take
//   emit(A, p, off, cap, next)  step's answer at a header the walk took, by the cheapest means
//   speculate(A, lo, hi)      the header a segment not holding the entry starts at, or kNone
//   kFixRounds                rounds of re-walks before the chunk is the host's
//   kStopKeeps                a stop on the true walk keeps the packets before it (status = the
//                             stop kind, `n` those packets, `next` the stopping header) or hands
//                             the whole chunk to the host (status = 1 | the stop kind, n = 0)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpd_internal.h"

namespace gpd {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t rd32(const uint8_t *p, bool be) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  return be ? __builtin_bswap32(v) : v;
}

// Walk segment s from `at` while headers start before hi.  `at` at or past hi: no header starts
// in the segment (a longer record covers the whole of it, or its scan found no start).
template <class F>
__device__ __forceinline__ void seg_walk_from(const typename F::Args &A, uint32_t s, uint32_t at, uint32_t hi) {
  if (at >= hi) {
    A.st[s] = kNone;
    A.ct[s] = 0;
    A.bad[s] = 0;
    return;
  }
  uint32_t p = at, cnt = 0, bad = 0;
  while (p < hi) {
    uint32_t off, cap, next;
    const int k = F::step(A, p, off, cap, next);
    if (k >= 2) {
      bad = (uint32_t)k;
      break;
    }
    cnt += (uint32_t)k;
    p = next;
  }
  A.st[s] = at;
  A.ex[s] = p;
  A.ct[s] = cnt;
  A.bad[s] = bad;
}

template <class F>
__device__ __forceinline__ void seg_walk_body(const typename F::Args &A) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= A.nseg) return;
  const uint32_t lo = s * kPwSeg, hi = min(lo + kPwSeg, A.own_end);
  const uint32_t e = A.ctl->entry;
  uint32_t start = kNone;
  if (e >= lo && e < hi)
    start = e;
  else if (e < lo)
    start = F::speculate(A, lo, hi);
  seg_walk_from<F>(A, s, start, hi);
}

// One workgroup of 1024 lanes; lane t owns segments [t*R, t*R + R).  Where the true walk
// disagrees with a segment's speculation (it enters the segment elsewhere, or enters one whose
// scan found no start), the owning lane re-walks that segment from where the true walk stands,
// and the check runs again (a fix can move where the next lane's first segment is entered): up
// to F::kFixRounds rounds, after which the chunk is the host's.  A segment on the true walk that
// stopped ends the walk: the segments behind it are neither checked nor counted.
template <class F>
__device__ __forceinline__ void seg_stitch_body(const typename F::Args &A) {
  __shared__ uint32_t s_cnt[1024], s_last[1024], s_stop[1024], s_why, s_fixed, s_nfix;
  __shared__ unsigned long long s_miss;  // the first refuted segment << 32 | its speculated start
  const uint32_t t = threadIdx.x;
  const uint32_t R = (A.nseg + 1023u) / 1024u;
  const uint32_t a = min(t * R, A.nseg), b = min(a + R, A.nseg);
  const uint32_t e = A.ctl->entry;
  if (t == 0) {
    s_miss = ~0ull;
    s_nfix = 0;
    s_why = 0;
  }
  uint32_t why = 0;  // the host's reasons for the whole chunk (PwCtl::status bits)
  for (int round = 0;; round++) {
    // this lane's last segment with a start, the first of them that stopped, and the packets up
    // to that one (every segment's words are loaded whatever they hold: the loads of several
    // segments are in flight together, where a load behind a branch would wait for the one before)
    uint32_t cnt = 0, last = kNone, stop = kNone;
#pragma unroll 4
    for (uint32_t s = a; s < b; s++) {
      const uint32_t st = A.st[s], ct = A.ct[s], bad = A.bad[s];
      const bool counts = st != kNone && stop == kNone;
      if (st != kNone) last = s;
      if (counts) cnt += ct;
      if (counts && bad != 0u) stop = s;
    }
    s_cnt[t] = cnt;
    s_last[t] = last;
    s_stop[t] = stop;
    if (t == 0) s_fixed = 0;
    __syncthreads();
    // inclusive scans across lanes (Hillis-Steele; 1024 entries): + of counts, max of last
    // (kNone = none), min of stop (kNone = none)
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
      const uint32_t c = t >= d ? s_cnt[t - d] : 0u;
      const uint32_t l = t >= d ? s_last[t - d] : kNone;
      const uint32_t p = t >= d ? s_stop[t - d] : kNone;
      __syncthreads();
      s_cnt[t] += c;
      if (l != kNone && (s_last[t] == kNone || l > s_last[t])) s_last[t] = l;
      if (p < s_stop[t]) s_stop[t] = p;
      __syncthreads();
    }
    uint32_t base = t ? s_cnt[t - 1] : 0u;      // the index of this lane's first packet
    uint32_t prev = t ? s_last[t - 1] : kNone;  // the last segment with a start before a
    bool stopped = t ? s_stop[t - 1] != kNone : false;  // the walk ended before this lane's segments
    uint32_t fixed = 0;
    why = 0;
    for (uint32_t s = a; s < b && !stopped; s++) {
      const uint32_t lo = s * kPwSeg, hi = min(lo + kPwSeg, A.own_end);
      // where the true walk stands when it reaches this segment
      const uint32_t at = prev == kNone ? e : A.ex[prev];
      uint32_t st = A.st[s], ct = A.ct[s], bad = A.bad[s];
      const bool refuted = st != kNone && st != at;             // a speculation the true walk misses
      const bool uncovered = st == kNone && at >= lo && at < hi;  // a header of the true walk, unwalked
      if (refuted || uncovered) {
        if (round < F::kFixRounds) {
          if (refuted) atomicMin(&s_miss, ((unsigned long long)s << 32) | st);
          // (`at` below the segment: an earlier lane is fixing a segment of its own in this
          // round, and the next round sees where the walk really enters this one)
          if (at >= lo) {
            seg_walk_from<F>(A, s, at, hi);
            st = A.st[s], ct = A.ct[s], bad = A.bad[s];
          }
          fixed++;
        } else {
          why |= refuted ? 2u : 8u;
        }
      }
      if (st != kNone) {
        A.base[s] = base;
        base += ct;
        prev = s;
        stopped = bad != 0u;
      }
    }
    if (fixed) {
      s_fixed = 1u;
      atomicAdd(&s_nfix, fixed);
    }
    __threadfence_block();  // (the re-walked segments' words, for the other lanes' next round)
    __syncthreads();
    const bool again = s_fixed != 0u;
    __syncthreads();
    if (!again) break;
  }
  // (the last round changed nothing: its scans and the indices it wrote describe the final
  // walk; a round that re-walked a segment worked with counts that the next one replaces)
  if (why) atomicOr(&s_why, why);
  __syncthreads();
  if (t == 1023u) {
    const uint32_t cut = s_stop[1023];  // the first segment on the true walk that stopped
    const uint32_t total = s_cnt[cut == kNone ? 1023u : cut / R];  // (its lane counted up to it)
    const uint32_t lastseg = cut != kNone ? cut : s_last[1023];
    const uint32_t next = lastseg == kNone ? e : A.ex[lastseg];
    const uint32_t stop = cut == kNone ? 0u : A.bad[cut];
    // without a stop the walk must leave the chunk (or end exactly at the capture's end): a
    // capture that does not end exactly after a record is the host's to walk
    const bool done = stop != 0u || (A.last ? next == A.T : next >= A.own_end);
    const uint32_t why_all = s_why | (done ? 0u : 16u) | (F::kStopKeeps ? 0u : stop);
    const bool good = why_all == 0u;
    A.ctl->miss_st = s_miss == ~0ull ? kNone : (uint32_t)s_miss;
    A.ctl->miss_at = s_miss == ~0ull ? kNone : (uint32_t)(s_miss >> 32);
    A.ctl->pad[0] = s_nfix;  // segments re-walked here
    A.ctl->pad[1] = cut;     // the fill writes the segments up to it
    A.ctl->n = good ? total : 0u;
    A.ctl->next = next;
    A.ctl->status = good ? stop : 1u | why_all;
    if (good && stop == 0u && A.ctl_next) A.ctl_next->entry = next - A.own_end;
  }
}

template <class F>
__device__ __forceinline__ void seg_fill_body(const typename F::Args &A) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= A.nseg || (A.ctl->status & 1u)) return;
  const uint32_t cut = A.ctl->pad[1];
  if (cut != kNone && s > cut) return;
  const uint32_t start = A.st[s];
  if (start == kNone) return;
  const uint32_t k = A.base[s], c = A.ct[s];
  uint32_t p = start, j = 0;
  while (j < c) {  // (the walk counted c packets from here: every step before them is 0 or 1)
    uint32_t off, cap, next;
    const int kind = F::emit(A, p, off, cap, next);
    if (kind >= 2) break;
    if (kind == 1) {
      A.off[k + j] = off;
      A.len[k + j] = cap;
      j++;
    }
    p = next;
  }
}

}  // namespace

}  // namespace gpd
