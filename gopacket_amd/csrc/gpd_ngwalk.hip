// gpd_ngwalk.hip — the pcapng block walk on the GPU, for gpd_decode_pcapng (include/gpd_pcapng.h).
//
// As in gpd_pcapwalk.hip the capture's bytes travel to HBM in fixed byte chunks and the packets
// are found there, so the host never reads a block header of the bulk of a capture.  A pcapng
// stream differs from pcap in that blocks change the reader's state (a section header switches
// the byte order and clears the interfaces, an interface description adds one, a statistics
// block can stop the reader), so the device walks between such blocks only.  The host
// (gpd_runtime.cpp) hands each chunk the reader's state — the section's byte order, which
// interfaces exist and which of them keep their packets, interface 0's snap length — and
//
//   ng_walk    one lane per 2 KiB segment of the chunk.  The segment holding the chunk's entry
//              walks from it; every later segment starts speculatively at its first 4-byte
//              aligned position whose chain of 4 blocks looks like pcapng (below), and walks while
//              block headers start inside the segment: start, exit, packet count, and whether it
//              stopped at a state-changing block (2) or at a block the device does not vouch
//              for (1);
//   ng_stitch  one workgroup: follows the true walk through the segments as pw_stitch does,
//              re-walking a segment whose speculation the true walk misses (up to kFixRounds
//              rounds, then the chunk is the host's: status 1).  The first segment on the true
//              walk that stopped ends the device's part of the chunk: `n` counts the packets
//              before that block, `next` is its position and status says which kind it was
//              (kNgTailState / kNgTailBlock) — the host reads on from there with the sequential
//              reader (gpd_pcapng.cpp) and hands back to the device behind it.  dumpcap ends every
//              file with a statistics block: its last chunk keeps all its packets this way;
//   ng_fill    one lane per segment up to that cut: its packets' data offsets (relative to the
//              chunk) and capture lengths at their final indices.
//
// The decode kernel reads the packet count from the control block (KParams::n_dev).
//
// The true walk takes a block only when the sequential reader (pcapgo/ngread.go:443-545) would
// take it the same way without any error, wrap or EOF: total length a multiple of 4, >= 12 and
// inside the bytes held; enhanced (6) and obsolete (2) packet blocks with the interface in
// range and caplen <= total - 32, simple (3) ones with an interface present and the clipped
// caplen <= total - 16; packets of an interface with another link type are skipped uncounted
// (the host's with ErrorOnMismatchingLinkType); any other type is skipped by its length.
// Everything else is the host's, which stops or goes on exactly as the reference does.
//
// Speculation may use evidence the reader ignores, since a wrong or missing guess only costs a
// re-walk: 4-byte alignment in the file, a known type at the head of the chain, the trailing
// total length equal to the leading one, interface ids in range.  False chains considered:
//   - the view 4 bytes into a block reads the total length as a type: >= 12, so never a known one;
//   - zero-filled payload reads as type 0 / length 0: rejected by the length;
//   - payload dwords {6, L} need the dword at +L-4 to equal L, four times in a row;
//   - a packet whose payload is itself a pcapng stream (packet data starts 4-byte aligned, so
//     the inner blocks are aligned and pass every test): a segment that begins inside it picks
//     the inner chain, which the true walk never meets — the stitch re-walks that segment from
//     where the true walk enters it (tests/test_pcapng_gpu.py case 8);
//   - a capture whose blocks are not 4-byte aligned in the file is never found by speculation:
//     every segment is re-walked, and past kFixRounds rounds the host walks the chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpd_internal.h"
#include "../../include/gpd_pcapng.h"

namespace gpd {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kChain = 4;
// A re-walk moves the true walk on by one lane's segments per round (a lane fixes its own
// segments in order; the next lane sees the result in the next round), so a run of refuted
// segments takes as many rounds as it spans lanes: nested captures refute every segment they
// cover.  64 rounds of a few microseconds each bound what an adversarial chunk can cost.
constexpr int kFixRounds = 64;

__device__ __forceinline__ uint32_t rd32(const uint8_t *p, bool be) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  return be ? __builtin_bswap32(v) : v;
}
__device__ __forceinline__ uint32_t rd16(const uint8_t *p, bool be) {
  return be ? ((uint32_t)p[0] << 8) | p[1] : ((uint32_t)p[1] << 8) | p[0];
}

__device__ __forceinline__ bool ng_state_type(uint32_t type) {
  return type == GPD_PCAPNG_BLOCK_SECTION || type == GPD_PCAPNG_BLOCK_INTERFACE || type == GPD_PCAPNG_BLOCK_STATS;
}

// One block of the true walk at p: 0 a block skipped, 1 a packet (off, cap), 2 a state-changing
// block, 3 a block the device does not vouch for.  0 and 1 set `next`.
__device__ __forceinline__ int ng_step(const NgArgs &A, uint32_t p, uint32_t &off, uint32_t &cap, uint32_t &next) {
  if ((uint64_t)p + 12u > A.T) return 3;
  const uint8_t *h = A.d + p;
  const uint32_t type = rd32(h, A.be), total = rd32(h + 4, A.be);
  if (ng_state_type(type)) return 2;
  if (total < 12u || (total & 3u) || (uint64_t)p + total > A.T) return 3;
  next = p + total;
  if (type == GPD_PCAPNG_BLOCK_ENHANCED || type == GPD_PCAPNG_BLOCK_PACKET) {
    if (total < 32u) return 3;
    const uint32_t idx = type == GPD_PCAPNG_BLOCK_ENHANCED ? rd32(h + 8, A.be) : rd16(h + 8, A.be);
    if (idx >= A.nif) return 3;
    cap = rd32(h + 20, A.be);
    if (cap > total - 32u) return 3;
    off = p + 28u;
    if (!((A.keep >> idx) & 1u)) return A.drop_is_error ? 3 : 0;
    return 1;
  }
  if (type == GPD_PCAPNG_BLOCK_SIMPLE) {
    if (total < 16u || A.nif == 0u) return 3;
    const uint32_t wire = rd32(h + 8, A.be);
    cap = A.snaplen0 != 0u && wire > A.snaplen0 ? A.snaplen0 : wire;
    if (cap > total - 16u) return 3;
    off = p + 12u;
    if (!(A.keep & 1u)) return A.drop_is_error ? 3 : 0;
    return 1;
  }
  return 0;
}

// A block at x (4-byte aligned) that heads a chain of kChain blocks with matching leading and
// trailing lengths (or reaches a state-changing block, or the end of the bytes held, after at
// least one).
__device__ __forceinline__ bool ng_plausible(const NgArgs &A, uint32_t x) {
  for (int k = 0; k < kChain; k++) {
    if ((uint64_t)x + 12u > A.T) return k > 0 && (A.last ? x == A.T : true);
    const uint8_t *h = A.d + x;
    const uint32_t type = rd32(h, A.be), total = rd32(h + 4, A.be);
    if (k > 0 && ng_state_type(type)) return true;
    if (total < 12u || (total & 3u)) return false;
    if ((uint64_t)x + total > A.T) return k > 0 && !A.last;
    if (rd32(h + total - 4u, A.be) != total) return false;
    if (type == GPD_PCAPNG_BLOCK_ENHANCED || type == GPD_PCAPNG_BLOCK_PACKET) {
      if (total < 32u || rd32(h + 20, A.be) > total - 32u) return false;
      if ((type == GPD_PCAPNG_BLOCK_ENHANCED ? rd32(h + 8, A.be) : rd16(h + 8, A.be)) >= A.nif) return false;
    } else if (type == GPD_PCAPNG_BLOCK_SIMPLE) {
      if (total < 16u) return false;
    } else if (k == 0 && !ng_state_type(type)) {
      return false;  // the chain's head has a known type
    }
    x += total;
  }
  return true;
}

// Walk segment s from `at` while block headers start before hi.
__device__ __forceinline__ void ng_walk_from(const NgArgs &A, uint32_t s, uint32_t at, uint32_t hi) {
  uint32_t p = at, cnt = 0, bad = 0;
  while (p < hi) {
    uint32_t off, cap, next;
    const int k = ng_step(A, p, off, cap, next);
    if (k >= 2) {
      bad = k == 2 ? 2u : 1u;
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

}  // namespace

__global__ __launch_bounds__(256) void ng_walk(NgArgs A) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= A.nseg) return;
  const uint32_t lo = s * kPwSeg, hi = min(lo + kPwSeg, A.own_end);
  const uint32_t e = A.ctl->entry;
  uint32_t start = kNone;
  if (e >= lo && e < hi) {
    start = e;
  } else if (e < lo) {  // speculation: the first plausible chain head of the segment
    for (uint32_t x = lo; x < hi && (uint64_t)x + 12u <= A.T; x += 4u) {
      uint32_t type = *reinterpret_cast<const uint32_t *>(A.d + x);
      if (A.be) type = __builtin_bswap32(type);
      if (type == 0u || (type > 6u && type != GPD_PCAPNG_BLOCK_SECTION) || type == 4u) continue;
      if (ng_plausible(A, x)) {
        start = x;
        break;
      }
    }
  }
  if (start == kNone) {
    A.st[s] = kNone;
    A.ex[s] = 0;
    A.ct[s] = 0;
    A.bad[s] = 0;
    return;
  }
  ng_walk_from(A, s, start, hi);
}

// One workgroup of 1024 lanes; lane t owns segments [t*R, t*R + R).  As pw_stitch, with one
// addition: a segment on the true walk that stopped (bad != 0) ends the walk, and the segments
// behind it are neither checked nor counted.
__global__ __launch_bounds__(1024) void ng_stitch(NgArgs A) {
  __shared__ uint32_t s_cnt[1024], s_last[1024], s_stop[1024], s_why[1024], s_fixed, s_nfix;
  const uint32_t t = threadIdx.x;
  const uint32_t R = (A.nseg + 1023u) / 1024u;
  const uint32_t a = min(t * R, A.nseg), b = min(a + R, A.nseg);
  const uint32_t e = A.ctl->entry;
  if (t == 0) s_nfix = 0;
  uint32_t why = 0;  // the host's reasons for the whole chunk (PwCtl::status bits)
  for (int round = 0;; round++) {
    uint32_t last = kNone, stop = kNone;  // this lane's last segment with a start; first one that stopped
    for (uint32_t s = a; s < b; s++) {
      if (A.st[s] != kNone) {
        last = s;
        if (stop == kNone && A.bad[s] != 0u) stop = s;
      }
    }
    s_last[t] = last;
    s_stop[t] = stop;
    if (t == 0) s_fixed = 0;
    __syncthreads();
    // inclusive scans across lanes: max of last (kNone = none), min of stop (kNone = none)
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
      const uint32_t l = t >= d ? s_last[t - d] : kNone;
      const uint32_t p = t >= d ? s_stop[t - d] : kNone;
      __syncthreads();
      if (l != kNone && (s_last[t] == kNone || l > s_last[t])) s_last[t] = l;
      if (p < s_stop[t]) s_stop[t] = p;
      __syncthreads();
    }
    uint32_t prev = t ? s_last[t - 1] : kNone;  // the last segment with a start before a
    bool stopped = t ? s_stop[t - 1] != kNone : false;  // the walk ended before this lane's segments
    uint32_t fixed = 0;
    why = 0;
    for (uint32_t s = a; s < b && !stopped; s++) {
      const uint32_t lo = s * kPwSeg, hi = min(lo + kPwSeg, A.own_end);
      const uint32_t at = prev == kNone ? e : A.ex[prev];  // where the true walk stands
      uint32_t st = A.st[s];
      const bool refuted = st != kNone && st != at;
      const bool uncovered = st == kNone && at >= lo && at < hi;
      if (refuted || uncovered) {
        if (round < kFixRounds) {
          // (`at` below the segment: an earlier lane is fixing a segment of its own in this
          // round, and the next round sees where the walk really enters this one)
          if (at >= lo) {
            if (at >= hi) {  // a longer block covers the whole segment: no header starts in it
              A.st[s] = kNone;
              A.ct[s] = 0;
              A.bad[s] = 0;
            } else {
              ng_walk_from(A, s, at, hi);
            }
            st = A.st[s];
          }
          fixed++;
        } else {
          why |= refuted ? 2u : 8u;
        }
      }
      if (st != kNone) {
        prev = s;
        stopped = A.bad[s] != 0u;
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
  // (the last round changed nothing: its scans describe the final walk)
  const uint32_t cut = s_stop[1023];  // the first segment on the true walk that stopped
  uint32_t cnt = 0;
  for (uint32_t s = a; s < b; s++)
    if (A.st[s] != kNone && (cut == kNone || s <= cut)) cnt += A.ct[s];
  s_cnt[t] = cnt;
  s_why[t] = why;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const uint32_t c = t >= d ? s_cnt[t - d] : 0u;
    const uint32_t w = t >= d ? s_why[t - d] : 0u;
    __syncthreads();
    s_cnt[t] += c;
    s_why[t] |= w;
    __syncthreads();
  }
  uint32_t base = t ? s_cnt[t - 1] : 0u;
  for (uint32_t s = a; s < b; s++)
    if (A.st[s] != kNone && (cut == kNone || s <= cut)) {
      A.base[s] = base;
      base += A.ct[s];
    }
  if (t == 1023u) {
    const uint32_t total = s_cnt[1023];
    const uint32_t lastseg = cut != kNone ? cut : s_last[1023];
    const uint32_t next = lastseg == kNone ? e : A.ex[lastseg];
    const uint32_t tail = cut == kNone ? 0u : A.bad[cut] == 2u ? kNgTailState : kNgTailBlock;
    // without a stop the walk must leave the chunk (or end exactly at the capture's end)
    const bool done = tail != 0u || (A.last ? next == A.T : next >= A.own_end);
    const uint32_t why_all = s_why[1023] | (done ? 0u : 16u);
    const bool good = why_all == 0u;
    A.ctl->miss_st = kNone;
    A.ctl->miss_at = kNone;
    A.ctl->pad[0] = s_nfix;  // segments re-walked here
    A.ctl->pad[1] = cut;     // ng_fill writes the segments up to it
    A.ctl->n = good ? total : 0u;
    A.ctl->next = next;
    A.ctl->status = good ? tail : 1u | why_all;
    if (good && tail == 0u && A.ctl_next) A.ctl_next->entry = next - A.own_end;
  }
}

__global__ __launch_bounds__(256) void ng_fill(NgArgs A) {
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
    const int kind = ng_step(A, p, off, cap, next);
    if (kind >= 2) break;
    if (kind == 1) {
      A.off[k + j] = off;
      A.len[k + j] = cap;
      j++;
    }
    p = next;
  }
}

hipError_t launch_ng_walk(const NgArgs &A, hipStream_t stream) {
  const unsigned g = (A.nseg + 255u) / 256u;
  if (A.nseg > kPwMaxSeg || A.nif > kNgMaxIfaces) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ng_walk, dim3(g ? g : 1), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(ng_stitch, dim3(1), dim3(1024), 0, stream, A);
  return hipGetLastError();
}

hipError_t launch_ng_fill(const NgArgs &A, hipStream_t stream) {
  const unsigned g = (A.nseg + 255u) / 256u;
  hipLaunchKernelGGL(ng_fill, dim3(g ? g : 1), dim3(256), 0, stream, A);
  return hipGetLastError();
}

}  // namespace gpd
