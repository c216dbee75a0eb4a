// gpd_ngwalk.hip — the pcapng block walk on the GPU, for gpd_decode_pcapng (include/gpd_pcapng.h).
//
// The capture's bytes travel to HBM in fixed byte chunks and the packets are found there by the
// segmented walk of gpd_segwalk.h (ng_walk, ng_stitch, ng_fill), so the host never reads a block
// header of the bulk of a capture.  A pcapng stream differs from pcap in that blocks change the
// reader's state (a section header switches the byte order and clears the interfaces, an
// interface description adds one, a statistics block can stop the reader), so the device walks
// between such blocks only.  The host (gpd_capture.cpp) hands each chunk the reader's state —
// the section's byte order, which interfaces exist and which of them keep their packets,
// interface 0's snap length — and pcapng's rules are:
//
//   step       below ("the true walk takes a block only when ..."); a state-changing block and
//              a block the device does not vouch for are the two stop kinds;
//   speculate  a segment's first 4-byte aligned position whose chain of 4 blocks looks like
//              pcapng (below);
//   a stop     on the true walk ends the device's part of the chunk and keeps what precedes it:
//              `n` counts the packets before that block, `next` is its position and status says
//              which kind it was (kNgTailState / kNgTailBlock) — the host reads on from there
//              with the sequential reader (gpd_pcapng.cpp) and hands back to the device behind
//              it.  dumpcap ends every file with a statistics block: its last chunk keeps all
//              its packets this way.  Only speculation the true walk still misses after
//              kFixRounds rounds makes the chunk the host's (status 1).
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
#include "gpd_segwalk.h"
#include "../../include/gpd_pcapng.h"

namespace gpd {

namespace {

constexpr int kChain = 4;

__device__ __forceinline__ uint32_t rd16(const uint8_t *p, bool be) {
  return be ? ((uint32_t)p[0] << 8) | p[1] : ((uint32_t)p[1] << 8) | p[0];
}

__device__ __forceinline__ bool ng_state_type(uint32_t type) {
  return type == GPD_PCAPNG_BLOCK_SECTION || type == GPD_PCAPNG_BLOCK_INTERFACE || type == GPD_PCAPNG_BLOCK_STATS;
}

// One block of the true walk at p: 0 a block skipped, 1 a packet (off, cap), kNgTailState a
// state-changing block, kNgTailBlock a block the device does not vouch for.  0 and 1 set `next`.
__device__ __forceinline__ int ng_step(const NgArgs &A, uint32_t p, uint32_t &off, uint32_t &cap, uint32_t &next) {
  if ((uint64_t)p + 12u > A.T) return kNgTailBlock;
  const uint8_t *h = A.d + p;
  const uint32_t type = rd32(h, A.be), total = rd32(h + 4, A.be);
  if (ng_state_type(type)) return kNgTailState;
  if (total < 12u || (total & 3u) || (uint64_t)p + total > A.T) return kNgTailBlock;
  next = p + total;
  if (type == GPD_PCAPNG_BLOCK_ENHANCED || type == GPD_PCAPNG_BLOCK_PACKET) {
    if (total < 32u) return kNgTailBlock;
    const uint32_t idx = type == GPD_PCAPNG_BLOCK_ENHANCED ? rd32(h + 8, A.be) : rd16(h + 8, A.be);
    if (idx >= A.nif) return kNgTailBlock;
    cap = rd32(h + 20, A.be);
    if (cap > total - 32u) return kNgTailBlock;
    off = p + 28u;
    if (!((A.keep >> idx) & 1u)) return A.drop_is_error ? (int)kNgTailBlock : 0;
    return 1;
  }
  if (type == GPD_PCAPNG_BLOCK_SIMPLE) {
    if (total < 16u || A.nif == 0u) return kNgTailBlock;
    const uint32_t wire = rd32(h + 8, A.be);
    cap = A.snaplen0 != 0u && wire > A.snaplen0 ? A.snaplen0 : wire;
    if (cap > total - 16u) return kNgTailBlock;
    off = p + 12u;
    if (!(A.keep & 1u)) return A.drop_is_error ? (int)kNgTailBlock : 0;
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

struct NgFmt {
  using Args = NgArgs;
  static constexpr bool kStopKeeps = true;
  // A re-walk moves the true walk on by one lane's segments per round (a lane fixes its own
  // segments in order; the next lane sees the result in the next round), so a run of refuted
  // segments takes as many rounds as it spans lanes: nested captures refute every segment they
  // cover.  64 rounds of a few microseconds each bound what an adversarial chunk can cost.
  static constexpr int kFixRounds = 64;

  static __device__ __forceinline__ int step(const NgArgs &A, uint32_t p, uint32_t &off, uint32_t &cap,
                                             uint32_t &next) {
    return ng_step(A, p, off, cap, next);
  }
  // (a block's kind and its packet's place take the whole step to tell again)
  static __device__ __forceinline__ int emit(const NgArgs &A, uint32_t p, uint32_t &off, uint32_t &cap,
                                             uint32_t &next) {
    return ng_step(A, p, off, cap, next);
  }

  // Speculation: the first plausible chain head of the segment
  static __device__ __forceinline__ uint32_t speculate(const NgArgs &A, uint32_t lo, uint32_t hi) {
    for (uint32_t x = lo; x < hi && (uint64_t)x + 12u <= A.T; x += 4u) {
      uint32_t type = *reinterpret_cast<const uint32_t *>(A.d + x);
      if (A.be) type = __builtin_bswap32(type);
      if (type == 0u || (type > 6u && type != GPD_PCAPNG_BLOCK_SECTION) || type == 4u) continue;
      if (ng_plausible(A, x)) return x;
    }
    return kNone;
  }
};

}  // namespace

__global__ __launch_bounds__(256) void ng_walk(NgArgs A) { seg_walk_body<NgFmt>(A); }
__global__ __launch_bounds__(1024) void ng_stitch(NgArgs A) { seg_stitch_body<NgFmt>(A); }
__global__ __launch_bounds__(256) void ng_fill(NgArgs A) { seg_fill_body<NgFmt>(A); }

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
