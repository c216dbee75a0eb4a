// gpd_pcapwalk.hip — the pcap record walk on the GPU, for gpd_decode_pcap_at (include/gpd_pcap.h).
//
// The host walk (gpd_pcap.cpp) reads every record header of the capture in host memory, and on
// a GPU box's share of host cores that walk, not PCIe, bounds a replay.  Here the
// capture's bytes travel to HBM in fixed byte chunks first, and the records are found there by
// the segmented walk of gpd_segwalk.h (pw_walk, pw_stitch, pw_fill), with pcap's rules:
//
//   step       a record that passes every ReadPacketData check (pcapgo/read.go:120-137) and
//              whose data lies inside the bytes held is a packet; anything else stops the walk;
//   speculate  a segment's first position whose 8-header chain passes every such check, chosen
//              among near-by candidates as described below;
//   a stop     on the true walk — a rejected record, a capture that ends in a partial record —
//              like a speculation that the true walk does not meet after kFixRounds rounds, sets
//              status 1 and count 0: the host walks from this chunk's entry on instead, with
//              the reference's exact stop and error text.
//
// The decode kernel then reads the record count from the control block (KParams::n_dev).
#include "gpd_segwalk.h"

namespace gpd {

namespace {

struct PcapFmt {
  using Args = PwArgs;
  static constexpr bool kStopKeeps = false;
  // Payload bytes that read as a chain of plausible headers (config 5's 64-B records: a view 3
  // bytes into each record chains 16,400-byte "records" forever) cost a few microseconds of the
  // stitch workgroup instead of a host walk of the chunk.
  static constexpr int kFixRounds = 4;

  // One ReadPacketData step at p of the chunk's T bytes: 1 when the record passes every check
  // and its data lies inside the bytes; else the stop 4 (PwCtl::status: a record the host would
  // reject, or one cut by the end of the capture: the host decides those).
  static __device__ __forceinline__ int step(const PwArgs &A, uint32_t p, uint32_t &off, uint32_t &cap,
                                             uint32_t &next) {
    if (p + 16u > A.T) return 4;
    const uint8_t *h = A.d + p;
    cap = rd32(h + 8, A.be);
    const uint32_t wire = rd32(h + 12, A.be);
    if (cap > A.snaplen || cap > wire) return 4;     // read.go:125-131
    if ((uint64_t)p + 16u + cap > A.T) return 4;     // read.go:133-134
    off = p + 16u;
    next = p + 16u + cap;
    return 1;
  }

  // ... at a record the walk took: its length is all the fill needs
  static __device__ __forceinline__ int emit(const PwArgs &A, uint32_t p, uint32_t &off, uint32_t &cap,
                                             uint32_t &next) {
    cap = rd32(A.d + p + 8, A.be);
    off = p + 16u;
    next = off + cap;
    return 1;
  }

  // A header at x whose chain of 8 passes every check (or reaches the capture's end exactly, or
  // the end of the bytes this chunk holds, after at least one).  Three things the reader accepts
  // are not taken as evidence here: an all-zero header (zero-filled payload is a chain of valid
  // empty records), a fraction-of-second field of a second or more (bytes that merely pass the
  // length checks rarely hold one below 10^6, resp. 10^9), and timestamps that run backwards.
  // A wrong speculation is caught by the stitch, at the cost of the host walk; these keep it rare.
  static __device__ __forceinline__ bool plausible(const PwArgs &A, uint32_t x) {
    uint32_t psec = 0, pfrac = 0;
    for (int k = 0; k < 8; k++) {
      if (x >= A.T) return k > 0 && (A.last ? x == A.T : true);
      uint32_t off, cap, next;
      if (step(A, x, off, cap, next) != 1) return false;
      const uint8_t *h = A.d + x;
      if ((rd32(h, false) | rd32(h + 4, false) | rd32(h + 8, false) | rd32(h + 12, false)) == 0u) return false;
      const uint32_t sec = rd32(h, A.be), frac = rd32(h + 4, A.be);
      if (frac >= (A.nano ? 1000000000u : 1000000u)) return false;  // not a sub-second count
      if (sec < psec || (sec == psec && frac < pfrac)) return false;  // time runs backwards
      psec = sec;
      pfrac = frac;
      x += 16u + cap;
    }
    return true;
  }

  // Speculation: the first plausible header of the segment
  // (when a record's original length equals its capture length, the view 4 bytes on —
  // seconds := fraction, fraction := length, length := original length — passes the same
  // checks and advances by the same steps as the true walk, forever).
  // Views of a true header shifted by a few bytes can chain in parallel with it too (64-B
  // records: the view one byte early reads length 64 << 8, a step of 205 records): of the
  // plausible positions within 8 bytes, the one with the shortest record is taken, and one
  // that is the 4-byte shift of a plausible header just before it is passed over.
  static __device__ __forceinline__ uint32_t speculate(const PwArgs &A, uint32_t lo, uint32_t hi) {
    const uint32_t lim = min(hi, lo + 16u + A.snaplen + 1u);
    uint32_t x = lo;
    while (x < lim) {
      if (!plausible(A, x)) {
        x++;
        continue;
      }
      uint32_t best = x, bc = rd32(A.d + x + 8, A.be);
      for (uint32_t y = x + 1; y < min(x + 8u, lim); y++)
        if (plausible(A, y)) {
          const uint32_t c = rd32(A.d + y + 8, A.be);
          if (c < bc) {
            best = y;
            bc = c;
          }
        }
      if (best >= 4u && plausible(A, best - 4u) && rd32(A.d + best + 4u, A.be) <= bc) {
        x = best + 1u;
        continue;
      }
      return best;
    }
    return kNone;
  }
};

}  // namespace

__global__ __launch_bounds__(256) void pw_walk(PwArgs A) { seg_walk_body<PcapFmt>(A); }
__global__ __launch_bounds__(1024) void pw_stitch(PwArgs A) { seg_stitch_body<PcapFmt>(A); }
__global__ __launch_bounds__(256) void pw_fill(PwArgs A) { seg_fill_body<PcapFmt>(A); }

hipError_t launch_pcap_walk(const PwArgs &A, hipStream_t stream) {
  const unsigned g = (A.nseg + 255u) / 256u;
  if (A.nseg > kPwMaxSeg) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pw_walk, dim3(g ? g : 1), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(pw_stitch, dim3(1), dim3(1024), 0, stream, A);
  return hipGetLastError();
}

hipError_t launch_pcap_fill(const PwArgs &A, hipStream_t stream) {
  const unsigned g = (A.nseg + 255u) / 256u;
  hipLaunchKernelGGL(pw_fill, dim3(g ? g : 1), dim3(256), 0, stream, A);
  return hipGetLastError();
}

}  // namespace gpd
