// gpd_tcpstream.hip — TCP stream assembly (include/gpd_tcpstream.h): the Reassembly lists
// tcpassembly's Assembler hands to its streams (tcpassembly/assembly.go:533-607, the drain
// :235-266,645-657 and FlushAll :276-287), built from the grouped segment hand-off
// (gpd_tcpseg.hip) with one wave per connection, and the records' bytes gathered into
// per-connection streams.
//
// Launches, separated by launch boundaries only (no kernel waits on another workgroup):
//
//   ta_pages_sum_kernel   per 2,048 segments: the pages they would be buffered in,
//                         max(1, ceil(payload_len / 1900)) each
//   ta_scan_kernel        one workgroup: exclusive scan of the block sums (gpd_compact.h)
//   ta_pages_apply_kernel the exclusive scan per segment: a segment's first page id, and with it
//                         a group's private record region (a page or a segment yields one record
//                         at most, so a group's pages bound its records)
//   ta_walk_kernel        one wave per group: the assembler's state machine
//                         (gpd_tcpstream_walk.h) on lane 0, the in-order run on all 64 lanes;
//                         records into the private region, totals per group
//   ta_group_sum / scan / apply   the groups' record, byte and call counts scanned (three arrays at
//                         once; the calls only for their total: a million waves adding to one
//                         word would queue up behind each other)
//   ta_totals_kernel      out[] for the host, which decides here whether anything is written
//   ta_place_kernel       one wave per group: its records to their dense places with the final
//                         stream_off, its stream record, its connection state
//   gather_kernel         the shared bandwidth path (gpd_gather.h) with one source: a wave per 64
//                         consecutive records, whose bytes are one contiguous run of the output,
//                         in 16-byte-aligned output chunks
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gpd_compact.h"
#include "gpd_gather.h"
#include "gpd_internal.h"
#include "gpd_stream_util.h"
#include "gpd_tcpstream_walk.h"

namespace gpd {
namespace {

static_assert(sizeof(gpd_tcp_conn) == 8 && sizeof(gpd_tcp_asm_opts) == 8 && sizeof(gpd_tcp_reasm) == 32 &&
                  sizeof(gpd_tcp_stream) == 48 && sizeof(TsmNode) == 32,
              "include/gpd_tcpstream.h layouts");

constexpr uint32_t kWalkWaves = 4;  // waves (groups) per walk / place workgroup

struct TaArgs {
  const gpd_tcp_seg *segs;
  uint32_t cnt;
  const gpd_tcp_group *groups;
  uint32_t ng;
  gpd_tcp_conn *state;
  uint32_t id_bound;
  uint32_t max_pages, close_all;
  gpd_tcp_reasm *recs;  // the caller's
  gpd_tcp_stream *streams;
  // scratch of the context
  uint64_t *res;        // [0..3] out[], [4] pages in all (the one atomic: a word per 2,048 segments)
  uint32_t *pbase;      // cnt + 1: a segment's first page id
  uint32_t *blk;        // block sums of the scan in flight: (nblk + 1) words per array
  uint32_t nblk;
  uint32_t *gsc;        // [3][ng]: records, bytes and calls per group -> their exclusive scans
  gpd_tcp_stream *sstr; // ng: the stream records before their places are known
  TsmNode *nodes;       // one per page
  gpd_tcp_reasm *precs; // one per page: the groups' private record regions
};

// ---- the scans (gpd_stream_util.h) --------------------------------------------------------------
__global__ __launch_bounds__(256) void ta_pages_sum_kernel(TaArgs A) {
  scan_sum(A.cnt, A.blk, A.res + 4, [&A](uint32_t i) { return tsm_pages(A.segs[i].payload_len); });
}
__global__ __launch_bounds__(256) void ta_pages_apply_kernel(TaArgs A) {
  scan_apply(A.cnt, A.blk, A.pbase, true, [&A](uint32_t i) { return tsm_pages(A.segs[i].payload_len); });
}
// blockIdx.y: the array (0 records, 1 bytes, 2 calls)
__global__ __launch_bounds__(256) void ta_group_sum_kernel(TaArgs A) {
  const uint32_t *v = A.gsc + (size_t)blockIdx.y * A.ng;
  scan_sum(A.ng, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), nullptr, [v](uint32_t i) { return v[i]; });
}
__global__ __launch_bounds__(256) void ta_group_apply_kernel(TaArgs A) {
  uint32_t *v = A.gsc + (size_t)blockIdx.y * A.ng;
  scan_apply(A.ng, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), v, false, [v](uint32_t i) { return v[i]; });
}
__global__ __launch_bounds__(1024) void ta_scan_kernel(TaArgs A) {
  compact_scan(A.blk + (size_t)blockIdx.x * (A.nblk + 1u), A.nblk);
}

// ---- the walk ---------------------------------------------------------------------------------
__device__ __forceinline__ void conn_from_lane0(TsmConn &c) {  // (lane 0 is the wave's first lane)
  c.exists = first_lane(c.exists);
  c.valid = first_lane(c.valid);
  c.next_seq = first_lane(c.next_seq);
  c.first = first_lane(c.first);
  c.last = first_lane(c.last);
  c.pages = first_lane(c.pages);
  c.nrec = first_lane(c.nrec);
  c.ncalls = first_lane(c.ncalls);
  c.completed = first_lane(c.completed);
  c.nbytes = first_lane(c.nbytes);
}

__device__ __forceinline__ gpd_tcp_seg load_seg(const gpd_tcp_seg *p) {
  gpd_tcp_seg s;
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  uint4 *d = reinterpret_cast<uint4 *>(&s);
  d[0] = q[0];
  d[1] = q[1];
  return s;
}

// The group's segments clamped to segs[] (the arrays are the caller's).
__device__ __forceinline__ void group_range(const TaArgs &A, const gpd_tcp_group &G, uint32_t &start, uint32_t &count) {
  start = min(G.start, A.cnt);
  count = min(G.count, A.cnt - start);
}

// One wave per group.  The sequential step runs on lane 0.  On top of it the wave takes the
// in-order run: with the connection open, nextSeq known and no page buffered, the following
// segments (up to 64) whose seq is nextSeq plus the payload bytes before them in the run, and that
// carry neither FIN nor RST, are each what :591-602 makes of them: one call, one record, skip 0,
// no flags, the whole payload.  The first segment that breaks the chain takes the step.
__global__ __launch_bounds__(64 * kWalkWaves) void ta_walk_kernel(TaArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (g >= A.ng) return;
  const gpd_tcp_group G = A.groups[g];
  uint32_t start, count;
  group_range(A, G, start, count);
  const bool un = G.flow_id == GPD_TCP_UNGROUPED;
  uint32_t open = 0, ns = 0;
  if (!un && A.state && G.flow_id < A.id_bound) {
    const gpd_tcp_conn s = A.state[G.flow_id];
    open = s.flags & GPD_TCP_CONN_OPEN;
    ns = open ? s.next_seq : 0u;
  }
  TsmConn c;
  tsm_conn_init(c, open, ns);
  const uint32_t p0 = A.pbase[start];
  const TsmIo io{A.nodes, A.precs + p0, A.pbase[start + count] - p0, A.max_pages};
  if (!un) {
    uint32_t i = 0;
    while (i < count) {
#ifndef GPD_TSM_NO_CHAIN  // (A/B: tools/tcpstream_time.py)
      if (c.exists && c.valid && c.first == kTsmNil) {
        const uint32_t j = i + lane;
        const bool in = j < count;
        gpd_tcp_seg s{};
        if (in) s = load_seg(A.segs + start + j);
        const uint32_t len = in ? s.payload_len : 0u;
        const uint32_t incl = wave_scan32(len, lane), excl = incl - len;
        const bool ok = in && s.seq == c.next_seq + excl && !(s.flags & (GPD_TCP_FIN | GPD_TCP_RST)) &&
                        (len > 0u || (s.flags & GPD_TCP_SYN));
        const uint64_t m = __ballot(ok);
        const uint32_t run = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
        if (run) {
          if (lane < run && c.nrec + lane < io.cap) {
            const v4u r0{s.packet, len ? s.payload_off : 0u, len, 0u};
            const v4u r1{c.nbytes + excl, 0u, c.ncalls + lane, 0u};
            v4u *d = reinterpret_cast<v4u *>(io.recs + c.nrec + lane);
            d[0] = r0;
            d[1] = r1;
          }
          const uint32_t total = __shfl(incl, (int)run - 1, 64);
          c.nrec += run;
          c.ncalls += run;
          c.nbytes += total;
          c.next_seq += total;
          i += run;
          continue;
        }
      }
#endif
      if (lane == 0) {
        const gpd_tcp_seg s = load_seg(A.segs + start + i);
        tsm_step(c, io, s, A.pbase[start + i]);
      }
      conn_from_lane0(c);
      ++i;
    }
    if (lane == 0) tsm_finish(c, io, A.close_all != 0);
  }
  if (lane == 0) {
    A.gsc[g] = un ? 0u : c.nrec;
    A.gsc[(size_t)A.ng + g] = un ? 0u : c.nbytes;
    A.gsc[2 * (size_t)A.ng + g] = un ? 0u : c.ncalls;
    gpd_tcp_stream S{};
    S.flow_id = G.flow_id;
    S.nrec = c.nrec;
    S.ncalls = c.ncalls;
    S.nbytes = c.nbytes;
    S.completed = c.completed;
    S.open = c.exists;
    S.next_seq = c.exists ? c.next_seq : 0u;
    A.sstr[g] = S;
  }
}

__global__ __launch_bounds__(64) void ta_totals_kernel(TaArgs A) {
  if (threadIdx.x != 0) return;
  A.res[0] = A.blk[A.nblk];
  A.res[1] = A.ng - (A.groups[A.ng - 1u].flow_id == GPD_TCP_UNGROUPED ? 1u : 0u);
  A.res[2] = A.blk[(size_t)(A.nblk + 1u) + A.nblk];
  A.res[3] = A.blk[2 * (size_t)(A.nblk + 1u) + A.nblk];
}

// One wave per group: the private records to recs[first_rec ...] with the stream's byte offset
// added, the stream record, the connection's state.
__global__ __launch_bounds__(64 * kWalkWaves) void ta_place_kernel(TaArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (g >= A.ng) return;
  const gpd_tcp_group G = A.groups[g];
  if (G.flow_id == GPD_TCP_UNGROUPED) return;
  uint32_t start, count;
  group_range(A, G, start, count);
  gpd_tcp_stream S = A.sstr[g];
  const uint32_t fr = A.gsc[g], bo = A.gsc[(size_t)A.ng + g];
  const v4u *src = reinterpret_cast<const v4u *>(A.precs + A.pbase[start]);
  v4u *dst = reinterpret_cast<v4u *>(A.recs + fr);
  for (uint32_t r = lane; r < S.nrec; r += 64u) {
    const v4u a = src[2u * r];
    v4u b = src[2u * r + 1u];
    const uint64_t so = (((uint64_t)b.y << 32) | b.x) + bo;
    b.x = (uint32_t)so;
    b.y = (uint32_t)(so >> 32);
    dst[2u * r] = a;
    dst[2u * r + 1u] = b;
  }
  if (lane == 0) {
    S.first_rec = fr;
    S.byte_off = bo;
    const v4u *s4 = reinterpret_cast<const v4u *>(&S);
    v4u *d4 = reinterpret_cast<v4u *>(A.streams + g);
    d4[0] = s4[0];
    d4[1] = s4[1];
    d4[2] = s4[2];
    if (A.state && G.flow_id < A.id_bound) A.state[G.flow_id] = gpd_tcp_conn{S.next_seq, S.open ? GPD_TCP_CONN_OPEN : 0u};
  }
}

// ---- the gather (gpd_gather.h): one source, the records loaded from recs[] ------------------------
struct RecSource : GatherBases<1> {
  const gpd_tcp_reasm *recs;
  const uint32_t *offset;
  uint32_t n;
  __device__ __forceinline__ GatherRec load(uint64_t i) const {
    const v4u *p = reinterpret_cast<const v4u *>(recs + i);
    const v4u a = p[0], b = p[1];  // packet, src_off, len, skip | stream_off, call, flags
    // (a record whose packet is not the batch's reads as zeros)
    return GatherRec{((uint64_t)b.y << 32) | b.x, a.x < n ? (int64_t)offset[a.x] + (int64_t)a.y : kNoSrc, a.z, 0u};
  }
};

}  // namespace
}  // namespace gpd

extern "C" int gpd_tcp_assemble(gpd_ctx *ctx, const gpd_batch *in, const gpd_tcp_seg *segs, uint64_t count,
                                const gpd_tcp_group *groups, uint64_t ngroups, gpd_tcp_conn *state,
                                uint32_t id_bound, const gpd_tcp_asm_opts *opts, gpd_tcp_reasm *recs,
                                uint64_t max_recs, gpd_tcp_stream *streams, uint8_t *bytes, uint64_t max_bytes,
                                uint64_t out[4], void *stream) {
  using namespace gpd;
  const char *who = "gpd_tcp_assemble";
  if (!ctx || !in || !opts || !out) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  out[0] = out[1] = out[2] = out[3] = 0;
  if (in->n > 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 256)", who, (unsigned long long)in->n);
  if (count >= 0x80000000ull)
    return set_error(GPD_ERR_INVALID, "%s: %llu segments (max 2^31 - 1)", who, (unsigned long long)count);
  if (ngroups > count)
    return set_error(GPD_ERR_INVALID, "%s: %llu groups of %llu segments", who, (unsigned long long)ngroups,
                     (unsigned long long)count);
  if (max_recs && !recs) return set_error(GPD_ERR_INVALID, "%s: null recs with max_recs > 0", who);
  if (max_bytes && !bytes) return set_error(GPD_ERR_INVALID, "%s: null bytes with max_bytes > 0", who);
  if (bytes && !recs) return set_error(GPD_ERR_INVALID, "%s: bytes without recs", who);
  if (recs && !streams) return set_error(GPD_ERR_INVALID, "%s: recs without streams[]", who);
  if (((uintptr_t)recs & 15u) || ((uintptr_t)streams & 15u) || ((uintptr_t)bytes & 15u))
    return set_error(GPD_ERR_INVALID, "%s: recs, streams and bytes must be 16-byte aligned", who);
  if (((uintptr_t)segs & 15u) || ((uintptr_t)groups & 15u))
    return set_error(GPD_ERR_INVALID, "%s: segs and groups must be 16-byte aligned", who);
  if (count == 0 || ngroups == 0) return GPD_OK;
  if (!segs || !groups) return set_error(GPD_ERR_INVALID, "%s: null segs or groups", who);
  if (!in->data || !in->offset || !in->caplen)
    return set_error(GPD_ERR_INVALID, "%s: batch data/offset/caplen must be non-NULL", who);
  if (in->data_len >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: data_len %llu outside the 32-bit offset range", who,
                     (unsigned long long)in->data_len);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  TaArgs A{};
  A.segs = segs;
  A.cnt = (uint32_t)count;
  A.groups = groups;
  A.ng = (uint32_t)ngroups;
  A.state = state;
  A.id_bound = state ? id_bound : 0u;
  A.max_pages = opts->max_pages_per_connection;
  A.close_all = opts->close_all;
  A.recs = recs;
  A.streams = streams;
  // scratch sized by the hand-off: result words, page ids, block sums, the groups' counts and streams
  const uint32_t nblk_s = (A.cnt + kCompactBlock - 1u) / kCompactBlock;
  const uint32_t nblk_g = (A.ng + kCompactBlock - 1u) / kCompactBlock;
  const size_t b_res = 64, b_pbase = up16(((size_t)A.cnt + 1) * 4);
  const size_t b_blk = up16(3 * ((size_t)std::max(nblk_s, nblk_g) + 1) * 4);
  const size_t b_gsc = up16(3 * (size_t)A.ng * 4), b_sstr = (size_t)A.ng * sizeof(gpd_tcp_stream);
  const size_t fixed = b_res + b_pbase + b_blk + b_gsc + b_sstr;
  // One slot holds the page arrays behind the fixed part; it grows once the pages are counted.
  // The first guess (one page per segment) is right for every payload up to 1900 bytes.
  auto carve = [&](uint8_t *base) {
    A.res = reinterpret_cast<uint64_t *>(base);
    A.pbase = reinterpret_cast<uint32_t *>(base + b_res);
    A.blk = reinterpret_cast<uint32_t *>(base + b_res + b_pbase);
    A.gsc = reinterpret_cast<uint32_t *>(base + b_res + b_pbase + b_blk);
    A.sstr = reinterpret_cast<gpd_tcp_stream *>(base + b_res + b_pbase + b_blk + b_gsc);
  };
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 17, fixed + 2 * (size_t)A.cnt * sizeof(TsmNode)));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  carve(base);
  A.nblk = nblk_s;
  GPD_TRY(hipMemsetAsync(A.res, 0, b_res, s));
  hipLaunchKernelGGL(ta_pages_sum_kernel, dim3(nblk_s), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t npages = 0;
  GPD_TRY(hipMemcpyAsync(&npages, A.res + 4, 8, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  if (npages > 0xFFFFFFFFull)
    return set_error(GPD_ERR_INVALID, "%s: %llu pages (max 2^32 - 1)", who, (unsigned long long)npages);
  // the page arrays: nodes and private records, 32 bytes each per page.  Growing the slot
  // replaces it; all it held so far is the block sums, which are computed again.
  const size_t b_pages = (size_t)npages * sizeof(TsmNode);
  if (npages > A.cnt) {
    base = static_cast<uint8_t *>(ctx_scratch(ctx, 17, fixed + 2 * b_pages));
    if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
    carve(base);
    GPD_TRY(hipMemsetAsync(A.res, 0, b_res, s));
    hipLaunchKernelGGL(ta_pages_sum_kernel, dim3(nblk_s), dim3(256), 0, s, A);
  }
  A.nodes = reinterpret_cast<TsmNode *>(base + fixed);
  A.precs = reinterpret_cast<gpd_tcp_reasm *>(base + fixed + b_pages);
  hipLaunchKernelGGL(ta_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(ta_pages_apply_kernel, dim3(nblk_s), dim3(256), 0, s, A);
  const unsigned wgrid = (A.ng + kWalkWaves - 1u) / kWalkWaves;
  hipLaunchKernelGGL(ta_walk_kernel, dim3(wgrid), dim3(64 * kWalkWaves), 0, s, A);
  A.nblk = nblk_g;
  hipLaunchKernelGGL(ta_group_sum_kernel, dim3(nblk_g, 3), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ta_scan_kernel, dim3(3), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(ta_group_apply_kernel, dim3(nblk_g, 2), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ta_totals_kernel, dim3(1), dim3(64), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t tot[4] = {0, 0, 0, 0};
  GPD_TRY(hipMemcpyAsync(tot, A.res, 32, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 4; ++k) out[k] = tot[k];
  if (!recs && !max_recs) return GPD_OK;  // the sizing call
  const bool gather = bytes != nullptr || max_bytes != 0;
  if (tot[0] > max_recs)
    return set_error(GPD_ERR_INVALID, "%s: %llu records, max_recs is %llu", who, (unsigned long long)tot[0],
                     (unsigned long long)max_recs);
  if (gather && tot[2] > max_bytes)
    return set_error(GPD_ERR_INVALID, "%s: %llu bytes, max_bytes is %llu", who, (unsigned long long)tot[2],
                     (unsigned long long)max_bytes);
  hipLaunchKernelGGL(ta_place_kernel, dim3(wgrid), dim3(64 * kWalkWaves), 0, s, A);
  if (gather) {
    RecSource G{};
    G.set(0, in->data, in->data_len);
    G.recs = recs;
    G.offset = in->offset;
    G.n = (uint32_t)in->n;
    launch_gather(G, (uint32_t)tot[0], bytes, tot[2], s);
  }
  GPD_TRY(hipGetLastError());
  GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}
