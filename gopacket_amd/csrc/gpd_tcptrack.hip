// gpd_tcptrack.hip — TCP connection tracking (include/gpd_tcptrack.h): reassembly's
// bidirectional connection (reassembly/memory.go:169-206), each packet's direction, and
// TCPSimpleFSM.CheckState (reassembly/tcpcheck.go:167-246) for every TCP packet of a decoded
// device batch, with one FSM per connection carried on the device from batch to batch.
//
// No lane, wave or workgroup walks a connection.  CheckState is a function of (state, t.dir) and
// of the packet's (SYN, ACK, FIN, RST, dir) only, so a packet is a map on 12 elements and the
// maps compose associatively (gpd_tcptrack_fsm.h).  The tracked packets are ordered by
// connection, stably, and a segmented inclusive scan of the maps over that order gives every
// packet the map from its connection's carried state to the state before it: the work per
// packet is a constant whatever the lengths of the connections.
//
//   tk_count_kernel     one lane per packet: is it tracked?  (mask bit, per-block count; every
//                       packet's verdict starts as GPD_TCP_UNTRACKED, its conn_id as GPD_FLOW_NONE)
//   tk_scan_kernel      one workgroup: exclusive scan of the block counts     } gpd_compact.h
//   tk_index_kernel     the tracked packets' indices in order                 }
//   flow_peer_kernel    (gpd_flow.hip) one lane per tracked packet: the reversed key's record,
//                       the connection c, and the packet's code and c's carried byte
//   sort_*_kernel       (gpd_radix_sort.h) the (c, index) pairs by c, stably; pairs only
//   tk_tile_kernel<0>   per tile of kTrkTile sorted packets: the tile's map and "holds a head"
//   tk_agg_kernel       one workgroup: segmented exclusive scan of the tile aggregates
//   tk_tile_kernel<1>   the tile again with its carry-in: verdicts scattered to packet order,
//                       and the lane at a connection's last packet writes the carried byte
//   tk_forget_kernel    gpd_tcp_tracker_forget
//
// Passes are separated by launch boundaries: no decoupled look-back, no spin on a global word.
// The carried byte of c is read by the peer kernel (into info[]) and written by the apply pass,
// a launch apart, so no lane reads a byte another lane of the same launch writes.
//
// A tile: 256 lanes, each with kTrkItems consecutive packets.  The lane folds its packets'
// maps (a constant number), the wave scans the lanes' folds (wave_scan32's shape, the value
// widened to the 64-bit map and the head flag), the four waves' totals meet in LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "gpd_compact.h"
#include "gpd_internal.h"
#include "gpd_radix_sort.h"
#include "gpd_tcptrack_fsm.h"
#include "../../include/gpd_flow.h"
#include "../../include/gpd_tcptrack.h"

struct gpd_tcp_tracker {
  gpd_ctx *ctx = nullptr;
  gpd_flowtable *ft = nullptr;
  int device = 0;
  int num_cus = 1;
  uint32_t cap = 0;      // the table's capacity: the id bound
  uint32_t missing = 0;  // SupportMissingEstablishment
  uint8_t *carried = nullptr;  // cap bytes, allocated on first use
  uint8_t *sa = nullptr, *sb = nullptr;  // scratch sized by the batch / by the tracked packets
  size_t sa_bytes = 0, sb_bytes = 0;
};

namespace gpd {
namespace {

constexpr uint32_t kTrkThreads = 256;
constexpr uint32_t kTrkWaves = kTrkThreads / 64u;
constexpr uint32_t kTrkItems = 8;                         // consecutive packets per lane
constexpr uint32_t kTrkTile = kTrkThreads * kTrkItems;    // packets per workgroup (tcptrack.SCAN_TILE)
constexpr uint32_t kAggRound = 256;                       // tiles the aggregate scan takes between barriers
                                                          // (tcptrack.AGG_ROUND)

__constant__ const fsm::GenTable g_gen = fsm::make_gen_table();
static_assert(fsm::make_gen_table().g[0][0] != 0 && fsm::compose(fsm::kIdentity, fsm::kIdentity) == fsm::kIdentity,
              "the generator table is a compile-time constant");

struct TkArgs {
  // the batch and its results
  const uint32_t *status, *hdr_off, *flow_id;
  const gpd_record *rec;
  uint32_t n, cap, missing;
  uint8_t *verdict;
  uint32_t *conn_id;  // may be NULL
  uint8_t *carried;
  // scratch
  uint32_t nblk;
  uint32_t *blk;
  uint64_t *mask;
  uint32_t *idx;
  unsigned long long *tally;  // [0] accepted, [1] connections
  uint32_t cnt;               // tracked packets (known on the host after the scan)
  const uint32_t *info;       // per tracked packet: code | carried byte << 8
  uint32_t ntile;
  uint64_t *agg_m, *pre;      // per tile: its map; the map carried into it
  uint32_t *agg_f;            // per tile: it holds a head
};

// Is packet i tracked?  The flow table keys it (gpd_flow.hip flow_key), its transport endpoint
// type is TCPPort, and its flow id is a record.
__device__ __forceinline__ bool tracked(const TkArgs &A, uint32_t i) {
  const uint32_t st = A.rec ? A.rec[i].status : A.status[i], ho = A.hdr_off[i];
  const uint32_t nt = GPD_STATUS_NET_EPT(st), tt = GPD_STATUS_TP_EPT(st);
  return nt != 0 && tt == 4u && GPD_HDR_NET(ho) != GPD_HDR_NONE && GPD_HDR_TP(ho) != GPD_HDR_NONE &&
         A.flow_id[i] < A.cap;
}

__global__ __launch_bounds__(256) void tk_count_kernel(TkArgs A) {
  compact_count(A.n, A.mask, A.blk, [&A](uint32_t i) {
    A.verdict[i] = (uint8_t)GPD_TCP_UNTRACKED;
    if (A.conn_id) A.conn_id[i] = GPD_FLOW_NONE;
    return tracked(A, i);
  });
}
__global__ __launch_bounds__(1024) void tk_scan_kernel(TkArgs A) { compact_scan(A.blk, A.nblk); }
__global__ __launch_bounds__(64) void tk_index_kernel(TkArgs A) { compact_index(A.blk, A.mask, A.idx, A.n); }

// ---- the segmented scan of maps ------------------------------------------------------------------
// A run of packets: the composition of its maps since its last head, and whether it holds one.
struct Seg {
  fsm::Map m;
  uint32_t f;
};
// a, then b: a head in b cuts a off
__device__ __forceinline__ Seg seg_op(const Seg &a, const Seg &b) {
  return Seg{b.f ? b.m : fsm::compose(a.m, b.m), a.f | b.f};
}
// wave_scan32 (gpd_compact.h) for Seg: inclusive in x, and the exclusive value (lane 0: empty)
__device__ __forceinline__ Seg wave_scan_seg(Seg &x, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const Seg y{__shfl_up(x.m, d, 64), __shfl_up(x.f, d, 64)};
    if (lane >= d) x = seg_op(y, x);
  }
  Seg e{__shfl_up(x.m, 1u, 64), __shfl_up(x.f, 1u, 64)};
  if (lane == 0u) e = Seg{fsm::kIdentity, 0u};
  return e;
}

template <bool APPLY>
__global__ __launch_bounds__(kTrkThreads) void tk_tile_kernel(TkArgs A, const uint2 *sorted) {
  __shared__ uint64_t wm[kTrkWaves];
  __shared__ uint32_t wf[kTrkWaves];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint32_t j0 = blockIdx.x * kTrkTile + t * kTrkItems;
  uint2 p[kTrkItems];
  if (j0 + kTrkItems <= A.cnt) {  // (sorted is 16-byte aligned and j0 a multiple of 8)
    const uint4 *s4 = reinterpret_cast<const uint4 *>(sorted + j0);
#pragma unroll
    for (uint32_t q = 0; q < kTrkItems / 2u; ++q) {
      const uint4 v = s4[q];
      p[2u * q] = make_uint2(v.x, v.y);
      p[2u * q + 1u] = make_uint2(v.z, v.w);
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kTrkItems; ++k)
      p[k] = j0 + k < A.cnt ? sorted[j0 + k] : make_uint2(0xFFFFFFFFu, 0u);  // (no connection has that id)
  }
  // the keys beside the lane's packets: a packet is a head when the one before has another key,
  // and its connection's last when the one after has
  const uint32_t before = (j0 > 0u && j0 <= A.cnt) ? sorted[j0 - 1u].x : 0xFFFFFFFFu;
  const uint32_t after = j0 + kTrkItems < A.cnt ? sorted[j0 + kTrkItems].x : 0xFFFFFFFFu;
  uint32_t inf[kTrkItems];
#pragma unroll
  for (uint32_t k = 0; k < kTrkItems; ++k) inf[k] = j0 + k < A.cnt ? A.info[p[k].y] : 0u;
  Seg L{fsm::kIdentity, 0u};
#pragma unroll
  for (uint32_t k = 0; k < kTrkItems; ++k) {
    if (j0 + k < A.cnt) {
      const bool head = p[k].x != (k ? p[k - 1u].x : before);
      const fsm::Map g = g_gen.g[A.missing][inf[k] & 31u];
      L = head ? Seg{g, 1u} : Seg{fsm::compose(L.m, g), L.f};
    }
  }
  const Seg X = wave_scan_seg(L, lane);  // L: inclusive now
  if (lane == 63u) {
    wm[w] = L.m;
    wf[w] = L.f;
  }
  __syncthreads();
  Seg pre{APPLY ? A.pre[blockIdx.x] : fsm::kIdentity, 0u};
  for (uint32_t k = 0; k < w; ++k) pre = seg_op(pre, Seg{wm[k], wf[k]});
  if (!APPLY) {
    if (t == kTrkThreads - 1u) {
      const Seg tot = seg_op(pre, L);
      A.agg_m[blockIdx.x] = tot.m;
      A.agg_f[blockIdx.x] = tot.f;
    }
    return;
  }
  // the map from the carried state to the state before the lane's first packet (when that
  // packet is no head), then the step function once per packet
  const Seg E = seg_op(pre, X);
  uint32_t e = 0, n_acc = 0, n_head = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTrkItems; ++k) {
    if (j0 + k < A.cnt) {
      const bool head = p[k].x != (k ? p[k - 1u].x : before);
      const uint32_t code = inf[k] & 31u, cb = fsm::elem_of_byte((inf[k] >> 8) & 15u);
      if (head) e = cb;
      else if (k == 0u) e = fsm::apply(E.m, cb);
      const uint32_t tdir = e >= 6u ? 1u : 0u;
      const fsm::Step s = fsm::step(e - 6u * tdir, tdir, code, A.missing != 0u);
      e = fsm::elem(s.state, s.tdir);
      A.verdict[A.idx[p[k].y]] = (uint8_t)fsm::verdict(s, code);
      const bool last = p[k].x != (k + 1u < kTrkItems ? p[k + 1u].x : after);
      if (last) A.carried[p[k].x] = (uint8_t)fsm::byte_of_elem(e);
      n_acc += s.accept;
      n_head += head ? 1u : 0u;
    }
  }
  // one atomic per counter per wave
  const uint32_t acc = wave_scan32(n_acc, lane), heads = wave_scan32(n_head, lane);
  if (lane == 63u) {
    if (acc) atomicAdd(A.tally + 0, (unsigned long long)acc);
    if (heads) atomicAdd(A.tally + 1, (unsigned long long)heads);
  }
}

// One workgroup: the segmented exclusive scan of the tile aggregates, kAggRound tiles between
// barriers; pre[b] = the map of the packets before tile b since the last head before it.
__global__ __launch_bounds__(kAggRound) void tk_agg_kernel(TkArgs A) {
  __shared__ uint64_t wm[kAggRound / 64u];
  __shared__ uint32_t wf[kAggRound / 64u];
  __shared__ uint64_t carry;
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  if (t == 0) carry = fsm::kIdentity;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < A.ntile; c0 += kAggRound) {
    const uint32_t b = c0 + t;
    Seg L = b < A.ntile ? Seg{A.agg_m[b], A.agg_f[b]} : Seg{fsm::kIdentity, 0u};
    const Seg X = wave_scan_seg(L, lane);
    if (lane == 63u) {
      wm[w] = L.m;
      wf[w] = L.f;
    }
    __syncthreads();
    Seg pre{carry, 0u};
    for (uint32_t k = 0; k < w; ++k) pre = seg_op(pre, Seg{wm[k], wf[k]});
    if (b < A.ntile) A.pre[b] = seg_op(pre, X).m;
    __syncthreads();
    if (t == kAggRound - 1u) carry = seg_op(pre, L).m;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void tk_forget_kernel(uint8_t *carried, uint32_t cap, const uint32_t *ids, uint64_t m) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < m; k += (uint64_t)gridDim.x * 256ull)
    if (ids[k] < cap) carried[ids[k]] = 0;
}

// The object's scratch buffer `buf` with at least `bytes` (its contents are not kept).
int grow(uint8_t *&buf, size_t &have, size_t bytes, const char *who) {
  if (have >= bytes) return GPD_OK;
  if (buf) GPD_TRY(hipFree(buf));
  buf = nullptr;
  have = 0;
  if (hipMalloc(reinterpret_cast<void **>(&buf), bytes) != hipSuccess) {
    buf = nullptr;
    return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  }
  have = bytes;
  return GPD_OK;
}

// The carried bytes, zeroed, on first use (the device is the caller's DeviceScope's).
int need_carry(gpd_tcp_tracker *t, const char *who) {
  if (t->carried) return GPD_OK;
  if (hipMalloc(reinterpret_cast<void **>(&t->carried), t->cap) != hipSuccess) {
    t->carried = nullptr;
    return set_error(GPD_ERR_NOMEM, "%s: state allocation failed", who);
  }
  GPD_TRY(hipMemset(t->carried, 0, t->cap));
  return GPD_OK;
}

}  // namespace
}  // namespace gpd

extern "C" int gpd_tcp_tracker_create(gpd_ctx *ctx, gpd_flowtable *flowtable, const gpd_tcp_track_opts *opts,
                                      gpd_tcp_tracker **t) {
  using namespace gpd;
  if (!ctx || !flowtable || !t) return set_error(GPD_ERR_INVALID, "gpd_tcp_tracker_create: null argument");
  *t = nullptr;
  if (opts && opts->reserved)
    return set_error(GPD_ERR_INVALID, "gpd_tcp_tracker_create: reserved option word is %u", opts->reserved);
  if (flow_device(flowtable) != ctx_device(ctx))
    return set_error(GPD_ERR_INVALID, "gpd_tcp_tracker_create: the flow table lives on device %d, the context on %d",
                     flow_device(flowtable), ctx_device(ctx));
  auto *o = new (std::nothrow) gpd_tcp_tracker();
  if (!o) return set_error(GPD_ERR_NOMEM, "gpd_tcp_tracker_create: out of memory");
  o->ctx = ctx;
  o->ft = flowtable;
  o->device = ctx_device(ctx);
  o->num_cus = ctx_num_cus(ctx);
  o->cap = (uint32_t)flow_capacity(flowtable);  // (at most 2^31)
  o->missing = opts && opts->support_missing_establishment ? 1u : 0u;
  *t = o;
  return GPD_OK;
}

extern "C" void gpd_tcp_tracker_destroy(gpd_tcp_tracker *t) {
  if (!t) return;
  if (t->carried || t->sa || t->sb) {
    gpd::DeviceScope dscope_;
    if (dscope_.set(t->device) == hipSuccess) {
      if (t->carried) (void)hipFree(t->carried);
      if (t->sa) (void)hipFree(t->sa);
      if (t->sb) (void)hipFree(t->sb);
    }
  }
  delete t;
}

extern "C" int gpd_tcp_tracker_run(gpd_tcp_tracker *t, const gpd_batch *in, const gpd_result *res,
                                   const uint32_t *flow_id, uint8_t *verdict, uint32_t *conn_id,
                                   uint64_t out[4], void *stream) {
  using namespace gpd;
  const char *who = "gpd_tcp_tracker_run";
  if (!t || !in || !res || !out) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  out[0] = out[1] = out[2] = out[3] = 0;
  if (in->n > 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 256)", who, (unsigned long long)in->n);
  if (in->n == 0) return GPD_OK;
  if (!flow_id || !verdict) return set_error(GPD_ERR_INVALID, "%s: flow_id and verdict must be non-NULL", who);
  if (!in->data || !in->offset || !in->caplen)
    return set_error(GPD_ERR_INVALID, "%s: batch data/offset/caplen must be non-NULL", who);
  if (!res->hdr_off || (!res->records && !res->status))
    return set_error(GPD_ERR_INVALID, "%s: needs hdr_off and status (or records)", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(t->device));
  const hipStream_t s = (hipStream_t)stream;
  int rc = need_carry(t, who);
  if (rc != GPD_OK) return rc;
  TkArgs A{};
  A.status = res->status;
  A.hdr_off = res->hdr_off;
  A.flow_id = flow_id;
  A.rec = res->records;
  A.n = (uint32_t)in->n;
  A.cap = t->cap;
  A.missing = t->missing;
  A.verdict = verdict;
  A.conn_id = conn_id;
  A.carried = t->carried;
  // the compaction's scratch, sized by the batch: the tallies, counts, mask, indices
  const uint32_t n = A.n;
  A.nblk = (n + kCompactBlock - 1u) / kCompactBlock;
  const size_t b_blk = up16(((size_t)A.nblk + 1) * 4), b_mask = up16(((size_t)n + 63) / 64 * 8);
  rc = grow(t->sa, t->sa_bytes, 16 + b_blk + b_mask + up16((size_t)n * 4), who);
  if (rc != GPD_OK) return rc;
  A.tally = reinterpret_cast<unsigned long long *>(t->sa);
  A.blk = reinterpret_cast<uint32_t *>(t->sa + 16);
  A.mask = reinterpret_cast<uint64_t *>(t->sa + 16 + b_blk);
  A.idx = reinterpret_cast<uint32_t *>(t->sa + 16 + b_blk + b_mask);
  GPD_TRY(hipMemsetAsync(A.tally, 0, 16, s));
  hipLaunchKernelGGL(tk_count_kernel, dim3(A.nblk), dim3(256), 0, s, A);
  hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint32_t total = 0;
  GPD_TRY(hipMemcpyAsync(&total, A.blk + A.nblk, 4, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  if (total == 0) return GPD_OK;
  A.cnt = total;
  hipLaunchKernelGGL(tk_index_kernel, dim3(A.nblk), dim3(64), 0, s, A);
  // the sort's and the scan's scratch, sized by the tracked packets
  const uint32_t stile = (total + kSortTile - 1u) / kSortTile;
  A.ntile = (total + kTrkTile - 1u) / kTrkTile;
  const size_t b_pair = up16((size_t)total * 8), b_info = up16((size_t)total * 4);
  const size_t b_hist = (size_t)stile * 256 * 4, b_m = up16((size_t)A.ntile * 8), b_f = up16((size_t)A.ntile * 4);
  rc = grow(t->sb, t->sb_bytes, 2 * b_pair + b_info + b_hist + 2 * b_m + b_f, who);
  if (rc != GPD_OK) return rc;
  uint2 *pa = reinterpret_cast<uint2 *>(t->sb), *pb = reinterpret_cast<uint2 *>(t->sb + b_pair);
  uint32_t *info = reinterpret_cast<uint32_t *>(t->sb + 2 * b_pair);
  uint32_t *hist = reinterpret_cast<uint32_t *>(t->sb + 2 * b_pair + b_info);
  A.info = info;
  A.agg_m = reinterpret_cast<uint64_t *>(t->sb + 2 * b_pair + b_info + b_hist);
  A.pre = reinterpret_cast<uint64_t *>(t->sb + 2 * b_pair + b_info + b_hist + b_m);
  A.agg_f = reinterpret_cast<uint32_t *>(t->sb + 2 * b_pair + b_info + b_hist + 2 * b_m);
  const PeerArgs Q{in->data, in->data_len, in->offset, res->status, res->hdr_off, res->records,
                   flow_id, A.idx, total, t->carried, pa, info, conn_id};
  GPD_TRY(launch_flow_peers(t->ft, Q, s));
  const SortArgs S{total, stile, hist};
  const uint32_t passes = sort_passes(t->cap - 1u);  // c < capacity
  const uint2 *src = sort_leading_passes(S, pa, pb, passes, s);
  uint2 *sorted = src == pa ? pb : pa;
  sort_last_pass(S, src, passes, PairSink{sorted}, s);
  hipLaunchKernelGGL(tk_tile_kernel<false>, dim3(A.ntile), dim3(kTrkThreads), 0, s, A, sorted);
  hipLaunchKernelGGL(tk_agg_kernel, dim3(1), dim3(kAggRound), 0, s, A);
  hipLaunchKernelGGL(tk_tile_kernel<true>, dim3(A.ntile), dim3(kTrkThreads), 0, s, A, sorted);
  GPD_TRY(hipGetLastError());
  unsigned long long tally[2] = {0, 0};
  GPD_TRY(hipMemcpyAsync(tally, A.tally, 16, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  out[0] = total;
  out[1] = tally[0];
  out[2] = total - tally[0];
  out[3] = tally[1];
  return GPD_OK;
}

extern "C" int gpd_tcp_tracker_states(gpd_tcp_tracker *t, uint8_t *out, void *stream) {
  using namespace gpd;
  const char *who = "gpd_tcp_tracker_states";
  if (!t || !out) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(t->device));
  const int rc = need_carry(t, who);
  if (rc != GPD_OK) return rc;
  GPD_TRY(hipMemcpyAsync(out, t->carried, t->cap, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GPD_OK;
}

extern "C" int gpd_tcp_tracker_forget(gpd_tcp_tracker *t, const uint32_t *ids, uint64_t m, void *stream) {
  using namespace gpd;
  const char *who = "gpd_tcp_tracker_forget";
  if (!t || (m && !ids)) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  if (m == 0 || !t->carried) return GPD_OK;  // (nothing carried yet: every connection is fresh)
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(t->device));
  const unsigned grid = (unsigned)std::min<uint64_t>((m + 255u) / 256u, (uint64_t)std::max(t->num_cus, 1) * 8u);
  hipLaunchKernelGGL(tk_forget_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, t->carried, t->cap, ids, m);
  GPD_TRY(hipGetLastError());
  return GPD_OK;
}

extern "C" int gpd_tcp_tracker_reset(gpd_tcp_tracker *t, void *stream) {
  using namespace gpd;
  if (!t) return set_error(GPD_ERR_INVALID, "gpd_tcp_tracker_reset: null argument");
  if (!t->carried) return GPD_OK;
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(t->device));
  GPD_TRY(hipMemsetAsync(t->carried, 0, t->cap, (hipStream_t)stream));
  return GPD_OK;
}
