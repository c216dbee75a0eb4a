// gpd_tcpasm.hip — the stateful TCP assembler (include/gpd_tcpasm.h): tcpassembly's Assembler +
// StreamPool as a device object.  Per flow record it keeps the connection (nextSeq, lastSeen,
// pages) and its out-of-order page list with the pages' bytes, from run to run; a run assembles a
// grouped segment hand-off on top of that state, then applies FlushWithOptions and FlushAll to
// every connection held (tcpassembly/assembly.go:533-607, 235-266, 276-287).
//
// The carry is two copies (info[], node0[], nodes[], store): a run reads the current one, builds
// the other, and the two are swapped on success only.  Items are the hand-off's groups followed
// by the held connections without a group that have pages (their pages must move to the new
// carry) or that steps 2 / 3 will touch.
//
// Launches, separated by launch boundaries only (no kernel waits on another workgroup):
//
//   tam_pages_sum_kernel    per 2,048 segments: the pages they would be buffered in
//   tam_mark_kernel         a group's flow id -> its group (and the refusal of an id >= id_bound)
//   tam_select_* (3)        gpd_compact.h over the id_bound connections: the extra items, ascending
//   tam_scan_kernel         one workgroup per array: exclusive scan of block sums
//   tam_pages_apply_kernel  a segment's first page id
//   tam_isize_sum / apply   an item's region: its carried pages plus its segments' pages
//   tam_walk_kernel         one wave per item: carried pages into the region by all lanes, the
//                           state machine (gpd_tcpasm_walk.h) on lane 0, the in-order run on all
//                           64 lanes while the list is empty; records into the private region
//   tam_item_sum / apply    nine per-item counts summed (exact totals for the host) and scanned
//   -- the host decides here whether anything is written --
//   tam_place_kernel        one wave per item: records, seen_ns, stream record and the output
//                           pieces to their dense places; the connection and its remaining pages
//                           (list order) to the new carry, with one piece per page
//   gather_kernel (x2)      the shared bandwidth path (gpd_gather.h): output bytes, then the new
//                           store's bytes, each from the batch and the old store
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "gpd_compact.h"
#include "gpd_gather.h"
#include "gpd_internal.h"
#include "gpd_stream_util.h"
#include "gpd_tcpasm_walk.h"

namespace gpd {
namespace {
struct TamCarry {
  gpd_tcp_conn_info *info = nullptr;  // id_bound
  uint32_t *node0 = nullptr;          // id_bound: a connection's pages are nodes[node0, node0 + pages)
  TamCarried *nodes = nullptr;
  uint8_t *store = nullptr;
  size_t cap_nodes = 0, cap_store = 0;  // bytes
  uint64_t nconn = 0, nwith = 0, npages = 0, nbytes = 0;
};
}  // namespace
}  // namespace gpd

struct gpd_tcp_assembler {
  gpd_ctx *ctx = nullptr;
  int device = 0;
  uint32_t id_bound = 0, max_pages = 0;
  gpd::TamCarry c[2];
  int cur = 0;
  bool tables = false;
  uint8_t *sa = nullptr, *sb = nullptr;  // scratch sized before / after the first counts are known
  size_t sa_bytes = 0, sb_bytes = 0;
};

namespace gpd {
namespace {

static_assert(sizeof(gpd_tcp_conn_info) == 24 && sizeof(gpd_tcp_flush) == 16 && sizeof(TamNode) == 48 &&
                  sizeof(TamCarried) == 32 && sizeof(gpd_tcp_reasm) == 32 && sizeof(gpd_tcp_stream) == 48,
              "include/gpd_tcpasm.h layouts");

constexpr uint32_t kWalkWaves = 4;  // waves (items) per walk / place workgroup
constexpr uint32_t kStoreSrc = 0, kBatchSrc = 1;  // GatherPiece::where
using TamPiece = GatherPiece;

// per-item arrays that are summed and scanned
enum { kIRec = 0, kIBytes, kIStream, kIPages, kIPageBytes, kICalls, kIAfter, kIBefore, kIWith, kItemArrays };
// res[] words
enum { kResPages = 0, kResBad = 1, kResItem = 8, kResWords = 24 };

struct TmArgs {
  const uint8_t *data;
  uint64_t dlen;
  const uint32_t *offset;
  uint32_t n;
  const gpd_tcp_seg *segs;
  uint32_t cnt;
  const gpd_tcp_group *groups;
  uint32_t ng, nx, M;  // groups, extra items, items
  uint32_t W;           // the regions' total: the pages of the call plus the pages carried
  const uint64_t *ts;
  uint64_t now;
  gpd_tcp_flush fl;
  uint32_t id_bound, max_pages;
  // the carry read and the carry built
  const gpd_tcp_conn_info *oinfo;
  const uint32_t *onode0;
  const TamCarried *onodes;
  gpd_tcp_conn_info *ninfo;
  uint32_t *nnode0;
  TamCarried *nnodes;
  // the caller's
  gpd_tcp_reasm *recs;
  uint64_t *seen_ns;
  gpd_tcp_stream *streams;
  // scratch of the object
  uint64_t *res;
  uint32_t *pbase;  // cnt + 1: a segment's first page id
  uint32_t *blk;    // block sums of the scan in flight: (nblk + 1) words per array
  uint32_t nblk;
  uint32_t *gmark;  // id_bound: the group of a flow id, plus one
  uint64_t *mask;   // the selection's kept bits
  uint32_t *xidx;   // the extra items' flow ids, ascending
  uint32_t *ibase;  // M + 1: an item's region
  uint32_t *gsc;    // [kItemArrays][M]
  gpd_tcp_stream *sstr;      // M: the stream records before their places are known
  gpd_tcp_conn_info *iinfo;  // M: the connections afterwards
  uint32_t *ifirst;          // M: their first page's node
  TamNode *nodes;            // the items' regions
  gpd_tcp_reasm *precs;
  uint64_t *pseen;
  uint32_t *psrc;
  TamPiece *opieces, *cpieces;  // the output's and the new store's pieces
};

__device__ __forceinline__ uint64_t seg_time(const TmArgs &A, uint32_t packet) {
  return (A.ts && packet < A.n) ? A.ts[packet] : A.now;
}

// ---- sizing ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tam_pages_sum_kernel(TmArgs A) {
  scan_sum(A.cnt, A.blk, A.res + kResPages, [&A](uint32_t i) { return tsm_pages(A.segs[i].payload_len); });
}
__global__ __launch_bounds__(256) void tam_pages_apply_kernel(TmArgs A) {
  scan_apply(A.cnt, A.blk, A.pbase, true, [&A](uint32_t i) { return tsm_pages(A.segs[i].payload_len); });
}
__global__ __launch_bounds__(1024) void tam_scan_kernel(uint32_t *blk, uint32_t nblk) {
  compact_scan(blk + (size_t)blockIdx.x * (nblk + 1u), nblk);
}

__global__ __launch_bounds__(256) void tam_mark_kernel(TmArgs A) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= A.ng) return;
  const uint32_t fid = A.groups[g].flow_id;
  if (fid == GPD_TCP_UNGROUPED) return;
  if (fid >= A.id_bound) {
    A.res[kResBad] = 1;
    return;
  }
  A.gmark[fid] = g + 1u;
}

// The held connections without a group that become items.
__global__ __launch_bounds__(256) void tam_select_count_kernel(TmArgs A) {
  compact_count(A.id_bound, A.mask, A.blk, [&A](uint32_t r) {
    const gpd_tcp_conn_info ci = A.oinfo[r];
    if (!(ci.flags & GPD_TCP_CONN_OPEN) || A.gmark[r]) return false;
    return ci.pages != 0u || tam_flush_touches(ci, 0, A.fl);
  });
}
__global__ __launch_bounds__(64) void tam_select_index_kernel(TmArgs A) { compact_index(A.blk, A.mask, A.xidx, A.id_bound); }

// An item's flow id and segments (clamped to segs[]: the arrays are the caller's); false for the
// ungrouped run.
__device__ __forceinline__ bool item_of(const TmArgs &A, uint32_t i, uint32_t &fid, uint32_t &start, uint32_t &count) {
  start = count = 0;
  if (i < A.ng) {
    const gpd_tcp_group G = A.groups[i];
    fid = G.flow_id;
    start = min(G.start, A.cnt);
    count = min(G.count, A.cnt - start);
  } else {
    fid = A.xidx[i - A.ng];
  }
  return fid < A.id_bound;
}
__device__ __forceinline__ uint32_t item_size(const TmArgs &A, uint32_t i) {
  uint32_t fid, start, count;
  if (!item_of(A, i, fid, start, count)) return 0u;
  const gpd_tcp_conn_info ci = A.oinfo[fid];
  const uint32_t cp = (ci.flags & GPD_TCP_CONN_OPEN) ? ci.pages : 0u;
  return cp + (count ? A.pbase[start + count] - A.pbase[start] : 0u);
}
__global__ __launch_bounds__(256) void tam_isize_sum_kernel(TmArgs A) {
  scan_sum(A.M, A.blk, nullptr, [&A](uint32_t i) { return item_size(A, i); });
}
__global__ __launch_bounds__(256) void tam_isize_apply_kernel(TmArgs A) {
  scan_apply(A.M, A.blk, A.ibase, true, [&A](uint32_t i) { return item_size(A, i); });
}
// blockIdx.y: the array
__global__ __launch_bounds__(256) void tam_item_sum_kernel(TmArgs A) {
  const uint32_t *v = A.gsc + (size_t)blockIdx.y * A.M;
  scan_sum(A.M, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), A.res + kResItem + blockIdx.y, [v](uint32_t i) { return v[i]; });
}
__global__ __launch_bounds__(256) void tam_item_apply_kernel(TmArgs A) {
  uint32_t *v = A.gsc + (size_t)blockIdx.y * A.M;
  scan_apply(A.M, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), v, false, [v](uint32_t i) { return v[i]; });
}

// ---- the walk ---------------------------------------------------------------------------------------
// Orders the wave's own global stores before its later loads, whichever lanes issue them (the
// carried nodes written by all lanes are read by lane 0).  Workgroup scope: the lanes share a
// compute unit, so this waits for the stores and moves no cache line.
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__device__ __forceinline__ uint64_t first_lane64(uint64_t v) {
  return ((uint64_t)first_lane((uint32_t)(v >> 32)) << 32) | first_lane((uint32_t)v);
}
__device__ __forceinline__ void conn_from_lane0(TamConn &c) {
  c.exists = first_lane(c.exists);
  c.valid = first_lane(c.valid);
  c.next_seq = first_lane(c.next_seq);
  c.first = first_lane(c.first);
  c.last = first_lane(c.last);
  c.pages = first_lane(c.pages);
  c.page_bytes = first_lane(c.page_bytes);
  c.last_seen = first_lane64(c.last_seen);
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

// One wave per item.  All lanes copy the carried pages into the item's region, in list order.
// The sequential step runs on lane 0.  On top of it the wave takes gpd_tcpstream.hip's in-order
// run: with the connection open, nextSeq known and no page buffered (so never while carried pages
// wait), the following segments (up to 64) whose seq is nextSeq plus the payload bytes before
// them in the run, and that carry neither FIN nor RST, are each one call, one record, skip 0, no
// flags, the whole payload; lastSeen becomes the largest timestamp of the run.
__global__ __launch_bounds__(64 * kWalkWaves) void tam_walk_kernel(TmArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t it = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (it >= A.M) return;
  uint32_t fid, start, count;
  bool ok = item_of(A, it, fid, start, count);
  const uint32_t b0 = A.ibase[it], cap = A.ibase[it + 1u] - b0;
  if (ok && (uint64_t)b0 + cap > A.W) {  // groups that overlap or repeat a flow id: refused by the host
    if (lane == 0) A.res[kResBad] = 1;
    ok = false;
  }
  TamConn c;
  tam_conn_init(c);
  uint32_t cp = 0;
  if (ok) {
    tam_conn_load(c, A.oinfo[fid]);
    cp = min(c.pages, cap);
    const uint32_t n0 = A.onode0[fid];
    for (uint32_t j = lane; j < cp; j += 64u) A.nodes[b0 + j] = tam_node_of(A.onodes[n0 + j], j, cp);
    wave_fence();
  }
  const uint32_t before = c.exists;
  const TamIo io{A.nodes + b0, A.precs + b0, A.pseen + b0, A.psrc + b0, cap, A.max_pages, A.offset, A.n};
  if (ok) {
    const uint32_t pb0 = count ? A.pbase[start] : 0u;
    uint32_t i = 0;
    while (i < count) {
#ifndef GPD_TAM_NO_CHAIN  // (A/B: tools/tcpasm_time.py)
      if (c.exists && c.valid && c.first == kTsmNil) {
        const uint32_t j = i + lane;
        const bool in = j < count;
        gpd_tcp_seg s{};
        if (in) s = load_seg(A.segs + start + j);
        const uint32_t len = in ? s.payload_len : 0u;
        const uint32_t incl = wave_scan32(len, lane), excl = incl - len;
        const bool good = in && s.seq == c.next_seq + excl && !(s.flags & (GPD_TCP_FIN | GPD_TCP_RST)) &&
                          (len > 0u || (s.flags & GPD_TCP_SYN));
        const uint64_t m = __ballot(good);
        const uint32_t run = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
        if (run) {
          uint64_t t = lane < run ? seg_time(A, s.packet) : 0ull;
          if (lane < run && c.nrec + lane < io.cap) {
            const v4u r0{s.packet, len ? s.payload_off : 0u, len, 0u};
            const v4u r1{c.nbytes + excl, 0u, c.ncalls + lane, 0u};
            v4u *d = reinterpret_cast<v4u *>(io.recs + c.nrec + lane);
            d[0] = r0;
            d[1] = r1;
            io.seen[c.nrec + lane] = t;
            io.src[c.nrec + lane] = len ? tam_packet_base(io, s.packet) + s.payload_off : 0u;
          }
#pragma unroll
          for (uint32_t d = 32; d >= 1u; d >>= 1) {
            const uint64_t o = shfl64(t, (int)(lane ^ d));
            t = o > t ? o : t;
          }
          const uint32_t total = __shfl(incl, (int)run - 1, 64);
          if (c.last_seen < t) c.last_seen = t;
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
        tam_step(c, io, s, cp + (A.pbase[start + i] - pb0), seg_time(A, s.packet));
      }
      conn_from_lane0(c);
      ++i;
    }
    if (lane == 0) tam_flush(c, io, A.fl);
  }
  if (lane == 0) {
    const size_t M = A.M;
    const bool group = it < A.ng;
    A.gsc[kIRec * M + it] = c.nrec;
    A.gsc[kIBytes * M + it] = c.nbytes;
    A.gsc[kIStream * M + it] = ok && (group || c.ncalls || c.completed) ? 1u : 0u;
    A.gsc[kIPages * M + it] = c.exists ? c.pages : 0u;
    A.gsc[kIPageBytes * M + it] = c.exists ? c.page_bytes : 0u;
    A.gsc[kICalls * M + it] = c.ncalls;
    A.gsc[kIAfter * M + it] = c.exists;
    A.gsc[kIBefore * M + it] = before;
    A.gsc[kIWith * M + it] = (c.exists && c.pages) ? 1u : 0u;
    const gpd_tcp_conn_info ci = tam_conn_info(c);
    gpd_tcp_stream S{};
    S.flow_id = fid;
    S.nrec = c.nrec;
    S.ncalls = c.ncalls;
    S.nbytes = c.nbytes;
    S.completed = c.completed;
    S.open = ci.flags;
    S.next_seq = ci.next_seq;
    S.reserved = ci.pages;
    A.sstr[it] = S;
    A.iinfo[it] = ci;
    A.ifirst[it] = c.exists ? c.first : kTsmNil;
  }
}

// One wave per item, after the host's decision: the private records to recs[first_rec ...] with
// the stream's byte offset added, their Seen and their output pieces; the stream record; the
// connection to the new carry, its remaining pages in list order (lane 0 follows the list) with
// one new-store piece each.
__global__ __launch_bounds__(64 * kWalkWaves) void tam_place_kernel(TmArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t it = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (it >= A.M) return;
  uint32_t fid, start, count;
  if (!item_of(A, it, fid, start, count)) return;
  const size_t M = A.M;
  gpd_tcp_stream S = A.sstr[it];
  const uint32_t fr = A.gsc[kIRec * M + it], bo = A.gsc[kIBytes * M + it];
  const uint32_t b0 = A.ibase[it], cap = A.ibase[it + 1u] - b0;
  if ((uint64_t)b0 + cap > A.W) return;  // (cannot happen: the host has refused the call)
  const v4u *src = reinterpret_cast<const v4u *>(A.precs + b0);
  v4u *dst = reinterpret_cast<v4u *>(A.recs + fr);
  for (uint32_t r = lane; r < S.nrec; r += 64u) {
    const v4u a = src[2u * r];
    v4u b = src[2u * r + 1u];
    const uint32_t pos = b.x + bo;  // (output bytes < 2^32 - 16: the host has checked)
    b.x = pos;
    b.y = 0u;
    dst[2u * r] = a;
    dst[2u * r + 1u] = b;
    if (A.seen_ns) A.seen_ns[fr + r] = A.pseen[b0 + r];
    A.opieces[fr + r] = TamPiece{A.psrc[b0 + r], a.z, pos, a.x == GPD_TCP_NO_PACKET ? kStoreSrc : kBatchSrc};
  }
  if (lane != 0) return;
  if (it < A.ng || S.ncalls || S.completed) {
    S.first_rec = fr;
    S.byte_off = bo;
    const v4u *s4 = reinterpret_cast<const v4u *>(&S);
    v4u *d4 = reinterpret_cast<v4u *>(A.streams + A.gsc[kIStream * M + it]);
    d4[0] = s4[0];
    d4[1] = s4[1];
    d4[2] = s4[2];
  }
  const gpd_tcp_conn_info ci = A.iinfo[it];
  const uint32_t n0 = A.gsc[kIPages * M + it];
  A.ninfo[fid] = ci;
  A.nnode0[fid] = n0;
  uint32_t cur = A.ifirst[it], off = A.gsc[kIPageBytes * M + it];
  for (uint32_t j = 0; j < ci.pages && cur < cap; ++j) {
    const TamNode nd = A.nodes[b0 + cur];
    TamCarried p;
    p.seq = nd.seq;
    p.len = nd.len;
    p.end = nd.end;
    p.off = off;
    p.seen = nd.seen;
    p.pad = 0;
    A.nnodes[n0 + j] = p;
    const bool st = nd.packet == GPD_TCP_NO_PACKET;
    const uint32_t base = st ? 0u : (nd.packet < A.n ? A.offset[nd.packet] : 0xFFFFFFF0u);
    A.cpieces[n0 + j] = TamPiece{base + nd.off, nd.len, off, st ? kStoreSrc : kBatchSrc};
    off += nd.len;
    cur = nd.next;
  }
}

// ---- the host side ----------------------------------------------------------------------------------
// The per-connection tables of both carries, zeroed (on the first call that needs the device).
int ensure_tables(gpd_tcp_assembler *a, const char *who) {
  if (a->tables) return GPD_OK;
  const size_t nb = (size_t)std::max(a->id_bound, 1u);
  for (auto &c : a->c) {
    if (!c.info && hipMalloc(reinterpret_cast<void **>(&c.info), nb * sizeof(gpd_tcp_conn_info)) != hipSuccess)
      return set_error(GPD_ERR_NOMEM, "%s: connection table allocation failed", who);
    if (!c.node0 && hipMalloc(reinterpret_cast<void **>(&c.node0), nb * 4) != hipSuccess)
      return set_error(GPD_ERR_NOMEM, "%s: connection table allocation failed", who);
    GPD_TRY(hipMemset(c.info, 0, nb * sizeof(gpd_tcp_conn_info)));
    GPD_TRY(hipMemset(c.node0, 0, nb * 4));
  }
  a->tables = true;
  return GPD_OK;
}

}  // namespace
}  // namespace gpd

extern "C" int gpd_tcp_assembler_create(gpd_ctx *ctx, uint32_t id_bound, const gpd_tcp_asm_opts *opts,
                                        gpd_tcp_assembler **a) {
  using namespace gpd;
  if (!ctx || !a) return set_error(GPD_ERR_INVALID, "gpd_tcp_assembler_create: null argument");
  *a = nullptr;
  auto *o = new (std::nothrow) gpd_tcp_assembler();
  if (!o) return set_error(GPD_ERR_NOMEM, "gpd_tcp_assembler_create: out of memory");
  o->ctx = ctx;
  o->device = ctx_device(ctx);
  o->id_bound = id_bound;
  o->max_pages = opts ? opts->max_pages_per_connection : 0u;
  *a = o;
  return GPD_OK;
}

extern "C" void gpd_tcp_assembler_destroy(gpd_tcp_assembler *a) {
  if (!a) return;
  gpd::DeviceScope dscope_;
  if (dscope_.set(a->device) == hipSuccess) {
    for (auto &c : a->c) {
      if (c.info) (void)hipFree(c.info);
      if (c.node0) (void)hipFree(c.node0);
      if (c.nodes) (void)hipFree(c.nodes);
      if (c.store) (void)hipFree(c.store);
    }
    if (a->sa) (void)hipFree(a->sa);
    if (a->sb) (void)hipFree(a->sb);
  }
  delete a;
}

extern "C" int gpd_tcp_assembler_stats(gpd_tcp_assembler *a, uint64_t out[4]) {
  if (!a || !out) return gpd::set_error(GPD_ERR_INVALID, "gpd_tcp_assembler_stats: null argument");
  const gpd::TamCarry &C = a->c[a->cur];
  out[0] = C.nconn;
  out[1] = C.nwith;
  out[2] = C.npages;
  out[3] = C.nbytes;
  return GPD_OK;
}

extern "C" int gpd_tcp_assembler_reset(gpd_tcp_assembler *a, void *stream) {
  using namespace gpd;
  if (!a) return set_error(GPD_ERR_INVALID, "gpd_tcp_assembler_reset: null argument");
  TamCarry &C = a->c[a->cur];
  if (a->tables) {
    DeviceScope dscope_;
    GPD_TRY(dscope_.set(a->device));
    const hipStream_t s = (hipStream_t)stream;
    GPD_TRY(hipMemsetAsync(C.info, 0, (size_t)std::max(a->id_bound, 1u) * sizeof(gpd_tcp_conn_info), s));
    GPD_TRY(hipStreamSynchronize(s));
  }
  C.nconn = C.nwith = C.npages = C.nbytes = 0;
  return GPD_OK;
}

extern "C" int gpd_tcp_assembler_conns(gpd_tcp_assembler *a, gpd_tcp_conn_info *out, void *stream) {
  using namespace gpd;
  const char *who = "gpd_tcp_assembler_conns";
  if (!a || !out) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  if ((uintptr_t)out & 7u) return set_error(GPD_ERR_INVALID, "%s: out must be 8-byte aligned", who);
  if (a->id_bound == 0) return GPD_OK;
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(a->device));
  const hipStream_t s = (hipStream_t)stream;
  const size_t nb = (size_t)a->id_bound * sizeof(gpd_tcp_conn_info);
  if (a->tables)
    GPD_TRY(hipMemcpyAsync(out, a->c[a->cur].info, nb, hipMemcpyDeviceToDevice, s));
  else
    GPD_TRY(hipMemsetAsync(out, 0, nb, s));
  GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}

extern "C" int gpd_tcp_assembler_run(gpd_tcp_assembler *a, const gpd_batch *in, const gpd_tcp_seg *segs, uint64_t count,
                                     const gpd_tcp_group *groups, uint64_t ngroups, const uint64_t *ts_ns,
                                     uint64_t now_ns, const gpd_tcp_flush *fl, gpd_tcp_reasm *recs, uint64_t max_recs,
                                     uint64_t *seen_ns, gpd_tcp_stream *streams, uint64_t max_streams, uint8_t *bytes,
                                     uint64_t max_bytes, uint64_t out[8], void *stream) {
  using namespace gpd;
  const char *who = "gpd_tcp_assembler_run";
  if (!a || !out) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  const TamCarry &Old = a->c[a->cur];
  for (int k = 0; k < 8; ++k) out[k] = 0;
  out[4] = Old.nconn;
  out[5] = Old.npages;
  out[6] = Old.nbytes;
  const bool work = count != 0 && ngroups != 0;  // segments to assemble
  if (work && !in) return set_error(GPD_ERR_INVALID, "%s: null batch with segments", who);
  if (in && in->n > 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 256)", who, (unsigned long long)in->n);
  if (count >= 0x80000000ull)
    return set_error(GPD_ERR_INVALID, "%s: %llu segments (max 2^31 - 1)", who, (unsigned long long)count);
  if (ngroups > count)
    return set_error(GPD_ERR_INVALID, "%s: %llu groups of %llu segments", who, (unsigned long long)ngroups,
                     (unsigned long long)count);
  if (max_recs && !recs) return set_error(GPD_ERR_INVALID, "%s: null recs with max_recs > 0", who);
  if (max_streams && !streams) return set_error(GPD_ERR_INVALID, "%s: null streams with max_streams > 0", who);
  if (max_bytes && !bytes) return set_error(GPD_ERR_INVALID, "%s: null bytes with max_bytes > 0", who);
  if (!recs && (streams || bytes || seen_ns)) return set_error(GPD_ERR_INVALID, "%s: streams, bytes or seen_ns without recs", who);
  if (recs && (!streams || !bytes))
    return set_error(GPD_ERR_INVALID, "%s: recs without streams[] and bytes[] (there is no records-only mode)", who);
  if (((uintptr_t)recs & 15u) || ((uintptr_t)streams & 15u) || ((uintptr_t)bytes & 15u))
    return set_error(GPD_ERR_INVALID, "%s: recs, streams and bytes must be 16-byte aligned", who);
  if ((uintptr_t)seen_ns & 7u) return set_error(GPD_ERR_INVALID, "%s: seen_ns must be 8-byte aligned", who);
  if (((uintptr_t)segs & 15u) || ((uintptr_t)groups & 15u))
    return set_error(GPD_ERR_INVALID, "%s: segs and groups must be 16-byte aligned", who);
  if ((uintptr_t)ts_ns & 7u) return set_error(GPD_ERR_INVALID, "%s: ts_ns must be 8-byte aligned", who);
  if (work) {
    if (!segs || !groups) return set_error(GPD_ERR_INVALID, "%s: null segs or groups", who);
    if (!in->data || !in->offset || !in->caplen)
      return set_error(GPD_ERR_INVALID, "%s: batch data/offset/caplen must be non-NULL", who);
    if (in->data_len >= 0xFFFFFFF0ull)
      return set_error(GPD_ERR_INVALID, "%s: data_len %llu outside the 32-bit offset range", who,
                       (unsigned long long)in->data_len);
  }
  if (!work && Old.nconn == 0) return GPD_OK;  // no segment and no connection: nothing to do
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(a->device));
  if (int rc = ensure_tables(a, who)) return rc;
  const hipStream_t s = (hipStream_t)stream;
  TamCarry &New = a->c[a->cur ^ 1];
  TmArgs A{};
  if (work) {
    A.data = in->data;
    A.dlen = in->data_len;
    A.offset = in->offset;
    A.n = (uint32_t)in->n;
    A.segs = segs;
    A.cnt = (uint32_t)count;
    A.groups = groups;
    A.ng = (uint32_t)ngroups;
    A.ts = ts_ns;
  }
  A.now = now_ns;
  if (fl) A.fl = *fl;
  A.id_bound = a->id_bound;
  A.max_pages = a->max_pages;
  A.oinfo = Old.info;
  A.onode0 = Old.node0;
  A.onodes = Old.nodes;
  A.ninfo = New.info;
  A.nnode0 = New.node0;
  A.recs = recs;
  A.seen_ns = seen_ns;
  A.streams = streams;
  // ---- scratch A: what is sized by the hand-off and the table
  const uint32_t nblk_s = (A.cnt + kCompactBlock - 1u) / kCompactBlock;
  const uint32_t nblk_i = (A.id_bound + kCompactBlock - 1u) / kCompactBlock;
  const bool sel = Old.nconn != 0;
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t o = at;
    at += up16(bytes);
    return o;
  };
  const size_t o_res = take(kResWords * 8), o_pbase = take(((size_t)A.cnt + 1) * 4), o_blks = take(((size_t)nblk_s + 1) * 4);
  const size_t o_gmark = take((size_t)std::max(A.id_bound, 1u) * 4);
  const size_t o_mask = take(((size_t)nblk_i * kCompactBlock / 64u + 1) * 8), o_blkx = take(((size_t)nblk_i + 1) * 4);
  const size_t o_xidx = take((size_t)std::max(A.id_bound, 1u) * 4);
  if (!grow(&a->sa, &a->sa_bytes, at)) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.res = reinterpret_cast<uint64_t *>(a->sa + o_res);
  A.pbase = reinterpret_cast<uint32_t *>(a->sa + o_pbase);
  uint32_t *blks = reinterpret_cast<uint32_t *>(a->sa + o_blks), *blkx = reinterpret_cast<uint32_t *>(a->sa + o_blkx);
  A.gmark = reinterpret_cast<uint32_t *>(a->sa + o_gmark);
  A.mask = reinterpret_cast<uint64_t *>(a->sa + o_mask);
  A.xidx = reinterpret_cast<uint32_t *>(a->sa + o_xidx);
  GPD_TRY(hipMemsetAsync(A.res, 0, kResWords * 8, s));
  GPD_TRY(hipMemsetAsync(A.gmark, 0, (size_t)std::max(A.id_bound, 1u) * 4, s));
  if (work) {
    A.blk = blks;
    A.nblk = nblk_s;
    hipLaunchKernelGGL(tam_pages_sum_kernel, dim3(nblk_s), dim3(256), 0, s, A);
    hipLaunchKernelGGL(tam_mark_kernel, dim3((A.ng + 255u) / 256u), dim3(256), 0, s, A);
  }
  uint32_t nx = 0;
  if (sel && nblk_i) {
    A.blk = blkx;
    A.nblk = nblk_i;
    hipLaunchKernelGGL(tam_select_count_kernel, dim3(nblk_i), dim3(256), 0, s, A);
    hipLaunchKernelGGL(tam_scan_kernel, dim3(1), dim3(1024), 0, s, blkx, nblk_i);
    hipLaunchKernelGGL(tam_select_index_kernel, dim3(nblk_i), dim3(64), 0, s, A);
    GPD_TRY(hipGetLastError());
    GPD_TRY(hipMemcpyAsync(&nx, blkx + nblk_i, 4, hipMemcpyDeviceToHost, s));
  }
  GPD_TRY(hipGetLastError());
  uint64_t first[2] = {0, 0};
  GPD_TRY(hipMemcpyAsync(first, A.res, 16, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  if (first[kResBad])
    return set_error(GPD_ERR_INVALID, "%s: a group's flow_id is not below id_bound %u", who, a->id_bound);
  const uint64_t npages = first[kResPages];
  if (npages + Old.npages >= 0x80000000ull)
    return set_error(GPD_ERR_INVALID, "%s: %llu pages and %llu carried (max 2^31 - 1 in all)", who,
                     (unsigned long long)npages, (unsigned long long)Old.npages);
  if (nx > Old.nconn) nx = (uint32_t)Old.nconn;  // (cannot happen: every extra item is a held connection)
  A.nx = nx;
  A.M = A.ng + nx;
  if (A.M == 0) return GPD_OK;
  const uint32_t M = A.M;
  const size_t W = (size_t)npages + Old.npages;
  A.W = (uint32_t)W;
  const uint32_t nblk_m = (M + kCompactBlock - 1u) / kCompactBlock;
  // ---- scratch B: the items and their regions
  at = 0;
  const size_t o_ibase = take(((size_t)M + 1) * 4), o_blkm = take((size_t)(kItemArrays + 1) * (nblk_m + 1) * 4);
  const size_t o_gsc = take((size_t)kItemArrays * M * 4), o_sstr = take((size_t)M * sizeof(gpd_tcp_stream));
  const size_t o_iinfo = take((size_t)M * sizeof(gpd_tcp_conn_info)), o_ifirst = take((size_t)M * 4);
  const size_t o_nodes = take(W * sizeof(TamNode)), o_precs = take(W * sizeof(gpd_tcp_reasm));
  const size_t o_pseen = take(W * 8), o_psrc = take(W * 4);
  const size_t o_opieces = take(W * sizeof(TamPiece)), o_cpieces = take(W * sizeof(TamPiece));
  if (!grow(&a->sb, &a->sb_bytes, at)) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.ibase = reinterpret_cast<uint32_t *>(a->sb + o_ibase);
  uint32_t *blkm = reinterpret_cast<uint32_t *>(a->sb + o_blkm);
  A.gsc = reinterpret_cast<uint32_t *>(a->sb + o_gsc);
  A.sstr = reinterpret_cast<gpd_tcp_stream *>(a->sb + o_sstr);
  A.iinfo = reinterpret_cast<gpd_tcp_conn_info *>(a->sb + o_iinfo);
  A.ifirst = reinterpret_cast<uint32_t *>(a->sb + o_ifirst);
  A.nodes = reinterpret_cast<TamNode *>(a->sb + o_nodes);
  A.precs = reinterpret_cast<gpd_tcp_reasm *>(a->sb + o_precs);
  A.pseen = reinterpret_cast<uint64_t *>(a->sb + o_pseen);
  A.psrc = reinterpret_cast<uint32_t *>(a->sb + o_psrc);
  A.opieces = reinterpret_cast<TamPiece *>(a->sb + o_opieces);
  A.cpieces = reinterpret_cast<TamPiece *>(a->sb + o_cpieces);
  if (work) {
    A.blk = blks;
    A.nblk = nblk_s;
    hipLaunchKernelGGL(tam_scan_kernel, dim3(1), dim3(1024), 0, s, blks, nblk_s);
    hipLaunchKernelGGL(tam_pages_apply_kernel, dim3(nblk_s), dim3(256), 0, s, A);
  }
  A.blk = blkm + (size_t)kItemArrays * (nblk_m + 1u);
  A.nblk = nblk_m;
  hipLaunchKernelGGL(tam_isize_sum_kernel, dim3(nblk_m), dim3(256), 0, s, A);
  hipLaunchKernelGGL(tam_scan_kernel, dim3(1), dim3(1024), 0, s, A.blk, nblk_m);
  hipLaunchKernelGGL(tam_isize_apply_kernel, dim3(nblk_m), dim3(256), 0, s, A);
  const unsigned wgrid = (M + kWalkWaves - 1u) / kWalkWaves;
  hipLaunchKernelGGL(tam_walk_kernel, dim3(wgrid), dim3(64 * kWalkWaves), 0, s, A);
  A.blk = blkm;
  hipLaunchKernelGGL(tam_item_sum_kernel, dim3(nblk_m, kItemArrays), dim3(256), 0, s, A);
  hipLaunchKernelGGL(tam_scan_kernel, dim3(kItemArrays), dim3(1024), 0, s, blkm, nblk_m);
  hipLaunchKernelGGL(tam_item_apply_kernel, dim3(nblk_m, kIPageBytes + 1), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t tot[kResWords] = {};
  GPD_TRY(hipMemcpyAsync(tot, A.res, sizeof tot, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  if (tot[kResBad])
    return set_error(GPD_ERR_INVALID, "%s: groups[] overlap or repeat a flow id", who);
  const uint64_t *ti = tot + kResItem;
  const uint64_t nconn = Old.nconn + ti[kIAfter] - std::min(ti[kIBefore], Old.nconn + ti[kIAfter]);
  out[0] = ti[kIRec];
  out[1] = ti[kIStream];
  out[2] = ti[kIBytes];
  out[3] = ti[kICalls];
  out[4] = nconn;
  out[5] = ti[kIPages];
  out[6] = ti[kIPageBytes];
  if (ti[kIBytes] >= 0xFFFFFFF0ull || ti[kIPageBytes] >= 0xFFFFFFF0ull) {
    out[4] = Old.nconn, out[5] = Old.npages, out[6] = Old.nbytes;
    return set_error(GPD_ERR_INVALID, "%s: %llu output bytes, %llu carried bytes (each max 2^32 - 17)", who,
                     (unsigned long long)ti[kIBytes], (unsigned long long)ti[kIPageBytes]);
  }
  if (!recs && !max_recs) return GPD_OK;  // the sizing call
  if (ti[kIRec] > max_recs)
    return set_error(GPD_ERR_INVALID, "%s: %llu records, max_recs is %llu", who, (unsigned long long)ti[kIRec],
                     (unsigned long long)max_recs);
  if (ti[kIStream] > max_streams)
    return set_error(GPD_ERR_INVALID, "%s: %llu streams, max_streams is %llu", who, (unsigned long long)ti[kIStream],
                     (unsigned long long)max_streams);
  if (ti[kIBytes] > max_bytes)
    return set_error(GPD_ERR_INVALID, "%s: %llu bytes, max_bytes is %llu", who, (unsigned long long)ti[kIBytes],
                     (unsigned long long)max_bytes);
  // ---- the new carry, beside the old one
  if (!grow(&New.nodes, &New.cap_nodes, (size_t)ti[kIPages] * sizeof(TamCarried)) ||
      !grow(&New.store, &New.cap_store, up16((size_t)ti[kIPageBytes]) + 16))
    return set_error(GPD_ERR_NOMEM, "%s: carry allocation failed", who);
  A.nnodes = New.nodes;
  GPD_TRY(hipMemcpyAsync(New.info, Old.info, (size_t)a->id_bound * sizeof(gpd_tcp_conn_info), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(tam_place_kernel, dim3(wgrid), dim3(64 * kWalkWaves), 0, s, A);
  PieceSource G{};  // both gathers read the old store and the batch
  G.set(kStoreSrc, Old.store, Old.nbytes);
  G.set(kBatchSrc, A.data, A.dlen);
  G.pieces = A.opieces;
  launch_gather(G, (uint32_t)ti[kIRec], bytes, ti[kIBytes], s);
  G.pieces = A.cpieces;
  launch_gather(G, (uint32_t)ti[kIPages], New.store, ti[kIPageBytes], s);
  GPD_TRY(hipGetLastError());
  GPD_TRY(hipStreamSynchronize(s));
  New.nconn = nconn;
  New.nwith = ti[kIWith];
  New.npages = ti[kIPages];
  New.nbytes = ti[kIPageBytes];
  a->cur ^= 1;
  return GPD_OK;
}
