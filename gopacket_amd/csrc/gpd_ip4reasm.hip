// gpd_ip4reasm.hip — IPv4 defragmentation (include/gpd_ip4reasm.h): what
// IPv4Defragmenter.DefragIPv4WithTimestamp (ip4defrag/defrag.go:86-135) returns for every record
// of the fragment hand-off, the reassembled datagrams as a decodable device batch, and the
// unfinished fragment lists carried from batch to batch in the object's device memory.
//
// Items are the carried lists (pseudo-records 0 .. L-1) followed by the hand-off's records.
// Launches, separated by launch boundaries only (no kernel waits on another workgroup):
//
//   ir_key_kernel      one lane per item: its 10-byte key into an open-addressing table
//                      (capacity >= 2 x items).  A slot is claimed by atomicCAS with the item's
//                      index and compared through that item's key bytes, never through a hash
//                      value; atomicMin keeps the key's first item
//   ir_pair_kernel     (first item of the key, item) pairs
//   sort_hist / sort_scan / sort_scatter   the shared stable LSD radix sort of the pairs, 8 bits
//                      a pass (gpd_radix_sort.h; the last pass's sink writes order[] and skey[]):
//                      groups in order of first appearance, each in packet order, a carried list
//                      ahead of its key's records
//   ir_head / scan / index   the groups' first positions (gpd_compact.h)
//   ir_wsum / scan / wapply  a group's private node and piece region: its carried nodes plus
//                      its records bound both
//   ir_walk_kernel     one wave per group: the state machine (gpd_ip4reasm_walk.h) on lane 0,
//                      the in-order run on all 64 lanes
//   ir_rsum / scan / rapply  per record: datagrams, output bytes and pieces scanned
//   ir_gsum / scan / gapply  per group: lists, nodes and payload bytes that stay, scanned
//   ir_totals_kernel   the counts for the host, which decides here whether anything is written
//   ir_place_kernel    one lane per record: its outcome, and a completing record's datagram
//   ir_pieces_kernel   one wave per datagram: the header piece and the build's pieces to their
//                      dense places in output order
//   ir_carry_kernel    one wave per group with a list left: the new list record, its nodes and
//                      the pieces that copy their payloads into the new byte store
//   gather_kernel      the shared bandwidth path (gpd_gather.h; twice: the new store, datagram
//                      bytes): a wave per 64 consecutive pieces, 16-byte output chunks from
//                      aligned source loads shifted together, a source base per piece
//   ir_patch_kernel    one lane per datagram: total length, flags/offset, header checksum
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "gpd_compact.h"
#include "gpd_gather.h"
#include "gpd_internal.h"
#include "gpd_ip4reasm_walk.h"
#include "gpd_radix_sort.h"
#include "gpd_stream_util.h"

// One key's list between batches (48 B).
struct IprListRec {
  uint32_t src, dst, id;  // the key (src and dst as the record's four raw bytes)
  uint32_t flags;         // kLrFinal, kLrDead
  uint32_t highest, current;
  uint32_t node0, nn;     // nodes[node0, node0 + nn)
  uint64_t last_seen;
  uint32_t store0, nbytes;  // the nodes' payloads: store[store0, store0 + nbytes)
};

struct IprCarry {
  IprListRec *lists = nullptr;
  gpd::IprNode *nodes = nullptr;
  uint8_t *store = nullptr;
  size_t cap_lists = 0, cap_nodes = 0, cap_store = 0;  // bytes
  uint32_t nl = 0, nf = 0;                             // records in lists[] (dead ones included), nodes
  uint64_t nb = 0;                                     // bytes of store in use
};

struct gpd_ip4_defrag {
  gpd_ctx *ctx = nullptr;
  int device = 0;
  IprCarry c[2];
  int cur = 0;
  uint8_t *scratch = nullptr;
  size_t scratch_bytes = 0;
  uint64_t live[3] = {0, 0, 0};  // lists, fragments, bytes held (dead lists not counted)
};

namespace gpd {
namespace {

static_assert(sizeof(gpd_ip4_outcome) == 8 && sizeof(gpd_ip4_dgram) == 32 && sizeof(IprNode) == 16 &&
                  sizeof(IprPiece) == 16 && sizeof(IprListRec) == 48 && sizeof(gpd_ip4_frag) == 32,
              "include/gpd_ip4reasm.h layouts");

constexpr uint32_t kLrFinal = 1, kLrDead = 2;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kWalkWaves = 4;  // waves (groups) per walk / pieces / carry workgroup

struct RDg {  // a completing record's datagram before its place is known (16 B)
  uint32_t payload_len, nfrags;
  uint32_t length_flags;  // Highest | flags << 16
  uint32_t piece0;        // its pieces: ppieces[piece0, piece0 + rsc[2][r] - 1)
};
struct GEnd {  // a group's list after the walk (24 B)
  uint32_t highest, current, final_received, pad;
  uint64_t last_seen;
};

// res[] words
enum { kResDgrams = 0, kResBytes, kResPieces, kResLists, kResNodes, kResStore, kResBad, kResWords = 8 };

struct IrArgs {
  const uint8_t *data;
  uint64_t dlen;
  const uint32_t *offset;
  uint32_t n;
  const gpd_ip4_frag *frags;
  uint32_t cnt;
  const uint64_t *ts;
  uint64_t now;
  // the carry read and the carry built
  const IprListRec *ol;
  const IprNode *on;
  uint32_t L, M;  // carried lists; items = L + cnt
  IprListRec *nl;
  IprNode *nn;
  // the caller's
  gpd_ip4_outcome *outcomes;
  gpd_ip4_dgram *dgrams;
  uint32_t *out_offset, *out_caplen;
  uint8_t *bytes;
  uint32_t ndg;
  // scratch of the object
  uint64_t *res;
  uint32_t *tab, tmask;
  uint32_t *slot;         // M
  uint2 *pa;              // M: the (first item of the key, item) pairs the sort takes
  uint32_t *order, *skey; // M: the items sorted, their keys (first item; M: none)
  uint64_t *mask;
  uint32_t *blk, nblk;    // block sums of the scan in flight: (nblk + 1) words per array
  uint32_t *heads, ng;    // a group's first sorted position
  uint32_t *wbase;        // M + 1: where a sorted position's nodes start
  IprNode *pnodes;        // the groups' private node regions
  IprPiece *ppieces;      // ... and piece regions
  uint32_t *rwhat;        // cnt
  uint32_t *rsc;          // [3][cnt]: datagrams, bytes, pieces per record -> their exclusive scans
  RDg *rdg;               // cnt
  uint32_t *dgrec;        // datagram -> its completing record
  GEnd *gend;             // per group
  uint32_t *gsc;          // [3][M]: lists, nodes, payload bytes that stay per group -> scans
  IprPiece *dpieces;      // the datagrams' pieces, dense, in output order
  IprPiece *cpieces;      // the new store's pieces
};

// ---- keys and the table ------------------------------------------------------------------------
struct Key {
  uint32_t src, dst, id;
};
__device__ __forceinline__ uint32_t le32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ gpd_ip4_frag load_frag(const gpd_ip4_frag *p) {
  gpd_ip4_frag f;
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  uint4 *d = reinterpret_cast<uint4 *>(&f);
  d[0] = q[0];
  d[1] = q[1];
  return f;
}
__device__ __forceinline__ Key item_key(const IrArgs &A, uint32_t i) {
  if (i < A.L) return Key{A.ol[i].src, A.ol[i].dst, A.ol[i].id};
  const gpd_ip4_frag f = load_frag(A.frags + (i - A.L));
  return Key{le32(f.src), le32(f.dst), f.id};
}
__device__ __forceinline__ uint32_t key_mix(const Key &k) {
  uint32_t h = k.src * 0x9E3779B1u;
  h = (h ^ (h >> 15)) + k.dst * 0x85EBCA77u;
  h = (h ^ (h >> 13)) + k.id * 0xC2B2AE3Du;
  return h ^ (h >> 16);
}

__global__ __launch_bounds__(256) void ir_key_kernel(IrArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.M) return;
  bool valid;
  if (i < A.L) {
    valid = !(A.ol[i].flags & kLrDead);
  } else {
    const uint32_t r = i - A.L;
    const uint32_t pk = A.frags[r].packet;
    valid = A.frags[r].verdict == GPD_FRAG_INSERT;
    // the hand-off is in packet order: anything else is not gpd_ip4_fragments' output
    if (pk >= A.n || (r > 0 && A.frags[r - 1].packet >= pk)) A.res[kResBad] = 1;
  }
  uint32_t h = kNone;
  if (valid) {
    const Key k = item_key(A, i);
    h = key_mix(k) & A.tmask;
    for (;;) {  // (at most half the slots are ever taken: an empty one ends every probe)
      const uint32_t cur = atomicCAS(&A.tab[h], kNone, i);
      if (cur == kNone) break;
      const Key c = item_key(A, cur);  // cur: some item of the slot's key (only the minimum moves)
      if (c.src == k.src && c.dst == k.dst && c.id == k.id) {
        atomicMin(&A.tab[h], i);
        break;
      }
      h = (h + 1u) & A.tmask;
    }
  }
  A.slot[i] = h;
}

__global__ __launch_bounds__(256) void ir_pair_kernel(IrArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.M) return;
  const uint32_t h = A.slot[i];
  A.pa[i] = make_uint2(h == kNone ? A.M : A.tab[h], i);
}

// ---- the sort of the (key, item) pairs (gpd_radix_sort.h): where its last pass puts them ----------
struct OrderSink {
  uint32_t *order, *skey;
  __device__ __forceinline__ void operator()(uint32_t pos, uint2 p) const {
    order[pos] = p.y;
    skey[pos] = p.x;
  }
};

// ---- groups and their private regions -----------------------------------------------------------
__global__ __launch_bounds__(256) void ir_head_kernel(IrArgs A) {
  compact_count(A.M, A.mask, A.blk, [&A](uint32_t i) { return i == 0 || A.skey[i] != A.skey[i - 1]; });
}
__global__ __launch_bounds__(1024) void ir_scan_kernel(IrArgs A) {
  compact_scan(A.blk + (size_t)blockIdx.x * (A.nblk + 1u), A.nblk);
}
__global__ __launch_bounds__(64) void ir_index_kernel(IrArgs A) { compact_index(A.blk, A.mask, A.heads, A.M); }

__device__ __forceinline__ uint32_t pos_weight(const IrArgs &A, uint32_t p) {
  if (A.skey[p] >= A.M) return 0u;
  const uint32_t it = A.order[p];
  return it < A.L ? A.ol[it].nn : 1u;
}
__global__ __launch_bounds__(256) void ir_wsum_kernel(IrArgs A) {
  scan_sum(A.M, A.blk, nullptr, [&A](uint32_t p) { return pos_weight(A, p); });
}
__global__ __launch_bounds__(256) void ir_wapply_kernel(IrArgs A) {
  scan_apply(A.M, A.blk, A.wbase, true, [&A](uint32_t p) { return pos_weight(A, p); });
}

// ---- the walk ---------------------------------------------------------------------------------
__device__ __forceinline__ IprNode frag_node(const IrArgs &A, const gpd_ip4_frag &f) {
  uint64_t s = 0xFFFFFFFFull;
  if (f.packet < A.n) s = (uint64_t)A.offset[f.packet] + f.net_off + 4u * f.ihl;
  return IprNode{s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s, f.payload_len, f.frag_offset, f.length, kIprBatch};
}
__device__ __forceinline__ uint64_t frag_time(const IrArgs &A, const gpd_ip4_frag &f) {
  return A.ts && f.packet < A.n ? A.ts[f.packet] : A.now;
}

// Orders the wave's own global stores before its later loads, whichever lanes issue them (nodes
// written by all lanes are read by lane 0 and the other way round).  Workgroup scope: the lanes
// share a compute unit, so this waits for the stores and moves no cache line.
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// One wave per group.  The sequential step runs on lane 0.  On top of it the wave takes the
// in-order run: the following records (up to 64) whose FragOffset*8 is Highest plus the
// Length-20 of the run's earlier records, while that sum stays within 65535 and the list under
// its length limit, are each a PushBack with Highest and Current advanced.  The run ends at the
// first record that breaks the chain and at the first at which FinalReceived && Highest ==
// Current would hold: that one takes the step, which builds.
__global__ __launch_bounds__(64 * kWalkWaves) void ir_walk_kernel(IrArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (g >= A.ng) return;
  const uint32_t p0 = A.heads[g], p1 = g + 1u < A.ng ? A.heads[g + 1u] : A.M;
  if (A.skey[p0] >= A.M) {  // the items that join no group
    if (lane == 0) A.gsc[g] = A.gsc[(size_t)A.M + g] = A.gsc[2 * (size_t)A.M + g] = 0u;
    return;
  }
  const uint32_t nb = A.wbase[p0];
  IprNode *nodes = A.pnodes + nb;
  IprPiece *pieces = A.ppieces + nb;
  IprList Ls;
  ipr_list_init(Ls);
  uint32_t ppos = 0, i = p0;
  const uint32_t it0 = A.order[p0];
  if (it0 < A.L) {  // the carried list
    const IprListRec R = A.ol[it0];
    for (uint32_t j = lane; j < R.nn; j += 64u) nodes[j] = A.on[R.node0 + j];
    Ls.nn = R.nn;
    Ls.highest = R.highest;
    Ls.current = R.current;
    Ls.final_received = R.flags & kLrFinal;
    Ls.last_seen = R.last_seen;
    ++i;
    wave_fence();  // lane 0 reads what the other lanes stored
  }
  while (i < p1) {
#ifndef GPD_IP4R_NO_RUN  // (A/B: tools/ip4reasm_time.py)
    {
      const uint32_t j = i + lane;
      const uint32_t it = j < p1 ? A.order[j] : 0u;
      const bool in = j < p1 && it >= A.L;  // (only a group's first item can be a carried list)
      gpd_ip4_frag f{};
      uint32_t r = 0;
      if (in) {
        r = it - A.L;
        f = load_frag(A.frags + r);
      }
      const uint32_t fl = in ? ipr_frag_length(f.length) : 0u;
      const uint32_t incl = wave_scan32(fl, lane), excl = incl - fl;
      const uint64_t below = lane == 63u ? ~0ull : (2ull << lane) - 1ull;  // lanes 0 .. lane
      const uint64_t fin = __ballot(in && !(f.flags & 1u));
      const bool finl = Ls.final_received || (fin & below) != 0ull;
      const uint32_t h_after = Ls.highest + incl;
      const bool ok = in && (uint32_t)f.frag_offset * 8u == Ls.highest + excl && h_after <= 65535u &&
                      !(finl && h_after == ((Ls.current + incl) & 0xFFFFu)) &&
                      Ls.nn + lane + 2u <= GPD_IP4_MAX_LIST_LEN;
      const uint64_t m = __ballot(ok);
      const uint32_t run = m == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~m);
      if (run) {
        if (lane < run) {
          nodes[Ls.nn + lane] = frag_node(A, f);
          A.rwhat[r] = GPD_IP4_FILED;
        }
        const uint32_t total = __shfl(incl, (int)run - 1, 64);
        Ls.highest += total;
        Ls.current = (Ls.current + total) & 0xFFFFu;
        const uint64_t runm = run == 64u ? ~0ull : (1ull << run) - 1ull;
        if (fin & runm) Ls.final_received = 1u;
        Ls.nn += run;
        Ls.last_seen = shfl64(frag_time(A, f), (int)run - 1);
        i += run;
        wave_fence();
        continue;
      }
    }
#endif
    if (lane == 0 && A.order[i] >= A.L) {
      const uint32_t r = A.order[i] - A.L;
      const gpd_ip4_frag f = load_frag(A.frags + r);
      IprBuilt B;
      const uint32_t what = ipr_step(Ls, nodes, frag_node(A, f), (f.flags & 1u) != 0u, frag_time(A, f), pieces + ppos, B);
      A.rwhat[r] = what;
      if (what == GPD_IP4_COMPLETE) {
        A.rdg[r] = RDg{B.payload_len, B.nfrags, B.length | (B.flags << 16), nb + ppos};
        A.rsc[r] = 1u;
        A.rsc[(size_t)A.cnt + r] = 4u * f.ihl + B.payload_len;
        A.rsc[2 * (size_t)A.cnt + r] = B.npieces + 1u;
        ppos += B.npieces;
      }
    }
    Ls.nn = first_lane(Ls.nn);
    Ls.highest = first_lane(Ls.highest);
    Ls.current = first_lane(Ls.current);
    Ls.final_received = first_lane(Ls.final_received);
    Ls.last_seen = ((uint64_t)first_lane((uint32_t)(Ls.last_seen >> 32)) << 32) | first_lane((uint32_t)Ls.last_seen);
    ppos = first_lane(ppos);
    ++i;
  }
  wave_fence();
  uint32_t nbytes = 0;  // the payload bytes the list holds
  for (uint32_t j = lane; j < Ls.nn; j += 64u) nbytes += nodes[j].payload_len;
#pragma unroll
  for (uint32_t d = 32; d >= 1u; d >>= 1) nbytes += __shfl_xor(nbytes, d, 64);
  if (lane == 0) {
    A.gsc[g] = Ls.nn ? 1u : 0u;
    A.gsc[(size_t)A.M + g] = Ls.nn;
    A.gsc[2 * (size_t)A.M + g] = nbytes;
    A.gend[g] = GEnd{Ls.highest, Ls.current, Ls.final_received, 0u, Ls.last_seen};
  }
}

// ---- totals ---------------------------------------------------------------------------------------
// blockIdx.y: the array.  The byte arrays (index 1 of the records, 2 of the groups) also leave
// their exact 64-bit sums.
__global__ __launch_bounds__(256) void ir_rsum_kernel(IrArgs A) {
  const uint32_t *v = A.rsc + (size_t)blockIdx.y * A.cnt;
  scan_sum(A.cnt, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), blockIdx.y == 1u ? A.res + kResBytes : nullptr,
           [v](uint32_t i) { return v[i]; });
}
__global__ __launch_bounds__(256) void ir_rapply_kernel(IrArgs A) {
  uint32_t *v = A.rsc + (size_t)blockIdx.y * A.cnt;
  scan_apply(A.cnt, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), v, false, [v](uint32_t i) { return v[i]; });
}
__global__ __launch_bounds__(64) void ir_rtotals_kernel(IrArgs A) {
  if (threadIdx.x != 0) return;
  A.res[kResDgrams] = A.blk[A.nblk];
  A.res[kResPieces] = A.blk[2 * (size_t)(A.nblk + 1u) + A.nblk];
}
__global__ __launch_bounds__(256) void ir_gsum_kernel(IrArgs A) {
  const uint32_t *v = A.gsc + (size_t)blockIdx.y * A.M;
  scan_sum(A.ng, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), blockIdx.y == 2u ? A.res + kResStore : nullptr,
           [v](uint32_t i) { return v[i]; });
}
__global__ __launch_bounds__(256) void ir_gapply_kernel(IrArgs A) {
  uint32_t *v = A.gsc + (size_t)blockIdx.y * A.M;
  scan_apply(A.ng, A.blk + (size_t)blockIdx.y * (A.nblk + 1u), v, false, [v](uint32_t i) { return v[i]; });
}
__global__ __launch_bounds__(64) void ir_gtotals_kernel(IrArgs A) {
  if (threadIdx.x != 0) return;
  A.res[kResLists] = A.blk[A.nblk];
  A.res[kResNodes] = A.blk[(size_t)(A.nblk + 1u) + A.nblk];
}

// ---- place ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ir_place_kernel(IrArgs A) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= A.cnt) return;
  const gpd_ip4_frag f = load_frag(A.frags + r);
  uint32_t what, k = 0;
  if (f.verdict == GPD_FRAG_INSERT) what = A.rwhat[r];
  else what = f.verdict == GPD_FRAG_WHOLE ? GPD_IP4_UNCHANGED : GPD_IP4_REJECTED;
  if (what == GPD_IP4_COMPLETE) {
    k = A.rsc[r];
    const RDg D = A.rdg[r];
    const uint32_t bo = A.rsc[(size_t)A.cnt + r];
    const uint64_t hdr = (uint64_t)A.offset[f.packet] + f.net_off;  // (packet < n: ir_key_kernel)
    const uint32_t proto = hdr + 9u < A.dlen ? A.data[hdr + 9u] : 0u;
    const v4u d0{f.packet, r, bo, 0u};
    const v4u d1{D.payload_len, D.nfrags, (D.length_flags & 0xFFFFu) | ((uint32_t)f.id << 16),
                 (uint32_t)f.ihl | (proto << 8) | ((D.length_flags >> 16) << 16)};
    v4u *d = reinterpret_cast<v4u *>(A.dgrams + k);
    d[0] = d0;
    d[1] = d1;
    A.dgrec[k] = r;
    if (A.out_offset) A.out_offset[k] = bo;
    if (A.out_caplen) A.out_caplen[k] = 4u * f.ihl + D.payload_len;
  }
  A.outcomes[r] = gpd_ip4_outcome{what, k};
}

// One wave per datagram: its header piece, then the build's pieces at their output positions.
__global__ __launch_bounds__(64 * kWalkWaves) void ir_pieces_kernel(IrArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (k >= A.ndg) return;
  const uint32_t r = A.dgrec[k];
  const gpd_ip4_frag f = load_frag(A.frags + r);
  const RDg D = A.rdg[r];
  const uint32_t bo = A.rsc[(size_t)A.cnt + r], base = A.rsc[2 * (size_t)A.cnt + r];
  const uint32_t np = (k + 1u < A.ndg ? A.rsc[2 * (size_t)A.cnt + A.dgrec[k + 1u]] : (uint32_t)A.res[kResPieces]) - base;
  const uint32_t hl = 4u * f.ihl;
  if (lane == 0) {
    const uint64_t hdr = (uint64_t)A.offset[f.packet] + f.net_off;
    A.dpieces[base] = IprPiece{hdr > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)hdr, hl, bo, kIprBatch};
  }
  for (uint32_t j = lane; j + 1u < np; j += 64u) {
    IprPiece P = A.ppieces[D.piece0 + j];
    P.pos += bo + hl;
    A.dpieces[base + 1u + j] = P;
  }
}

// One wave per group that keeps a list: its record, its nodes with their places in the new
// store, and the pieces that copy their payloads there.
__global__ __launch_bounds__(64 * kWalkWaves) void ir_carry_kernel(IrArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * kWalkWaves + (threadIdx.x >> 6);
  if (g >= A.ng) return;
  const uint32_t p0 = A.heads[g];
  if (A.skey[p0] >= A.M) return;
  const uint32_t li = A.gsc[g], n0 = A.gsc[(size_t)A.M + g], b0 = A.gsc[2 * (size_t)A.M + g];
  const uint32_t li_next = g + 1u < A.ng ? A.gsc[g + 1u] : (uint32_t)A.res[kResLists];
  if (li_next == li) return;  // no list left
  const uint32_t n_next = g + 1u < A.ng ? A.gsc[(size_t)A.M + g + 1u] : (uint32_t)A.res[kResNodes];
  const uint32_t nn = n_next - n0;
  const IprNode *nodes = A.pnodes + A.wbase[p0];
  uint32_t run = 0;
  for (uint32_t j0 = 0; j0 < nn; j0 += 64u) {
    const uint32_t j = j0 + lane;
    IprNode e{};
    if (j < nn) e = nodes[j];
    const uint32_t incl = wave_scan32(e.payload_len, lane);
    if (j < nn) {
      const uint32_t at = b0 + run + incl - e.payload_len;
      A.cpieces[n0 + j] = IprPiece{e.src, e.payload_len, at, e.where};
      e.src = at;
      e.where = kIprStore;
      A.nn[n0 + j] = e;
    }
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) {
    const Key k = item_key(A, A.order[p0]);
    const GEnd E = A.gend[g];
    A.nl[li] = IprListRec{k.src, k.dst, k.id, E.final_received ? kLrFinal : 0u, E.highest, E.current, n0, nn,
                          E.last_seen, b0, run};
  }
}

// One lane per datagram: the three header patches of include/gpd_ip4reasm.h.
__global__ __launch_bounds__(256) void ir_patch_kernel(IrArgs A, uint64_t nbytes) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= A.ndg) return;
  const gpd_ip4_dgram D = A.dgrams[k];
  const uint32_t hl = 4u * D.ihl;
  if (hl < 20u || D.byte_off + hl > nbytes) return;  // (no IPv4 layer decodes with IHL < 5)
  uint8_t *h = A.bytes + D.byte_off;
  const uint64_t total = (uint64_t)hl + D.payload_len;
  const uint32_t tl = total <= 65535ull ? (uint32_t)total : 0u;
  h[2] = (uint8_t)(tl >> 8);
  h[3] = (uint8_t)tl;
  h[6] = h[7] = 0;
  h[10] = h[11] = 0;
  uint32_t sum = 0;
  for (uint32_t b = 0; b < hl; b += 2u) sum += ((uint32_t)h[b] << 8) | h[b + 1u];
  sum = (sum & 0xFFFFu) + (sum >> 16);
  sum = (sum & 0xFFFFu) + (sum >> 16);
  const uint32_t cs = ~sum & 0xFFFFu;
  h[10] = (uint8_t)(cs >> 8);
  h[11] = (uint8_t)cs;
}

// ---- DiscardOlderThan -----------------------------------------------------------------------------
// res[0..2] += the lists, fragments and bytes dropped.
__global__ __launch_bounds__(256) void ir_discard_kernel(IprListRec *lists, uint32_t nl, uint64_t t, uint64_t *res) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nl) return;
  IprListRec R = lists[i];
  if ((R.flags & kLrDead) || R.last_seen >= t) return;
  lists[i].flags = R.flags | kLrDead;
  atomicAdd(reinterpret_cast<unsigned long long *>(res), 1ull);
  atomicAdd(reinterpret_cast<unsigned long long *>(res + 1), (unsigned long long)R.nn);
  atomicAdd(reinterpret_cast<unsigned long long *>(res + 2), (unsigned long long)R.nbytes);
}

}  // namespace
}  // namespace gpd

extern "C" int gpd_ip4_defrag_create(gpd_ctx *ctx, gpd_ip4_defrag **d) {
  using namespace gpd;
  if (!ctx || !d) return set_error(GPD_ERR_INVALID, "gpd_ip4_defrag_create: null argument");
  *d = nullptr;
  auto *o = new (std::nothrow) gpd_ip4_defrag();
  if (!o) return set_error(GPD_ERR_NOMEM, "gpd_ip4_defrag_create: out of memory");
  o->ctx = ctx;
  o->device = ctx_device(ctx);
  *d = o;
  return GPD_OK;
}

extern "C" void gpd_ip4_defrag_destroy(gpd_ip4_defrag *d) {
  if (!d) return;
  gpd::DeviceScope dscope_;
  if (dscope_.set(d->device) == hipSuccess) {
    for (auto &c : d->c) {
      if (c.lists) (void)hipFree(c.lists);
      if (c.nodes) (void)hipFree(c.nodes);
      if (c.store) (void)hipFree(c.store);
    }
    if (d->scratch) (void)hipFree(d->scratch);
  }
  delete d;
}

extern "C" int gpd_ip4_defrag_stats(gpd_ip4_defrag *d, uint64_t out[3]) {
  if (!d || !out) return gpd::set_error(GPD_ERR_INVALID, "gpd_ip4_defrag_stats: null argument");
  out[0] = d->live[0];
  out[1] = d->live[1];
  out[2] = d->live[2];
  return GPD_OK;
}

extern "C" int gpd_ip4_defrag_discard(gpd_ip4_defrag *d, uint64_t t_ns, uint64_t *n) {
  using namespace gpd;
  const char *who = "gpd_ip4_defrag_discard";
  if (!d || !n) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *n = 0;
  IprCarry &C = d->c[d->cur];
  if (C.nl == 0) return GPD_OK;
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(d->device));
  if (!grow(&d->scratch, &d->scratch_bytes, 64)) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  uint64_t *res = reinterpret_cast<uint64_t *>(d->scratch);
  GPD_TRY(hipMemsetAsync(res, 0, 64, nullptr));
  hipLaunchKernelGGL(ir_discard_kernel, dim3((C.nl + 255u) / 256u), dim3(256), 0, nullptr, C.lists, C.nl, t_ns, res);
  GPD_TRY(hipGetLastError());
  uint64_t got[3] = {0, 0, 0};
  GPD_TRY(hipMemcpy(got, res, 24, hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) d->live[k] -= std::min(got[k], d->live[k]);
  *n = got[0];
  return GPD_OK;
}

extern "C" int gpd_ip4_defrag_run(gpd_ip4_defrag *d, const gpd_batch *in, const gpd_ip4_frag *frags, uint64_t count,
                                  const uint64_t *ts_ns, uint64_t now_ns, gpd_ip4_outcome *outcomes,
                                  gpd_ip4_dgram *dgrams, uint64_t max_dgrams, uint32_t *offset, uint32_t *caplen,
                                  uint8_t *bytes, uint64_t max_bytes, uint64_t out[4], void *stream) {
  using namespace gpd;
  const char *who = "gpd_ip4_defrag_run";
  if (!d || !in || !out) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  out[0] = out[1] = out[2] = 0;
  out[3] = d->live[0];
  if (in->n > 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 256)", who, (unsigned long long)in->n);
  if (count > in->n)
    return set_error(GPD_ERR_INVALID, "%s: %llu records for %llu packets", who, (unsigned long long)count,
                     (unsigned long long)in->n);
  const IprCarry &Old = d->c[d->cur];
  if (count + Old.nl + Old.nf >= 0x80000000ull)
    return set_error(GPD_ERR_INVALID, "%s: %llu records and %u carried fragments (max 2^31 - 1 in all)", who,
                     (unsigned long long)count, Old.nf);
  if (max_dgrams && !dgrams) return set_error(GPD_ERR_INVALID, "%s: null dgrams with max_dgrams > 0", who);
  if (max_bytes && !bytes) return set_error(GPD_ERR_INVALID, "%s: null bytes with max_bytes > 0", who);
  if (bytes && !dgrams) return set_error(GPD_ERR_INVALID, "%s: bytes without dgrams", who);
  if (dgrams && count && !outcomes) return set_error(GPD_ERR_INVALID, "%s: dgrams without outcomes[]", who);
  if (bytes && (!offset || !caplen)) return set_error(GPD_ERR_INVALID, "%s: bytes without offset[] and caplen[]", who);
  if (((uintptr_t)outcomes & 15u) || ((uintptr_t)dgrams & 15u) || ((uintptr_t)bytes & 15u) ||
      ((uintptr_t)offset & 15u) || ((uintptr_t)caplen & 15u))
    return set_error(GPD_ERR_INVALID, "%s: outcomes, dgrams, offset, caplen and bytes must be 16-byte aligned", who);
  if ((uintptr_t)frags & 15u) return set_error(GPD_ERR_INVALID, "%s: frags must be 16-byte aligned", who);
  if (count == 0) return GPD_OK;  // no call is made: the lists stay as they are
  if (!frags) return set_error(GPD_ERR_INVALID, "%s: null frags", who);
  if (!in->data || !in->offset || !in->caplen)
    return set_error(GPD_ERR_INVALID, "%s: batch data/offset/caplen must be non-NULL", who);
  if (in->data_len >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: data_len %llu outside the 32-bit offset range", who,
                     (unsigned long long)in->data_len);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(d->device));
  const hipStream_t s = (hipStream_t)stream;
  IprCarry &New = d->c[d->cur ^ 1];
  IrArgs A{};
  A.data = in->data;
  A.dlen = in->data_len;
  A.offset = in->offset;
  A.n = (uint32_t)in->n;
  A.frags = frags;
  A.cnt = (uint32_t)count;
  A.ts = ts_ns;
  A.now = now_ns;
  A.ol = Old.lists;
  A.on = Old.nodes;
  A.L = Old.nl;
  A.M = A.L + A.cnt;
  A.outcomes = outcomes;
  A.dgrams = dgrams;
  A.out_offset = offset;
  A.out_caplen = caplen;
  A.bytes = bytes;
  const uint32_t M = A.M, cnt = A.cnt;
  const size_t W = (size_t)Old.nf + cnt;  // bound of the nodes, and of the pieces, of all groups
  uint32_t tcap = 64;
  while (tcap < 2ull * M) tcap <<= 1;
  A.tmask = tcap - 1u;
  const uint32_t ntile = (M + kSortTile - 1u) / kSortTile;
  const uint32_t nblk_m = (M + kCompactBlock - 1u) / kCompactBlock, nblk_r = (cnt + kCompactBlock - 1u) / kCompactBlock;
  // the scratch, carved in one piece
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t a = at;
    at += up16(bytes);
    return a;
  };
  const size_t o_res = take(kResWords * 8), o_tab = take((size_t)tcap * 4), o_slot = take((size_t)M * 4);
  const size_t o_pa = take((size_t)M * 8), o_pb = take((size_t)M * 8), o_hist = take((size_t)ntile * 256 * 4);
  const size_t o_order = take((size_t)M * 4), o_skey = take((size_t)M * 4), o_mask = take(((size_t)M + 63) / 64 * 8);
  const size_t o_blk = take(3 * ((size_t)nblk_m + 1) * 4), o_heads = take((size_t)M * 4);
  const size_t o_wbase = take(((size_t)M + 1) * 4), o_pnodes = take(W * sizeof(IprNode));
  const size_t o_ppieces = take(W * sizeof(IprPiece)), o_rwhat = take((size_t)cnt * 4), o_rsc = take(3 * (size_t)cnt * 4);
  const size_t o_rdg = take((size_t)cnt * sizeof(RDg)), o_dgrec = take((size_t)cnt * 4);
  const size_t o_gend = take((size_t)M * sizeof(GEnd)), o_gsc = take(3 * (size_t)M * 4);
  const size_t o_dpieces = take((W + cnt) * sizeof(IprPiece)), o_cpieces = take(W * sizeof(IprPiece));
  if (!grow(&d->scratch, &d->scratch_bytes, at)) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  uint8_t *sb = d->scratch;
  A.res = reinterpret_cast<uint64_t *>(sb + o_res);
  A.tab = reinterpret_cast<uint32_t *>(sb + o_tab);
  A.slot = reinterpret_cast<uint32_t *>(sb + o_slot);
  A.pa = reinterpret_cast<uint2 *>(sb + o_pa);
  uint2 *pb = reinterpret_cast<uint2 *>(sb + o_pb);
  const SortArgs S{M, ntile, reinterpret_cast<uint32_t *>(sb + o_hist)};
  A.order = reinterpret_cast<uint32_t *>(sb + o_order);
  A.skey = reinterpret_cast<uint32_t *>(sb + o_skey);
  A.mask = reinterpret_cast<uint64_t *>(sb + o_mask);
  A.blk = reinterpret_cast<uint32_t *>(sb + o_blk);
  A.heads = reinterpret_cast<uint32_t *>(sb + o_heads);
  A.wbase = reinterpret_cast<uint32_t *>(sb + o_wbase);
  A.pnodes = reinterpret_cast<IprNode *>(sb + o_pnodes);
  A.ppieces = reinterpret_cast<IprPiece *>(sb + o_ppieces);
  A.rwhat = reinterpret_cast<uint32_t *>(sb + o_rwhat);
  A.rsc = reinterpret_cast<uint32_t *>(sb + o_rsc);
  A.rdg = reinterpret_cast<RDg *>(sb + o_rdg);
  A.dgrec = reinterpret_cast<uint32_t *>(sb + o_dgrec);
  A.gend = reinterpret_cast<GEnd *>(sb + o_gend);
  A.gsc = reinterpret_cast<uint32_t *>(sb + o_gsc);
  A.dpieces = reinterpret_cast<IprPiece *>(sb + o_dpieces);
  A.cpieces = reinterpret_cast<IprPiece *>(sb + o_cpieces);

  // group: keys, first items, the sort, the heads
  GPD_TRY(hipMemsetAsync(A.res, 0, kResWords * 8, s));
  GPD_TRY(hipMemsetAsync(A.tab, 0xFF, (size_t)tcap * 4, s));
  GPD_TRY(hipMemsetAsync(A.rsc, 0, 3 * (size_t)cnt * 4, s));
  const unsigned igrid = (M + 255u) / 256u;
  hipLaunchKernelGGL(ir_key_kernel, dim3(igrid), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ir_pair_kernel, dim3(igrid), dim3(256), 0, s, A);
  const uint32_t passes = sort_passes(M);  // keys lie in [0, M]; M: no key
  sort_last_pass(S, sort_leading_passes(S, A.pa, pb, passes, s), passes, OrderSink{A.order, A.skey}, s);
  A.nblk = nblk_m;
  hipLaunchKernelGGL(ir_head_kernel, dim3(nblk_m), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ir_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(ir_index_kernel, dim3(nblk_m), dim3(64), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint32_t ng = 0;
  uint64_t bad = 0;
  GPD_TRY(hipMemcpyAsync(&ng, A.blk + nblk_m, 4, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipMemcpyAsync(&bad, A.res + kResBad, 8, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  if (bad)
    return set_error(GPD_ERR_INVALID, "%s: frags[] is not a complete hand-off of this batch (packets out of order "
                     "or outside it)", who);
  A.ng = ng;
  // regions, the walk, the totals
  hipLaunchKernelGGL(ir_wsum_kernel, dim3(nblk_m), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ir_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(ir_wapply_kernel, dim3(nblk_m), dim3(256), 0, s, A);
  const unsigned wgrid = (ng + kWalkWaves - 1u) / kWalkWaves;
  hipLaunchKernelGGL(ir_walk_kernel, dim3(wgrid), dim3(64 * kWalkWaves), 0, s, A);
  A.nblk = nblk_r;
  hipLaunchKernelGGL(ir_rsum_kernel, dim3(nblk_r, 3), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ir_scan_kernel, dim3(3), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(ir_rapply_kernel, dim3(nblk_r, 3), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ir_rtotals_kernel, dim3(1), dim3(64), 0, s, A);
  const uint32_t nblk_g = (ng + kCompactBlock - 1u) / kCompactBlock;
  A.nblk = nblk_g;
  hipLaunchKernelGGL(ir_gsum_kernel, dim3(nblk_g, 3), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ir_scan_kernel, dim3(3), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(ir_gapply_kernel, dim3(nblk_g, 3), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ir_gtotals_kernel, dim3(1), dim3(64), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t tot[kResWords] = {};
  GPD_TRY(hipMemcpyAsync(tot, A.res, sizeof tot, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  out[0] = tot[kResDgrams];
  out[2] = tot[kResBytes];
  out[3] = tot[kResLists];
  if (tot[kResBytes] >= 0xFFFFFFF0ull || tot[kResStore] >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: %llu output bytes, %llu carried bytes (max 2^32 - 17 each)", who,
                     (unsigned long long)tot[kResBytes], (unsigned long long)tot[kResStore]);
  if (!dgrams && !max_dgrams) {  // the sizing call
    out[3] = tot[kResLists];
    return GPD_OK;
  }
  const bool want_bytes = bytes != nullptr || max_bytes != 0;
  if (tot[kResDgrams] > max_dgrams)
    return set_error(GPD_ERR_INVALID, "%s: %llu datagrams, max_dgrams is %llu", who,
                     (unsigned long long)tot[kResDgrams], (unsigned long long)max_dgrams);
  if (want_bytes && tot[kResBytes] > max_bytes)
    return set_error(GPD_ERR_INVALID, "%s: %llu bytes, max_bytes is %llu", who, (unsigned long long)tot[kResBytes],
                     (unsigned long long)max_bytes);
  // the new carry beside the old one
  const uint32_t nl2 = (uint32_t)tot[kResLists], nf2 = (uint32_t)tot[kResNodes];
  const uint64_t nb2 = tot[kResStore];
  if (!grow(&New.lists, &New.cap_lists, (size_t)nl2 * sizeof(IprListRec)) ||
      !grow(&New.nodes, &New.cap_nodes, (size_t)nf2 * sizeof(IprNode)) ||
      !grow(&New.store, &New.cap_store, up16((size_t)nb2)))
    return set_error(GPD_ERR_NOMEM, "%s: allocating the carried lists failed", who);
  A.nl = New.lists;
  A.nn = New.nodes;
  A.ndg = (uint32_t)tot[kResDgrams];
  hipLaunchKernelGGL(ir_place_kernel, dim3((cnt + 255u) / 256u), dim3(256), 0, s, A);
  if (A.ndg) hipLaunchKernelGGL(ir_pieces_kernel, dim3((A.ndg + kWalkWaves - 1u) / kWalkWaves), dim3(64 * kWalkWaves), 0, s, A);
  if (nl2) hipLaunchKernelGGL(ir_carry_kernel, dim3(wgrid), dim3(64 * kWalkWaves), 0, s, A);
  PieceSource G{};  // both gathers read the old store and the batch
  G.set(kIprStore, Old.store, Old.nb);
  G.set(kIprBatch, A.data, A.dlen);
  G.pieces = A.cpieces;
  launch_gather(G, nf2, New.store, nb2, s);
  if (want_bytes && A.ndg) {
    G.pieces = A.dpieces;
    launch_gather(G, (uint32_t)tot[kResPieces], bytes, tot[kResBytes], s);
    hipLaunchKernelGGL(ir_patch_kernel, dim3((A.ndg + 255u) / 256u), dim3(256), 0, s, A, tot[kResBytes]);
  }
  GPD_TRY(hipGetLastError());
  GPD_TRY(hipStreamSynchronize(s));
  New.nl = nl2;
  New.nf = nf2;
  New.nb = nb2;
  d->cur ^= 1;
  d->live[0] = nl2;
  d->live[1] = nf2;
  d->live[2] = nb2;
  out[1] = cnt;
  if (!want_bytes) out[2] = tot[kResBytes];
  return GPD_OK;
}
