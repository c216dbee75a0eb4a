// gpd_tcpseg.hip — the tcpassembly hand-off (include/gpd_tcpassembly.h): the TCP segments of a
// decoded device batch that Assembler.AssembleWithTimestamp acts on
// (tcpassembly/assembly.go:533-607), each with what that call reads from the TCP layer, in
// packet order or grouped by flow record (the assembler's key, :289,543), stably.
//
// The hand-over is the fragment hand-off's ordered compaction (gpd_compact.h, one copy for both): per-2048-packet
// counts and one bit per packet, their exclusive scan by one workgroup, the kept packets'
// indices in order, and one record per kept packet.  Grouping adds the project's first device
// sort, an LSD radix sort of (key, segment index) pairs, key = min(flow_id, id_bound), 8 bits a
// pass.  Each pass is three launches and no kernel waits on another workgroup (no decoupled
// look-back, no spin on a global word): passes are separated by launch boundaries only.
//
//   ts_count_kernel     one lane per packet: is it handed over?  (mask bit, per-block count)
//   ts_scan_kernel      one workgroup: exclusive scan of the block counts
//   ts_index_kernel     the kept packets' indices in order, from the mask words
//   ts_record_kernel    one lane per segment: the 32-byte record (in packet order), and with
//                       grouping its (key, index) pair
//   (the three sort kernels live in gpd_radix_sort.h, shared with gpd_tcptrack.hip)
//   sort_hist_kernel    per workgroup tile of kSortTile pairs: counts per digit, [digit][tile]
//   sort_scan_kernel    one workgroup: exclusive scan of the [digit][tile] counts in place
//   sort_scatter_kernel stable ranks inside the tile: per wave eight ballots give the lanes
//                       with the same digit, the rank is the popcount below the lane, and the
//                       waves' bases are scanned in wave order through LDS.  The last pass
//                       gathers the 32-byte records to their final places instead of the pairs.
//   ts_head_kernel      head flags where the sorted key changes (the same count/scan/index)
//   ts_group_kernel     one lane per group: its gpd_tcp_group
//
// Where t.Payload lies.  For the plain stacks — Ethernet, 802.1Q tags, IPv4 or IPv6 (no
// hop-by-hop header), TCP — the record reads the network header and trims as the decoders do:
// IPv4 Length (0 => len(data)) against the captured bytes (ip4.go:214-236), IPv6 Length
// against them (ip6.go:270-275).  Every other stack (VXLAN, extension headers, a packet whose
// decode ended in an error or past 12 layers) is run through the generic decoder again for the
// TCP object's exact BaseLayer, as the fragment hand-off does for the IPv4 object.
#include <hip/hip_runtime.h>

#include "gpd_compact.h"
#include "gpd_dev_generic.h"
#include "gpd_radix_sort.h"
#include "../../include/gpd_flow.h"
#include "../../include/gpd_tcpassembly.h"

namespace gpd {
namespace {

static_assert(sizeof(gpd_tcp_seg) == 32 && sizeof(gpd_tcp_group) == 16, "include/gpd_tcpassembly.h layouts");

constexpr uint32_t kCountBlock = kCompactBlock;  // items per counting workgroup

struct TsArgs {
  KParams P;
  const uint32_t *flow_id;  // may be NULL
  uint32_t id_bound;
  uint32_t cnt;             // handed-over segments (known on the host after the scan)
  gpd_tcp_seg *segs;        // the caller's
  gpd_tcp_group *groups;
  // scratch of the context
  uint32_t nblk;            // blocks of the compaction in flight
  uint32_t *blk;            // nblk + 1: per-block counts -> exclusive prefix; [nblk] = total
  uint64_t *mask;           // one bit per item
  uint32_t *idx;            // the kept items in order
  gpd_tcp_seg *tmp;         // grouping: the records in packet order
  uint2 *pa, *pb;           // ping-pong (key, segment index) pairs
  uint32_t *hist;           // [256][tiles]
  uint32_t *skey;           // the keys in final order
  uint64_t *res;            // [0] groups, [1] ungrouped
  uint32_t ntile;
};

__device__ __forceinline__ uint32_t be16p(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
__device__ __forceinline__ uint32_t be32p(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// Packet i's segment record; false when it is not handed over.  The candidates are the packets
// the flow table keys (gpd_flow.hip flow_key) whose transport endpoint type is TCPPort.
template <bool PAGES>
__device__ __forceinline__ bool tcp_segment(const KParams &P, const Tab<PAGES> &T, uint32_t options, uint32_t i,
                                            gpd_tcp_seg &r) {
  uint32_t st;
  uint64_t lw;
  if (P.rec) {
    st = P.rec[i].status;
    lw = P.rec[i].layers;
  } else {
    st = P.status[i];
    lw = P.layers[i];
  }
  const uint32_t ho = P.hdr_off[i];
  const uint32_t nt = GPD_STATUS_NET_EPT(st), tt = GPD_STATUS_TP_EPT(st);
  const uint32_t no = GPD_HDR_NET(ho), to = GPD_HDR_TP(ho);
  if (nt == 0 || tt != 4u || no == GPD_HDR_NONE || to == GPD_HDR_NONE) return false;
  const uint32_t dlen = (uint32_t)P.data_len;
  const uint32_t off = min(P.offset[i], dlen), len = min(P.caplen[i], dlen - off);
  const uint8_t *pkt = P.data + off;
  uint32_t c_off = to, p_off = 0, p_len = 0;
  bool have = false;
  const uint32_t nl = GPD_STATUS_NLAYERS(st);
  if (P.first == GPD_LT_ETHERNET && GPD_STATUS_CLASS(st) != GPD_ST_DECODE_ERROR && !GPD_STATUS_SATURATED(st) &&
      nl >= 3 && nl <= GPD_CORE_MAX_LAYERS && GPD_LAYERS_CODE(lw, 0) == GPD_C_ETHERNET) {
    uint32_t k = 1;
    while (k < nl && GPD_LAYERS_CODE(lw, k) == GPD_C_DOT1Q) ++k;
    const uint32_t net = k < nl ? GPD_LAYERS_CODE(lw, k) : 0u;
    const bool tail = k + 2 == nl || (k + 3 == nl && GPD_LAYERS_CODE(lw, k + 2) == GPD_C_PAYLOAD);
    const uint32_t ipo = 14u + 4u * (k - 1u);
    if ((net == GPD_C_IPV4 || net == GPD_C_IPV6) && k + 1 < nl && GPD_LAYERS_CODE(lw, k + 1) == GPD_C_TCP && tail &&
        no == ipo && be16p(pkt + 12) >= 0x0600u) {  // (a length-typed frame trims: ethernet.go:50-57)
      const uint8_t *h = pkt + ipo;
      const uint32_t l0 = len - ipo;
      uint32_t tcp_at = 0, tlen = 0;
      if (net == GPD_C_IPV4) {  // ip4.go:214-236
        uint32_t length = be16p(h + 2);
        if (length == 0) length = l0 & 0xFFFFu;
        const uint32_t hl = (h[0] & 0x0Fu) * 4u, d = l0 > length ? length : l0;
        tcp_at = ipo + hl;
        tlen = d - hl;
      } else if (h[6] != 0) {  // ip6.go:270-275 (a hop-by-hop header is parsed inside: generic)
        const uint32_t length = be16p(h + 4);
        tlen = l0 - 40u;
        if (length <= tlen) tlen = length;
        tcp_at = ipo + 40u;
      }
      if (tcp_at == to && tlen <= len) {
        const uint32_t ds = (uint32_t)(pkt[to + 12] >> 4) * 4u;
        if (ds >= 20u && ds <= tlen) {
          p_off = to + ds;
          p_len = tlen - ds;
          have = true;
        }
      }
    }
  }
  if (!have) {
    gpd_ext_rec e;
    decode_packet<true>(GlbSrc{P.data, off}, len, T, P.first,
                        options | GPD_OPT_NO_CHECKSUMS | GPD_OPT_NO_FLOW_HASH, &e);
    if (!(e.obj_valid & (1u << GPD_OBJ_TCP))) return false;
    c_off = e.obj[GPD_OBJ_TCP].contents_off;
    p_off = e.obj[GPD_OBJ_TCP].payload_off;
    p_len = e.obj[GPD_OBJ_TCP].payload_len;
  }
  const uint8_t *t = pkt + to;  // the header t's fields were last read from (gpd.h hdr_off)
  const uint32_t flags = be16p(t + 12) & 0x1FFu;
  if (!(flags & (GPD_TCP_SYN | GPD_TCP_FIN | GPD_TCP_RST)) && p_len == 0) return false;  // assembly.go:535
  r.packet = i;
  r.flow_id = GPD_FLOW_NONE;
  r.seq = be32p(t + 4);
  r.ack = be32p(t + 8);
  r.payload_off = p_off;
  r.payload_len = p_len;
  r.tcp_off = (uint16_t)c_off;
  r.flags = (uint16_t)flags;
  r.lookup_only = (uint8_t)(!(flags & GPD_TCP_SYN) && p_len == 0);  // :550-551
  r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
  return true;
}

// ---- ordered compaction: count, scan, index (gpd_compact.h) -----------------------------------
template <bool PAGES>
__global__ __launch_bounds__(256) void ts_count_kernel(TsArgs A) {
  const KParams &P = A.P;
  for (uint32_t k = threadIdx.x; k < P.image_words; k += 256) reinterpret_cast<uint32_t *>(g_lds)[k] = P.image[k];
  __syncthreads();
  const Tab<PAGES> T = make_tab<PAGES>(P);
  const uint32_t options = P.options & ~kDiagMask;
  compact_count((uint32_t)P.n, A.mask, A.blk, [&](uint32_t i) {
    gpd_tcp_seg rec;
    return tcp_segment<PAGES>(P, T, options, i, rec);
  });
}

// Head flags of the sorted keys: item r starts a group when its key differs from r - 1's.
__global__ __launch_bounds__(256) void ts_head_kernel(TsArgs A) {
  compact_count(A.cnt, A.mask, A.blk, [&A](uint32_t i) { return i == 0 || A.skey[i] != A.skey[i - 1]; });
}

__global__ __launch_bounds__(1024) void ts_scan_kernel(TsArgs A) { compact_scan(A.blk, A.nblk); }

__global__ __launch_bounds__(64) void ts_index_kernel(TsArgs A, uint32_t nitems) {
  compact_index(A.blk, A.mask, A.idx, nitems);
}

// One lane per handed-over packet, in packet order: its record, to the caller's array or (with
// grouping) to the scratch the last sort pass gathers from, and its (key, index) pair.
template <bool PAGES>
__global__ __launch_bounds__(256) void ts_record_kernel(TsArgs A) {
  const KParams &P = A.P;
  for (uint32_t k = threadIdx.x; k < P.image_words; k += 256) reinterpret_cast<uint32_t *>(g_lds)[k] = P.image[k];
  __syncthreads();
  const Tab<PAGES> T = make_tab<PAGES>(P);
  const uint32_t options = P.options & ~kDiagMask;
  gpd_tcp_seg *dst = A.flow_id ? A.tmp : A.segs;
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < A.cnt; j += gridDim.x * 256u) {
    const uint32_t i = A.idx[j];
    gpd_tcp_seg r{};
    r.packet = i;
    (void)tcp_segment<PAGES>(P, T, options, i, r);  // (true: the count kernel kept it)
    if (A.flow_id) {
      r.flow_id = A.flow_id[i];
      A.pa[j] = make_uint2(min(r.flow_id, A.id_bound), j);
    }
    const uint4 *s = reinterpret_cast<const uint4 *>(&r);
    uint4 *d = reinterpret_cast<uint4 *>(dst + j);
    d[0] = s[0];
    d[1] = s[1];
  }
}

// ---- the radix sort (gpd_radix_sort.h) -----------------------------------------------------------
// The last pass's sink: the record of the pair's segment goes to its final place, with the key
// beside it for the groups.
struct SegSink {
  const gpd_tcp_seg *tmp;
  gpd_tcp_seg *segs;
  uint32_t *skey;
  __device__ __forceinline__ void operator()(uint32_t pos, uint2 p) const {
    const uint4 *s = reinterpret_cast<const uint4 *>(tmp + p.y);
    const uint4 s0 = s[0], s1 = s[1];
    uint4 *q = reinterpret_cast<uint4 *>(segs + pos);
    q[0] = s0;
    q[1] = s1;
    skey[pos] = p.x;
  }
};

// One lane per group: heads[g] (idx) is where it starts.  The last lane leaves the counts.
__global__ __launch_bounds__(256) void ts_group_kernel(TsArgs A) {
  const uint32_t ng = A.blk[A.nblk];
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= ng) return;
  const uint32_t r = A.idx[g], nxt = g + 1u < ng ? A.idx[g + 1u] : A.cnt;
  const uint32_t key = A.skey[r];
  const bool un = key >= A.id_bound;
  A.groups[g] = gpd_tcp_group{un ? GPD_TCP_UNGROUPED : key, r, nxt - r, A.segs[r].packet};
  if (g == ng - 1u) {
    A.res[0] = ng;
    A.res[1] = un ? nxt - r : 0u;
  }
}

}  // namespace
}  // namespace gpd

extern "C" int gpd_tcp_segments(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res,
                                const uint32_t *flow_id, uint32_t id_bound,
                                gpd_tcp_seg *segs, gpd_tcp_group *groups, uint64_t max_out,
                                uint64_t *count, uint64_t *ngroups, uint64_t *ungrouped, void *stream) {
  using namespace gpd;
  const char *who = "gpd_tcp_segments";
  if (!ctx || !in || !res || !count || !ngroups || !ungrouped)
    return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *count = *ngroups = *ungrouped = 0;
  if (in->n > 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 256)", who, (unsigned long long)in->n);
  if (max_out && !segs) return set_error(GPD_ERR_INVALID, "%s: null segs with max_out > 0", who);
  if (segs && flow_id && !groups) return set_error(GPD_ERR_INVALID, "%s: grouping needs groups[]", who);
  if (((uintptr_t)segs & 15u) || ((uintptr_t)groups & 15u))
    return set_error(GPD_ERR_INVALID, "%s: segs and groups must be 16-byte aligned", who);
  if (in->n == 0) return GPD_OK;
  if (!in->data || !in->offset || !in->caplen)
    return set_error(GPD_ERR_INVALID, "%s: batch data/offset/caplen must be non-NULL", who);
  if (in->data_len >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: data_len %llu outside the 32-bit offset range", who,
                     (unsigned long long)in->data_len);
  if (!res->hdr_off || (!res->records && (!res->status || !res->layers)))
    return set_error(GPD_ERR_INVALID, "%s: needs hdr_off and status + layers (or records)", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  TsArgs A{};
  KParams &P = A.P;
  P.data = in->data;
  P.data_len = in->data_len;
  P.offset = in->offset;
  P.caplen = in->caplen;
  P.n = in->n;
  P.status = res->status;
  P.layers = res->layers;
  P.rec = res->records;
  P.hdr_off = res->hdr_off;
  ctx_fill_kparams(ctx, P);
  A.flow_id = flow_id;
  A.id_bound = id_bound;
  A.segs = segs;
  A.groups = groups;
  // the compaction's scratch, sized by the batch: counts, mask, indices, the result words
  const uint32_t n = (uint32_t)in->n;
  A.nblk = (n + kCountBlock - 1u) / kCountBlock;
  const size_t b_blk = up16(((size_t)A.nblk + 1) * 4), b_mask = up16(((size_t)n + 63) / 64 * 8);
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 15, 16 + b_blk + b_mask + up16((size_t)n * 4)));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.res = reinterpret_cast<uint64_t *>(base);
  A.blk = reinterpret_cast<uint32_t *>(base + 16);
  A.mask = reinterpret_cast<uint64_t *>(base + 16 + b_blk);
  A.idx = reinterpret_cast<uint32_t *>(base + 16 + b_blk + b_mask);
  const size_t lds = (P.image_words * 4u + 15u) & ~15u;
  if (P.use_pages) hipLaunchKernelGGL(ts_count_kernel<true>, dim3(A.nblk), dim3(256), lds, s, A);
  else hipLaunchKernelGGL(ts_count_kernel<false>, dim3(A.nblk), dim3(256), lds, s, A);
  hipLaunchKernelGGL(ts_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint32_t total = 0;
  GPD_TRY(hipMemcpyAsync(&total, A.blk + A.nblk, 4, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  *count = total;
  if (!segs && !max_out) return GPD_OK;  // the sizing call
  if (total > max_out)
    return set_error(GPD_ERR_INVALID, "%s: %u segments, max_out is %llu", who, total, (unsigned long long)max_out);
  if (total == 0) return GPD_OK;
  A.cnt = total;
  hipLaunchKernelGGL(ts_index_kernel, dim3(A.nblk), dim3(64), 0, s, A, n);
  if (flow_id) {  // the sort's scratch, sized by the hand-off: records, two pair arrays, keys, counts
    A.ntile = (total + kSortTile - 1u) / kSortTile;
    const size_t b_tmp = (size_t)total * sizeof(gpd_tcp_seg), b_pair = up16((size_t)total * 8);
    const size_t b_key = up16((size_t)total * 4), b_hist = (size_t)A.ntile * 256 * 4;
    auto *sb = static_cast<uint8_t *>(ctx_scratch(ctx, 16, b_tmp + 2 * b_pair + b_key + b_hist));
    if (!sb) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
    A.tmp = reinterpret_cast<gpd_tcp_seg *>(sb);
    A.pa = reinterpret_cast<uint2 *>(sb + b_tmp);
    A.pb = reinterpret_cast<uint2 *>(sb + b_tmp + b_pair);
    A.skey = reinterpret_cast<uint32_t *>(sb + b_tmp + 2 * b_pair);
    A.hist = reinterpret_cast<uint32_t *>(sb + b_tmp + 2 * b_pair + b_key);
  }
  const unsigned rgrid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, (total + 255u) / 256u);
  if (P.use_pages) hipLaunchKernelGGL(ts_record_kernel<true>, dim3(rgrid), dim3(256), lds, s, A);
  else hipLaunchKernelGGL(ts_record_kernel<false>, dim3(rgrid), dim3(256), lds, s, A);
  GPD_TRY(hipGetLastError());
  if (!flow_id) {
    GPD_TRY(hipStreamSynchronize(s));
    return GPD_OK;
  }
  const SortArgs S{total, A.ntile, A.hist};
  const uint32_t passes = sort_passes(id_bound);  // keys lie in [0, id_bound]
  const uint2 *src = sort_leading_passes(S, A.pa, A.pb, passes, s);
  sort_last_pass(S, src, passes, SegSink{A.tmp, A.segs, A.skey}, s);
  // the groups: the compaction again, over the sorted keys' head flags
  A.nblk = (total + kCountBlock - 1u) / kCountBlock;
  GPD_TRY(hipMemsetAsync(A.res, 0, 16, s));
  hipLaunchKernelGGL(ts_head_kernel, dim3(A.nblk), dim3(256), 0, s, A);
  hipLaunchKernelGGL(ts_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(ts_index_kernel, dim3(A.nblk), dim3(64), 0, s, A, total);
  hipLaunchKernelGGL(ts_group_kernel, dim3((total + 255u) / 256u), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t out[2] = {0, 0};
  GPD_TRY(hipMemcpyAsync(out, A.res, 16, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  *ngroups = out[0];
  *ungrouped = out[1];
  return GPD_OK;
}
