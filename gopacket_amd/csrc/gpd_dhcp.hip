// gpd_dhcp.hip — the DHCP message decode (include/gpd_dhcp.h): (*DHCPv4).DecodeFromBytes
// (layers/dhcpv4.go:126-179) and (*DHCPv6).DecodeFromBytes (layers/dhcpv6.go:89-124) for every
// packet of a decoded device batch whose decode stopped at LayerTypeDHCPv4 or LayerTypeDHCPv6.  The
// walk itself is gpd_dhcp_walk.h, shared with the host entry point.
//
// Passes are separated by launch boundaries only; no kernel waits on another workgroup (no
// decoupled look-back, no spin on a global word).  The candidate count stays on the device until
// the one host synchronisation: every kernel after the compaction reads it from blk[nblk] and
// strides over the candidates.  One compaction serves both versions; a candidate's version is read
// again from its layers word.
//
//   dhcp_count_kernel    one lane per packet: is it a candidate?  (gpd_compact.h: mask bit, block count)
//   dhcp_scan_kernel     one workgroup: exclusive scan of the block counts
//   dhcp_index_kernel    the candidates' packet indices in order
//   dhcp_locate_kernel   one lane per candidate: where the message lies (gpd_locate.h, shared with
//                        gpd_dns.hip and gpd_tls.hip)
//   dhcp_size_kernel     one lane per message: the walk with the counting sink; the message's
//                        option count and the deferred total
//   dhcp_sum_kernel      per 2048 messages the sum of the option counts (gpd_stream_util.h scan_sum)
//   dhcp_scan2_kernel    one workgroup: compact_scan over the block sums
//   dhcp_apply_kernel    the counts -> exclusive prefixes in place (scan_apply), the total behind them
//     -- the host reads the totals, checks the capacities --
//   dhcp_emit_kernel     one lane per message: the walk again with the storing sink, and the
//                        message record
//
// A lane per message reads the fixed header and then two (v4) or four (v6) bytes an option and a
// jump; a wave's 64 messages diverge, which is accepted.  The budget
// (gpd_dhcp_config.max_options) bounds what one lane can be made to do.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpd_compact.h"
#include "gpd_dev_generic.h"
#include "gpd_dhcp_walk.h"
#include "gpd_locate.h"
#include "gpd_stream_util.h"
#include "../../include/gpd_dhcp.h"

namespace gpd {
namespace {

static_assert(sizeof(gpd_dhcp_msg) == 48 && sizeof(gpd_dhcp_opt) == 8, "include/gpd_dhcp.h layouts");
static_assert(offsetof(gpd_dhcp_msg, n_opts) == 16 && offsetof(gpd_dhcp_msg, secs) == 32 &&
                  offsetof(gpd_dhcp_msg, verdict) == 36 && offsetof(gpd_dhcp_msg, htype) == 40 &&
                  offsetof(gpd_dhcp_msg, mflags) == 43,
              "dhcp_emit_kernel packs the message record by these offsets");

struct DhcpArgs {
  KParams P;                // the batch
  uint32_t max_options;
  gpd_dhcp_msg *msgs;       // the caller's
  gpd_dhcp_opt *opts;
  // scratch of the context
  uint32_t nblk;            // ceil(n / 2048): blocks of the compaction, and the bound of the count scan's
  uint32_t *blk;            // nblk + 1: per-block candidate counts -> exclusive prefix; [nblk] = candidates
  uint64_t *mask;           // one bit per packet
  uint32_t *idx;            // the candidates' packet indices in order
  uint32_t *d_off, *d_len;  // per candidate: where its message lies in the packet
  uint32_t *forced;         // per candidate: saturated offsets or layer count: deferred unwalked
  uint32_t *no;             // per message (+1): options -> exclusive prefix; [cnt] = the total
  uint32_t *blk2;           // nblk + 1: block sums of no
  uint64_t *tot;            // [0] options (exact), [1] deferred
};

// The stop type of packet i when it is a candidate (its decode stopped at LayerTypeDHCPv4 or
// LayerTypeDHCPv6 without an error), else 0.
__device__ __forceinline__ uint32_t dhcp_stop(const KParams &P, uint32_t i) {
  uint32_t st;
  uint64_t lw;
  if (P.rec) {
    st = P.rec[i].status;
    lw = P.rec[i].layers;
  } else {
    st = P.status[i];
    lw = P.layers[i];
  }
  const uint32_t stop = (uint32_t)GPD_LAYERS_STOP(lw);
  if (GPD_STATUS_CLASS(st) == GPD_ST_DECODE_ERROR) return 0u;
  return stop == GPD_LT_DHCPV4 || stop == GPD_LT_DHCPV6 ? stop : 0u;
}

__global__ __launch_bounds__(256) void dhcp_count_kernel(DhcpArgs A) {
  compact_count((uint32_t)A.P.n, A.mask, A.blk, [&A](uint32_t i) { return dhcp_stop(A.P, i) != 0u; });
}
__global__ __launch_bounds__(1024) void dhcp_scan_kernel(DhcpArgs A) { compact_scan(A.blk, A.nblk); }
__global__ __launch_bounds__(64) void dhcp_index_kernel(DhcpArgs A) {
  compact_index(A.blk, A.mask, A.idx, (uint32_t)A.P.n);
}
template <bool PAGES>
__global__ __launch_bounds__(256) void dhcp_locate_kernel(DhcpArgs A) {
  locate_payloads<PAGES>(A.P, A.blk[A.nblk], A.idx, A.d_off, A.d_len, A.forced);
}

// Message j: the located payload of candidate j, and which decode it gets.
struct DhcpData {
  const uint8_t *d;
  uint32_t len, packet, data_off, version;
  bool forced;  // deferred without a walk
};

__device__ __forceinline__ DhcpData dhcp_data(const DhcpArgs &A, uint32_t j) {
  const KParams &P = A.P;
  DhcpData D;
  D.packet = A.idx[j];
  D.data_off = A.d_off[j];
  D.len = A.d_len[j];
  D.d = P.data + min(P.offset[D.packet], (uint32_t)P.data_len) + D.data_off;
  D.forced = A.forced[j] != 0;
  D.version = dhcp_stop(P, D.packet) == GPD_LT_DHCPV6 ? 6u : 4u;
  return D;
}

template <class Sink>
__device__ __forceinline__ void dhcp_walk_msg(const DhcpArgs &A, const DhcpData &D, const Sink &sink, DhcpWalk &W,
                                              gpd_dhcp_msg &m) {
  W.max_options = A.max_options;
  if (D.forced) dhcp_deferred(D.version, D.len, W, m);
  else dhcp_walk(D.version, D.d, D.len, sink, W, m);
}

__global__ __launch_bounds__(256) void dhcp_size_kernel(DhcpArgs A) {
  const uint32_t cnt = A.blk[A.nblk];
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const DhcpData D = dhcp_data(A, j);
    DhcpWalk W;
    gpd_dhcp_msg m;
    dhcp_walk_msg(A, D, DhcpCountSink{}, W, m);
    A.no[j] = W.n_opts;
    if (m.verdict == GPD_DHCP_DEFERRED) atomicAdd(reinterpret_cast<unsigned long long *>(A.tot + 1), 1ull);
  }
}

__global__ __launch_bounds__(256) void dhcp_sum_kernel(DhcpArgs A) {
  const uint32_t *v = A.no;
  scan_sum(A.blk[A.nblk], A.blk2, A.tot, [v](uint32_t j) { return v[j]; });
}
__global__ __launch_bounds__(1024) void dhcp_scan2_kernel(DhcpArgs A) { compact_scan(A.blk2, A.nblk); }
__global__ __launch_bounds__(256) void dhcp_apply_kernel(DhcpArgs A) {
  uint32_t *v = A.no;
  scan_apply(A.blk[A.nblk], A.blk2, v, true, [v](uint32_t j) { return v[j]; });
}

// The capacities were checked on the host: msgs holds cnt records, opts no[cnt].
__global__ __launch_bounds__(256) void dhcp_emit_kernel(DhcpArgs A) {
  const uint32_t cnt = A.blk[A.nblk];
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const DhcpData D = dhcp_data(A, j);
    const uint32_t o0 = A.no[j], o1 = A.no[j + 1u];
    DhcpWalk W;
    gpd_dhcp_msg m;
    dhcp_walk_msg(A, D, DhcpStoreSink{A.opts + o0, o1 - o0}, W, m);
    // the record as three 16-byte stores (its last four bytes are reserved: zero)
    v4u *q = reinterpret_cast<v4u *>(A.msgs + j);
    q[0] = v4u{D.packet, D.data_off, m.data_len, o0};
    q[1] = v4u{m.n_opts, m.xid, m.err_off, m.err_arg};
    q[2] = v4u{(uint32_t)m.secs | ((uint32_t)m.flags << 16),
               (uint32_t)m.verdict | ((uint32_t)m.truncated << 8) | ((uint32_t)m.version << 16) | ((uint32_t)m.op << 24),
               (uint32_t)m.htype | ((uint32_t)m.hlen << 8) | ((uint32_t)m.hops << 16) | ((uint32_t)m.mflags << 24), 0u};
  }
}

}  // namespace
}  // namespace gpd

extern "C" int gpd_dhcp_decode(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res, const gpd_dhcp_config *cfg,
                               const gpd_dhcp_out *out, gpd_dhcp_counts *counts, void *stream) {
  using namespace gpd;
  const char *who = "gpd_dhcp_decode";
  if (!ctx || !in || !res || !out || !counts) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *counts = gpd_dhcp_counts{};
  const uint32_t max_options = cfg ? cfg->max_options : GPD_DHCP_MAX_OPTIONS_DEFAULT;
  if (max_options < 1u || max_options > GPD_DHCP_MAX_OPTIONS_LIMIT || (cfg && cfg->reserved))
    return set_error(GPD_ERR_INVALID, "%s: max_options %u outside 1..%u (or a nonzero reserved word)", who,
                     max_options, GPD_DHCP_MAX_OPTIONS_LIMIT);
  if (in->n >= 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: %llu packets (max 2^32 - 257)", who, (unsigned long long)in->n);
  if ((out->cap_msgs && !out->msgs) || (out->cap_opts && !out->opts))
    return set_error(GPD_ERR_INVALID, "%s: null array with a nonzero capacity", who);
  if (((uintptr_t)out->msgs & 15u) || ((uintptr_t)out->opts & 15u))
    return set_error(GPD_ERR_INVALID, "%s: msgs and opts must be 16-byte aligned", who);
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
  DhcpArgs A{};
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
  A.max_options = max_options;
  A.msgs = out->msgs;
  A.opts = out->opts;
  // one carve of the context's scratch (the slot of the DNS and TLS decodes and the TCP hand-off:
  // a context serves one call at a time, and every such call synchronises before it returns)
  const uint32_t n = (uint32_t)in->n;
  A.nblk = (n + kCompactBlock - 1u) / kCompactBlock;
  const size_t b_blk = up16(((size_t)A.nblk + 1) * 4), b_mask = up16(((size_t)n + 63) / 64 * 8);
  const size_t b_n = up16(((size_t)n + 1) * 4);
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 15, 32 + 2 * b_blk + b_mask + 5 * b_n));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.tot = reinterpret_cast<uint64_t *>(base);
  uint8_t *p = base + 32;
  A.blk = reinterpret_cast<uint32_t *>(p);
  A.blk2 = reinterpret_cast<uint32_t *>(p + b_blk);
  p += 2 * b_blk;
  A.mask = reinterpret_cast<uint64_t *>(p);
  p += b_mask;
  uint32_t **arr[5] = {&A.idx, &A.d_off, &A.d_len, &A.forced, &A.no};
  for (auto a : arr) {
    *a = reinterpret_cast<uint32_t *>(p);
    p += b_n;
  }
  const size_t lds = (P.image_words * 4u + 15u) & ~15u;
  const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, ((uint64_t)n + 255u) / 256u);
  GPD_TRY(hipMemsetAsync(A.tot, 0, 32, s));
  hipLaunchKernelGGL(dhcp_count_kernel, dim3(A.nblk), dim3(256), 0, s, A);
  hipLaunchKernelGGL(dhcp_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(dhcp_index_kernel, dim3(A.nblk), dim3(64), 0, s, A);
  if (P.use_pages) hipLaunchKernelGGL(dhcp_locate_kernel<true>, dim3(grid), dim3(256), lds, s, A);
  else hipLaunchKernelGGL(dhcp_locate_kernel<false>, dim3(grid), dim3(256), lds, s, A);
  hipLaunchKernelGGL(dhcp_size_kernel, dim3(grid), dim3(256), 0, s, A);
  hipLaunchKernelGGL(dhcp_sum_kernel, dim3(A.nblk), dim3(256), 0, s, A);
  hipLaunchKernelGGL(dhcp_scan2_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(dhcp_apply_kernel, dim3(A.nblk), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  uint32_t cnt = 0;
  GPD_TRY(hipMemcpyAsync(tot, A.tot, 16, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipMemcpyAsync(&cnt, A.blk + A.nblk, 4, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  counts->msgs = cnt;
  counts->options = tot[0];
  counts->deferred = tot[1];
  if (tot[0] > 0xFFFFFFFFull)
    return set_error(GPD_ERR_INVALID, "%s: %llu options: more than 2^32 - 1, split the batch", who,
                     (unsigned long long)tot[0]);
  if (cnt > out->cap_msgs || tot[0] > out->cap_opts)
    return set_error(GPD_ERR_INVALID, "%s: %u messages, %llu options; the capacities are %llu, %llu", who, cnt,
                     (unsigned long long)tot[0], (unsigned long long)out->cap_msgs,
                     (unsigned long long)out->cap_opts);
  if (cnt == 0) return GPD_OK;
  const unsigned egrid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, ((uint64_t)cnt + 255u) / 256u);
  hipLaunchKernelGGL(dhcp_emit_kernel, dim3(egrid), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}

extern "C" int gpd_dhcp_decode_host(uint32_t version, const uint8_t *data, uint32_t len, uint32_t max_options,
                                    gpd_dhcp_msg *msg, gpd_dhcp_opt *opts, uint64_t cap_opts,
                                    gpd_dhcp_counts *counts) {
  using namespace gpd;
  const char *who = "gpd_dhcp_decode_host";
  if ((!data && len) || !msg || !counts) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  if (version != 4u && version != 6u) return set_error(GPD_ERR_INVALID, "%s: version %u is neither 4 nor 6", who, version);
  if (cap_opts && !opts) return set_error(GPD_ERR_INVALID, "%s: null array with a nonzero capacity", who);
  *counts = gpd_dhcp_counts{};
  DhcpWalk S;
  S.max_options = max_options;
  dhcp_walk(version, data, len, DhcpCountSink{}, S, *msg);
  counts->msgs = 1;
  counts->options = S.n_opts;
  counts->deferred = msg->verdict == GPD_DHCP_DEFERRED;
  counts->work = S.work;
  if (S.n_opts > cap_opts)
    return set_error(GPD_ERR_INVALID, "%s: %u options; the capacity is %llu", who, S.n_opts,
                     (unsigned long long)cap_opts);
  DhcpWalk W;
  W.max_options = max_options;
  dhcp_walk(version, data, len, DhcpStoreSink{opts, S.n_opts}, W, *msg);
  return GPD_OK;
}
