// gpd_dns.hip — the DNS message decode (include/gpd_dns.h): (*DNS).DecodeFromBytes
// (layers/dns.go:304-392) for every packet of a decoded device batch whose decode stopped at
// LayerTypeDNS.  The walk itself is gpd_dns_walk.h, shared with the host entry point.
//
// Passes are separated by launch boundaries only; no kernel waits on another workgroup (no
// decoupled look-back, no spin on a global word).  The candidate count stays on the device until
// the one host synchronisation: every kernel after the compaction reads it from blk[nblk] and
// strides over the candidates.
//
//   dns_count_kernel    one lane per packet: is it a candidate?  (gpd_compact.h: mask bit, block count)
//   dns_scan_kernel     one workgroup: exclusive scan of the block counts
//   dns_index_kernel    the candidates' packet indices in order
//   dns_locate_kernel   one lane per candidate: the generic decoder over the packet again for the
//                       last decoded layer's Payload — where the message lies (data_off, data_len;
//                       gpd_locate.h, shared with gpd_tls.hip)
//   dns_size_kernel     one lane per candidate: the full validating walk with the counting sink;
//                       the message's entry count and name bytes, and the deferred total
//   dns_sum_kernel      per 2048 candidates the sums of both counts (gpd_stream_util.h scan_sum)
//   dns_scan2_kernel    two workgroups: compact_scan over each array of block sums
//   dns_apply_kernel    both counts -> exclusive prefixes in place (scan_apply), totals behind them
//     -- the host reads the totals, checks the capacities --
//   dns_emit_kernel     one lane per candidate: the walk again with the storing sink, and the
//                       message record
//
// A lane per message reads `data` from global memory; a wave's 64 messages diverge, which is
// accepted (a query walks ~30 bytes).  The budget (gpd_dns_config.max_work, at most 65535 steps)
// bounds what one lane can be made to do.
#include <hip/hip_runtime.h>

#include "gpd_compact.h"
#include "gpd_dev_generic.h"
#include "gpd_dns_walk.h"
#include "gpd_locate.h"
#include "gpd_stream_util.h"
#include "../../include/gpd_dns.h"

namespace gpd {
namespace {

static_assert(sizeof(gpd_dns_msg) == 48 && sizeof(gpd_dns_entry) == 32, "include/gpd_dns.h layouts");

struct DnsArgs {
  KParams P;
  uint32_t max_work;
  gpd_dns_msg *msgs;        // the caller's
  gpd_dns_entry *entries;
  uint8_t *names;
  // scratch of the context
  uint32_t nblk;            // ceil(n / 2048): blocks of the compaction, and the bound of the count scans'
  uint32_t *blk;            // nblk + 1: per-block candidate counts -> exclusive prefix; [nblk] = candidates
  uint64_t *mask;           // one bit per packet
  uint32_t *idx;            // the candidates' packet indices in order
  uint32_t *d_off, *d_len;  // per candidate: where its message lies in the packet
  uint32_t *forced;         // per candidate: saturated offsets or layer count, so the message is the
                            // host's: walked with a budget of one step, which defers whatever has
                            // a question or record and decides the rest (they have no entries)
  uint32_t *ne, *nb;        // per candidate (+1): entries / name bytes -> exclusive prefixes; [cnt] = totals
  uint32_t *blk2;           // 2 x (nblk + 1): block sums of ne, then of nb
  uint64_t *tot;            // [0] entries, [1] name bytes (exact), [2] deferred
};

// Packet i is a candidate when its decode stopped at LayerTypeDNS without an error.
__device__ __forceinline__ bool dns_candidate(const KParams &P, uint32_t i) {
  uint32_t st;
  uint64_t lw;
  if (P.rec) {
    st = P.rec[i].status;
    lw = P.rec[i].layers;
  } else {
    st = P.status[i];
    lw = P.layers[i];
  }
  return GPD_STATUS_CLASS(st) != GPD_ST_DECODE_ERROR && GPD_LAYERS_STOP(lw) == GPD_LT_DNS;
}

__global__ __launch_bounds__(256) void dns_count_kernel(DnsArgs A) {
  compact_count((uint32_t)A.P.n, A.mask, A.blk, [&A](uint32_t i) { return dns_candidate(A.P, i); });
}
__global__ __launch_bounds__(1024) void dns_scan_kernel(DnsArgs A) { compact_scan(A.blk, A.nblk); }
__global__ __launch_bounds__(64) void dns_index_kernel(DnsArgs A) {
  compact_index(A.blk, A.mask, A.idx, (uint32_t)A.P.n);
}

template <bool PAGES>
__global__ __launch_bounds__(256) void dns_locate_kernel(DnsArgs A) {
  locate_payloads<PAGES>(A.P, A.blk[A.nblk], A.idx, A.d_off, A.d_len, A.forced);  // gpd_locate.h
}

__global__ __launch_bounds__(256) void dns_size_kernel(DnsArgs A) {
  const KParams &P = A.P;
  const uint32_t cnt = A.blk[A.nblk];
  const uint32_t dlen = (uint32_t)P.data_len;
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const uint32_t i = A.idx[j];
    const uint32_t off = min(P.offset[i], dlen);
    DnsWalk W;
    W.max_work = A.forced[j] ? 1u : A.max_work;
    gpd_dns_msg m;
    dns_walk(P.data + off + A.d_off[j], A.d_len[j], DnsCountSink{}, W, m);
    A.ne[j] = W.n_entries;
    A.nb[j] = W.name_bytes;
    if (m.verdict == GPD_DNS_DEFERRED) atomicAdd(reinterpret_cast<unsigned long long *>(A.tot + 2), 1ull);
  }
}

// blockIdx.y: 0 the entry counts, 1 the name bytes.
__global__ __launch_bounds__(256) void dns_sum_kernel(DnsArgs A) {
  const uint32_t cnt = A.blk[A.nblk];
  const uint32_t *v = blockIdx.y ? A.nb : A.ne;
  scan_sum(cnt, A.blk2 + (size_t)blockIdx.y * (A.nblk + 1u), A.tot + blockIdx.y, [v](uint32_t j) { return v[j]; });
}
__global__ __launch_bounds__(1024) void dns_scan2_kernel(DnsArgs A) {
  compact_scan(A.blk2 + (size_t)blockIdx.x * (A.nblk + 1u), A.nblk);
}
__global__ __launch_bounds__(256) void dns_apply_kernel(DnsArgs A) {
  const uint32_t cnt = A.blk[A.nblk];
  uint32_t *v = blockIdx.y ? A.nb : A.ne;
  scan_apply(cnt, A.blk2 + (size_t)blockIdx.y * (A.nblk + 1u), v, true, [v](uint32_t j) { return v[j]; });
}

// The capacities were checked on the host: msgs holds cnt records, entries ne[cnt], names nb[cnt].
__global__ __launch_bounds__(256) void dns_emit_kernel(DnsArgs A) {
  const KParams &P = A.P;
  const uint32_t cnt = A.blk[A.nblk];
  const uint32_t dlen = (uint32_t)P.data_len;
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const uint32_t i = A.idx[j];
    const uint32_t off = min(P.offset[i], dlen);
    const uint32_t e0 = A.ne[j], e1 = A.ne[j + 1u], b0 = A.nb[j], b1 = A.nb[j + 1u];
    const uint32_t d_off = A.d_off[j], d_len = A.d_len[j];
    const uint8_t *d = P.data + off + d_off;
    gpd_dns_msg m;
    DnsWalk W;
    W.max_work = A.forced[j] ? 1u : A.max_work;
    dns_walk(d, d_len, DnsStoreSink{A.entries + e0, e1 - e0, A.names + b0, b1 - b0, b0}, W, m);
    m.packet = i;
    m.data_off = d_off;
    m.first_entry = e0;
    const uint4 *s = reinterpret_cast<const uint4 *>(&m);
    uint4 *q = reinterpret_cast<uint4 *>(A.msgs + j);
    q[0] = s[0];
    q[1] = s[1];
    q[2] = s[2];
  }
}

}  // namespace
}  // namespace gpd

extern "C" int gpd_dns_decode(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res, const gpd_dns_config *cfg,
                              const gpd_dns_out *out, gpd_dns_counts *counts, void *stream) {
  using namespace gpd;
  const char *who = "gpd_dns_decode";
  if (!ctx || !in || !res || !out || !counts) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *counts = gpd_dns_counts{};
  const uint32_t max_work = cfg ? cfg->max_work : GPD_DNS_MAX_WORK_DEFAULT;
  if (max_work < 1u || max_work > GPD_DNS_MAX_WORK_LIMIT || (cfg && cfg->reserved))
    return set_error(GPD_ERR_INVALID, "%s: max_work %u outside 1..%u (or a nonzero reserved word)", who, max_work,
                     GPD_DNS_MAX_WORK_LIMIT);
  if (in->n >= 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 257)", who, (unsigned long long)in->n);
  if ((out->cap_msgs && !out->msgs) || (out->cap_entries && !out->entries) || (out->cap_names && !out->names))
    return set_error(GPD_ERR_INVALID, "%s: null array with a nonzero capacity", who);
  if (((uintptr_t)out->msgs & 15u) || ((uintptr_t)out->entries & 15u))
    return set_error(GPD_ERR_INVALID, "%s: msgs and entries must be 16-byte aligned", who);
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
  DnsArgs A{};
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
  A.max_work = max_work;
  A.msgs = out->msgs;
  A.entries = out->entries;
  A.names = out->names;
  // one carve of the context's scratch (the TCP hand-off's slot: a context serves one call at a
  // time, and both calls synchronise before they return)
  const uint32_t n = (uint32_t)in->n;
  A.nblk = (n + kCompactBlock - 1u) / kCompactBlock;
  const size_t b_blk = up16(((size_t)A.nblk + 1) * 4), b_mask = up16(((size_t)n + 63) / 64 * 8);
  const size_t b_n = up16(((size_t)n + 1) * 4);
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 15, 32 + 3 * b_blk + b_mask + 6 * b_n));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.tot = reinterpret_cast<uint64_t *>(base);
  uint8_t *p = base + 32;
  A.blk = reinterpret_cast<uint32_t *>(p);
  A.blk2 = reinterpret_cast<uint32_t *>(p + b_blk);  // 2 x (nblk + 1) words inside 2 x b_blk bytes
  p += 3 * b_blk;
  A.mask = reinterpret_cast<uint64_t *>(p);
  p += b_mask;
  uint32_t **arr[6] = {&A.idx, &A.d_off, &A.d_len, &A.forced, &A.ne, &A.nb};
  for (auto a : arr) {
    *a = reinterpret_cast<uint32_t *>(p);
    p += b_n;
  }
  const size_t lds = (P.image_words * 4u + 15u) & ~15u;
  const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, ((uint64_t)n + 255u) / 256u);
  GPD_TRY(hipMemsetAsync(A.tot, 0, 32, s));
  hipLaunchKernelGGL(dns_count_kernel, dim3(A.nblk), dim3(256), 0, s, A);
  hipLaunchKernelGGL(dns_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(dns_index_kernel, dim3(A.nblk), dim3(64), 0, s, A);
  if (P.use_pages) hipLaunchKernelGGL(dns_locate_kernel<true>, dim3(grid), dim3(256), lds, s, A);
  else hipLaunchKernelGGL(dns_locate_kernel<false>, dim3(grid), dim3(256), lds, s, A);
  hipLaunchKernelGGL(dns_size_kernel, dim3(grid), dim3(256), 0, s, A);
  hipLaunchKernelGGL(dns_sum_kernel, dim3(A.nblk, 2), dim3(256), 0, s, A);
  hipLaunchKernelGGL(dns_scan2_kernel, dim3(2), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(dns_apply_kernel, dim3(A.nblk, 2), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t tot[3] = {0, 0, 0};
  uint32_t cnt = 0;
  GPD_TRY(hipMemcpyAsync(tot, A.tot, 24, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipMemcpyAsync(&cnt, A.blk + A.nblk, 4, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  counts->msgs = cnt;
  counts->entries = tot[0];
  counts->name_bytes = tot[1];
  counts->deferred = tot[2];
  if (tot[0] > 0xFFFFFFFFull || tot[1] > 0xFFFFFFFFull)
    return set_error(GPD_ERR_INVALID, "%s: %llu entries, %llu name bytes: more than 2^32 - 1, split the batch", who,
                     (unsigned long long)tot[0], (unsigned long long)tot[1]);
  if (cnt > out->cap_msgs || tot[0] > out->cap_entries || tot[1] > out->cap_names)
    return set_error(GPD_ERR_INVALID,
                     "%s: %u messages, %llu entries, %llu name bytes; the capacities are %llu, %llu, %llu", who, cnt,
                     (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)out->cap_msgs,
                     (unsigned long long)out->cap_entries, (unsigned long long)out->cap_names);
  if (cnt == 0) return GPD_OK;
  const unsigned egrid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, ((uint64_t)cnt + 255u) / 256u);
  hipLaunchKernelGGL(dns_emit_kernel, dim3(egrid), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}

extern "C" int gpd_dns_decode_host(const uint8_t *data, uint32_t len, uint32_t max_work, gpd_dns_msg *msg,
                                   gpd_dns_entry *entries, uint64_t cap_entries, uint8_t *names, uint64_t cap_names,
                                   gpd_dns_counts *counts) {
  using namespace gpd;
  const char *who = "gpd_dns_decode_host";
  if ((!data && len) || !msg || !counts) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  if ((cap_entries && !entries) || (cap_names && !names))
    return set_error(GPD_ERR_INVALID, "%s: null array with a nonzero capacity", who);
  *counts = gpd_dns_counts{};
  *msg = gpd_dns_msg{};
  DnsWalk S;
  S.max_work = max_work;
  dns_walk(data, len, DnsCountSink{}, S, *msg);
  counts->msgs = 1;
  counts->entries = S.n_entries;
  counts->name_bytes = S.name_bytes;
  counts->deferred = msg->verdict == GPD_DNS_DEFERRED;
  counts->work = S.work;
  if (S.n_entries > cap_entries || S.name_bytes > cap_names)
    return set_error(GPD_ERR_INVALID, "%s: %u entries, %u name bytes; the capacities are %llu, %llu", who,
                     S.n_entries, S.name_bytes, (unsigned long long)cap_entries, (unsigned long long)cap_names);
  DnsWalk W;
  W.max_work = max_work;
  dns_walk(data, len, DnsStoreSink{entries, S.n_entries, names, S.name_bytes, 0u}, W, *msg);
  return GPD_OK;
}
