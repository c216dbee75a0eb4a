// gpd_tls.hip — the TLS record decode (include/gpd_tls.h): (*TLS).DecodeFromBytes
// (layers/tls.go:118-194) for every packet of a decoded device batch whose decode stopped at
// LayerTypeTLS, and for byte ranges of a device buffer (reassembled streams).  The walk itself is
// gpd_tls_walk.h, shared with the host entry point.
//
// Passes are separated by launch boundaries only; no kernel waits on another workgroup (no
// decoupled look-back, no spin on a global word).  For a batch the candidate count stays on the
// device until the one host synchronisation: every kernel after the compaction reads it from
// blk[nblk] and strides over the candidates.  For ranges every range is a message and the count
// is the caller's n.
//
//   tls_count_kernel    one lane per packet: is it a candidate?  (gpd_compact.h: mask bit, block count)
//   tls_scan_kernel     one workgroup: exclusive scan of the block counts
//   tls_index_kernel    the candidates' packet indices in order
//   tls_locate_kernel   one lane per candidate: where the message lies (gpd_locate.h, shared with
//                       gpd_dns.hip)
//     -- the ranges entry begins here: its index is the identity, its data the ranges --
//   tls_size_kernel     one lane per message: the walk with the counting sink; the message's
//                       record count, the deferred total, and for ranges the bounds test
//   tls_sum_kernel      per 2048 messages the sum of the record counts (gpd_stream_util.h scan_sum)
//   tls_scan2_kernel    one workgroup: compact_scan over the block sums
//   tls_apply_kernel    the counts -> exclusive prefixes in place (scan_apply), the total behind them
//     -- the host reads the totals, checks the capacities --
//   tls_emit_kernel     one lane per message: the walk again with the storing sink, and the
//                       message record
//
// A lane per message reads record headers from global memory, 5 to 7 bytes a record and a jump;
// a wave's 64 messages diverge, which is accepted.  The budget (gpd_tls_config.max_records)
// bounds what one lane can be made to do.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gpd_compact.h"
#include "gpd_dev_generic.h"
#include "gpd_locate.h"
#include "gpd_stream_util.h"
#include "gpd_tls_walk.h"
#include "../../include/gpd_tls.h"

namespace gpd {
namespace {

static_assert(sizeof(gpd_tls_msg) == 48 && sizeof(gpd_tls_rec) == 16, "include/gpd_tls.h layouts");
static_assert(offsetof(gpd_tls_msg, n_ccs) == 16 && offsetof(gpd_tls_msg, contents_off) == 32 &&
                  offsetof(gpd_tls_msg, verdict) == 40 && offsetof(gpd_tls_msg, truncated) == 41,
              "tls_emit_kernel packs the message record by these offsets");

struct TlsArgs {
  KParams P;                // the batch (gpd_tls_decode)
  gpd_tls_ranges R;         // the ranges (gpd_tls_decode_ranges)
  uint32_t max_records;
  gpd_tls_msg *msgs;        // the caller's
  gpd_tls_rec *recs;
  // scratch of the context
  uint32_t nblk;            // ceil(n / 2048): blocks of the compaction, and the bound of the count scan's
  uint32_t *blk;            // nblk + 1: per-block candidate counts -> exclusive prefix; [nblk] = candidates
  uint64_t *mask;           // one bit per packet
  uint32_t *idx;            // the candidates' packet indices in order
  uint32_t *d_off, *d_len;  // per candidate: where its message lies in the packet
  uint32_t *forced;         // per candidate: saturated offsets or layer count: deferred unwalked
  uint32_t *nr;             // per message (+1): records -> exclusive prefix; [cnt] = the total
  uint32_t *blk2;           // nblk + 1: block sums of nr
  uint64_t *tot;            // [0] records (exact), [1] deferred, [2] ranges that pass nbytes
};

// Packet i is a candidate when its decode stopped at LayerTypeTLS without an error.
__device__ __forceinline__ bool tls_candidate(const KParams &P, uint32_t i) {
  uint32_t st;
  uint64_t lw;
  if (P.rec) {
    st = P.rec[i].status;
    lw = P.rec[i].layers;
  } else {
    st = P.status[i];
    lw = P.layers[i];
  }
  return GPD_STATUS_CLASS(st) != GPD_ST_DECODE_ERROR && GPD_LAYERS_STOP(lw) == GPD_LT_TLS;
}

__global__ __launch_bounds__(256) void tls_count_kernel(TlsArgs A) {
  compact_count((uint32_t)A.P.n, A.mask, A.blk, [&A](uint32_t i) { return tls_candidate(A.P, i); });
}
__global__ __launch_bounds__(1024) void tls_scan_kernel(TlsArgs A) { compact_scan(A.blk, A.nblk); }
__global__ __launch_bounds__(64) void tls_index_kernel(TlsArgs A) {
  compact_index(A.blk, A.mask, A.idx, (uint32_t)A.P.n);
}
template <bool PAGES>
__global__ __launch_bounds__(256) void tls_locate_kernel(TlsArgs A) {
  locate_payloads<PAGES>(A.P, A.blk[A.nblk], A.idx, A.d_off, A.d_len, A.forced);
}

// Where message j's data comes from: the located payload of candidate j, or range j.
struct TlsData {
  const uint8_t *d;
  uint32_t len, packet, data_off;
  bool forced;  // deferred without a walk
  bool bad;     // a range that passes nbytes: never read
};

template <bool RANGES>
__device__ __forceinline__ uint32_t tls_msgs(const TlsArgs &A) {
  return RANGES ? (uint32_t)A.R.n : A.blk[A.nblk];
}

template <bool RANGES>
__device__ __forceinline__ TlsData tls_data(const TlsArgs &A, uint32_t j) {
  TlsData D;
  if (RANGES) {
    const uint64_t off = A.R.off[j];
    D.len = A.R.len[j];
    D.bad = off > A.R.nbytes || D.len > A.R.nbytes - off;
    D.d = A.R.bytes + (D.bad ? 0 : off);
    if (D.bad) D.len = 0;
    D.packet = j;
    D.data_off = 0;
    D.forced = false;
  } else {
    const KParams &P = A.P;
    const uint32_t dlen = (uint32_t)P.data_len;
    D.packet = A.idx[j];
    D.data_off = A.d_off[j];
    D.len = A.d_len[j];
    D.d = P.data + min(P.offset[D.packet], dlen) + D.data_off;
    D.forced = A.forced[j] != 0;
    D.bad = false;
  }
  return D;
}

template <class Sink>
__device__ __forceinline__ void tls_walk_msg(const TlsArgs &A, const TlsData &D, const Sink &sink, TlsWalk &W,
                                             gpd_tls_msg &m) {
  W.max_records = A.max_records;
  if (D.forced) tls_deferred(D.len, W, m);
  else tls_walk(D.d, D.len, sink, W, m);
}

template <bool RANGES>
__global__ __launch_bounds__(256) void tls_size_kernel(TlsArgs A) {
  const uint32_t cnt = tls_msgs<RANGES>(A);
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const TlsData D = tls_data<RANGES>(A, j);
    if (D.bad) {
      A.nr[j] = 0;
      atomicAdd(reinterpret_cast<unsigned long long *>(A.tot + 2), 1ull);
      continue;
    }
    TlsWalk W;
    gpd_tls_msg m;
    tls_walk_msg(A, D, TlsCountSink{}, W, m);
    A.nr[j] = W.n_records;
    if (m.verdict == GPD_TLS_DEFERRED) atomicAdd(reinterpret_cast<unsigned long long *>(A.tot + 1), 1ull);
  }
}

template <bool RANGES>
__global__ __launch_bounds__(256) void tls_sum_kernel(TlsArgs A) {
  const uint32_t *v = A.nr;
  scan_sum(tls_msgs<RANGES>(A), A.blk2, A.tot, [v](uint32_t j) { return v[j]; });
}
__global__ __launch_bounds__(1024) void tls_scan2_kernel(TlsArgs A) { compact_scan(A.blk2, A.nblk); }
template <bool RANGES>
__global__ __launch_bounds__(256) void tls_apply_kernel(TlsArgs A) {
  uint32_t *v = A.nr;
  scan_apply(tls_msgs<RANGES>(A), A.blk2, v, true, [v](uint32_t j) { return v[j]; });
}

// The capacities were checked on the host: msgs holds cnt records, recs nr[cnt]; no range is bad.
template <bool RANGES>
__global__ __launch_bounds__(256) void tls_emit_kernel(TlsArgs A) {
  const uint32_t cnt = tls_msgs<RANGES>(A);
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const TlsData D = tls_data<RANGES>(A, j);
    const uint32_t r0 = A.nr[j], r1 = A.nr[j + 1u];
    TlsWalk W;
    gpd_tls_msg m;
    tls_walk_msg(A, D, TlsStoreSink{A.recs + r0, r1 - r0}, W, m);
    // the record as three 16-byte stores (its last six bytes are reserved: zero)
    v4u *q = reinterpret_cast<v4u *>(A.msgs + j);
    q[0] = v4u{D.packet, D.data_off, m.data_len, r0};
    q[1] = v4u{m.n_ccs, m.n_handshake, m.n_appdata, m.n_alert};
    q[2] = v4u{m.contents_off, m.err_off, (uint32_t)m.verdict | ((uint32_t)m.truncated << 8), 0u};
  }
}

int tls_check_common(const char *who, const gpd_tls_config *cfg, const gpd_tls_out *out, uint64_t n,
                     uint32_t *max_records) {
  *max_records = cfg ? cfg->max_records : GPD_TLS_MAX_RECORDS_DEFAULT;
  if (*max_records < 1u || *max_records > GPD_TLS_MAX_RECORDS_LIMIT || (cfg && cfg->reserved))
    return set_error(GPD_ERR_INVALID, "%s: max_records %u outside 1..%u (or a nonzero reserved word)", who,
                     *max_records, GPD_TLS_MAX_RECORDS_LIMIT);
  if (n >= 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: %llu messages (max 2^32 - 257)", who, (unsigned long long)n);
  if ((out->cap_msgs && !out->msgs) || (out->cap_recs && !out->recs))
    return set_error(GPD_ERR_INVALID, "%s: null array with a nonzero capacity", who);
  if (((uintptr_t)out->msgs & 15u) || ((uintptr_t)out->recs & 15u))
    return set_error(GPD_ERR_INVALID, "%s: msgs and recs must be 16-byte aligned", who);
  return GPD_OK;
}

// From the sizing pass on: the same kernels for both entry points.  n: the items the scratch was
// carved for (packets, or ranges).
template <bool RANGES>
int tls_run(const char *who, gpd_ctx *ctx, TlsArgs &A, uint32_t n, const gpd_tls_out *out, gpd_tls_counts *counts,
            hipStream_t s) {
  const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, ((uint64_t)n + 255u) / 256u);
  hipLaunchKernelGGL(tls_size_kernel<RANGES>, dim3(grid), dim3(256), 0, s, A);
  hipLaunchKernelGGL(tls_sum_kernel<RANGES>, dim3(A.nblk), dim3(256), 0, s, A);
  hipLaunchKernelGGL(tls_scan2_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(tls_apply_kernel<RANGES>, dim3(A.nblk), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  uint64_t tot[3] = {0, 0, 0};
  uint32_t cnt = n;
  GPD_TRY(hipMemcpyAsync(tot, A.tot, 24, hipMemcpyDeviceToHost, s));
  if (!RANGES) GPD_TRY(hipMemcpyAsync(&cnt, A.blk + A.nblk, 4, hipMemcpyDeviceToHost, s));
  GPD_TRY(hipStreamSynchronize(s));
  if (tot[2])
    return set_error(GPD_ERR_INVALID, "%s: %llu of the %u ranges pass nbytes (%llu)", who, (unsigned long long)tot[2],
                     n, (unsigned long long)A.R.nbytes);
  counts->msgs = cnt;
  counts->records = tot[0];
  counts->deferred = tot[1];
  if (tot[0] > 0xFFFFFFFFull)
    return set_error(GPD_ERR_INVALID, "%s: %llu records: more than 2^32 - 1, split the batch", who,
                     (unsigned long long)tot[0]);
  if (cnt > out->cap_msgs || tot[0] > out->cap_recs)
    return set_error(GPD_ERR_INVALID, "%s: %u messages, %llu records; the capacities are %llu, %llu", who, cnt,
                     (unsigned long long)tot[0], (unsigned long long)out->cap_msgs,
                     (unsigned long long)out->cap_recs);
  if (cnt == 0) return GPD_OK;
  const unsigned egrid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, ((uint64_t)cnt + 255u) / 256u);
  hipLaunchKernelGGL(tls_emit_kernel<RANGES>, dim3(egrid), dim3(256), 0, s, A);
  GPD_TRY(hipGetLastError());
  GPD_TRY(hipStreamSynchronize(s));
  return GPD_OK;
}

}  // namespace
}  // namespace gpd

extern "C" int gpd_tls_decode(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res, const gpd_tls_config *cfg,
                              const gpd_tls_out *out, gpd_tls_counts *counts, void *stream) {
  using namespace gpd;
  const char *who = "gpd_tls_decode";
  if (!ctx || !in || !res || !out || !counts) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *counts = gpd_tls_counts{};
  uint32_t max_records = 0;
  if (int rc = tls_check_common(who, cfg, out, in->n, &max_records)) return rc;
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
  TlsArgs A{};
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
  A.max_records = max_records;
  A.msgs = out->msgs;
  A.recs = out->recs;
  // one carve of the context's scratch (the slot of the DNS decode and the TCP hand-off: a
  // context serves one call at a time, and every such call synchronises before it returns)
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
  uint32_t **arr[5] = {&A.idx, &A.d_off, &A.d_len, &A.forced, &A.nr};
  for (auto a : arr) {
    *a = reinterpret_cast<uint32_t *>(p);
    p += b_n;
  }
  const size_t lds = (P.image_words * 4u + 15u) & ~15u;
  const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)ctx_num_cus(ctx) * 8, ((uint64_t)n + 255u) / 256u);
  GPD_TRY(hipMemsetAsync(A.tot, 0, 32, s));
  hipLaunchKernelGGL(tls_count_kernel, dim3(A.nblk), dim3(256), 0, s, A);
  hipLaunchKernelGGL(tls_scan_kernel, dim3(1), dim3(1024), 0, s, A);
  hipLaunchKernelGGL(tls_index_kernel, dim3(A.nblk), dim3(64), 0, s, A);
  if (P.use_pages) hipLaunchKernelGGL(tls_locate_kernel<true>, dim3(grid), dim3(256), lds, s, A);
  else hipLaunchKernelGGL(tls_locate_kernel<false>, dim3(grid), dim3(256), lds, s, A);
  return tls_run<false>(who, ctx, A, n, out, counts, s);
}

extern "C" int gpd_tls_decode_ranges(gpd_ctx *ctx, const gpd_tls_ranges *ranges, const gpd_tls_config *cfg,
                                     const gpd_tls_out *out, gpd_tls_counts *counts, void *stream) {
  using namespace gpd;
  const char *who = "gpd_tls_decode_ranges";
  if (!ctx || !ranges || !out || !counts) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *counts = gpd_tls_counts{};
  uint32_t max_records = 0;
  if (int rc = tls_check_common(who, cfg, out, ranges->n, &max_records)) return rc;
  if (ranges->n == 0) return GPD_OK;
  if (!ranges->off || !ranges->len || (!ranges->bytes && ranges->nbytes))
    return set_error(GPD_ERR_INVALID, "%s: ranges bytes/off/len must be non-NULL", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  TlsArgs A{};
  A.R = *ranges;
  A.max_records = max_records;
  A.msgs = out->msgs;
  A.recs = out->recs;
  const uint32_t n = (uint32_t)ranges->n;
  A.nblk = (n + kCompactBlock - 1u) / kCompactBlock;
  const size_t b_blk = up16(((size_t)A.nblk + 1) * 4), b_n = up16(((size_t)n + 1) * 4);
  auto *base = static_cast<uint8_t *>(ctx_scratch(ctx, 15, 32 + b_blk + b_n));
  if (!base) return set_error(GPD_ERR_NOMEM, "%s: scratch allocation failed", who);
  A.tot = reinterpret_cast<uint64_t *>(base);
  A.blk2 = reinterpret_cast<uint32_t *>(base + 32);
  A.nr = reinterpret_cast<uint32_t *>(base + 32 + b_blk);
  GPD_TRY(hipMemsetAsync(A.tot, 0, 32, s));
  return tls_run<true>(who, ctx, A, n, out, counts, s);
}

extern "C" int gpd_tls_decode_host(const uint8_t *data, uint32_t len, uint32_t max_records, gpd_tls_msg *msg,
                                   gpd_tls_rec *recs, uint64_t cap_recs, gpd_tls_counts *counts) {
  using namespace gpd;
  const char *who = "gpd_tls_decode_host";
  if ((!data && len) || !msg || !counts) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  if (cap_recs && !recs) return set_error(GPD_ERR_INVALID, "%s: null array with a nonzero capacity", who);
  *counts = gpd_tls_counts{};
  TlsWalk S;
  S.max_records = max_records;
  tls_walk(data, len, TlsCountSink{}, S, *msg);
  counts->msgs = 1;
  counts->records = S.n_records;
  counts->deferred = msg->verdict == GPD_TLS_DEFERRED;
  counts->work = S.work;
  if (S.n_records > cap_recs)
    return set_error(GPD_ERR_INVALID, "%s: %u records; the capacity is %llu", who, S.n_records,
                     (unsigned long long)cap_recs);
  TlsWalk W;
  W.max_records = max_records;
  tls_walk(data, len, TlsStoreSink{recs, S.n_records}, W, *msg);
  return GPD_OK;
}
