// gpd_staging.cpp — the two staging slots of a context and the host-memory path on them.
//
// A slot is one chunk in flight: pinned host buffers, their device twins, the result arrays
// (gpd_ctx.h lists them once; everything here loops over that list), streams and events.
// gpd_decode_host runs batches in host memory through the slots; the capture pipelines
// (gpd_capture.cpp) and the TPACKET_V3 device path (gpd_afpacket.cpp) use the same slots.
#include "gpd_ctx.h"

using namespace gpd;

void gpd::par_memcpy(uint8_t *dst, const uint8_t *src, uint64_t n, int nthreads) {
  const uint64_t kMin = 8ull << 20;
  int T = (int)std::min<uint64_t>((uint64_t)std::max(1, nthreads), std::max<uint64_t>(1, n / kMin));
  if (T <= 1) {
    std::memcpy(dst, src, n);
    return;
  }
  std::vector<std::thread> th;
  for (int k = 0; k < T; k++) {
    const uint64_t lo = n * (uint64_t)k / (uint64_t)T, hi = n * (uint64_t)(k + 1) / (uint64_t)T;
    th.emplace_back([=] { std::memcpy(dst + lo, src + lo, hi - lo); });
  }
  for (auto &t : th) t.join();
}

void gpd::free_slots(gpd_ctx *ctx) {
  if (ctx->tw_in) (void)hipStreamSynchronize(ctx->tw_in);
  for (auto &s : ctx->slot) {
    for (hipStream_t st : {s.stream, s.stream_out})
      if (st) (void)hipStreamSynchronize(st);
    for (void *p : {(void *)s.h_data, (void *)s.h_off, (void *)s.h_len, (void *)s.h_tw})
      if (p) (void)hipHostFree(p);
    for (void *p : {(void *)s.d_data, (void *)s.d_off, (void *)s.d_len, (void *)s.d_pw, (void *)s.d_tw})
      if (p) (void)hipFree(p);
    for (int a = 0; a < kNumRes; a++) {
      if (s.h_res[a]) (void)hipHostFree(s.h_res[a]);
      if (s.d_res[a]) (void)hipFree(s.d_res[a]);
    }
    for (hipStream_t st : {s.stream, s.stream_out})
      if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : {s.ev_in, s.ev_dec, s.ev_out})
      if (e) (void)hipEventDestroy(e);
    s = Slot{};
  }
  if (ctx->d_pw_ctl) (void)hipFree(ctx->d_pw_ctl);
  if (ctx->h_pw_ctl) (void)hipHostFree(ctx->h_pw_ctl);
  ctx->d_pw_ctl = ctx->h_pw_ctl = nullptr;
  if (ctx->tw_in) (void)hipStreamDestroy(ctx->tw_in);
  ctx->tw_in = nullptr;
  for (auto *ev : {ctx->ev_pw, ctx->ev_twin})
    for (int q = 0; q < 2; q++)
      if (ev[q]) (void)hipEventDestroy(ev[q]), ev[q] = nullptr;
  for (auto *ev : {ctx->ev_tw, ctx->ev_twdec})
    for (int q = 0; q < 4; q++)
      if (ev[q]) (void)hipEventDestroy(ev[q]), ev[q] = nullptr;
  ctx->slot_bytes = ctx->slot_pkts = 0;
}

int gpd::alloc_slots(gpd_ctx *ctx, uint64_t bytes, uint64_t pkts, bool ext, bool det) {
  const Slot &s0 = ctx->slot[0];
  if (ctx->slot_bytes >= bytes && ctx->slot_pkts >= pkts && (!ext || s0.d_res[kResExt]) &&
      (!det || s0.d_res[kResDetail]))
    return GPD_OK;
  ext = ext || s0.d_res[kResExt];  // (a re-allocation keeps what earlier calls asked for)
  det = det || s0.d_res[kResDetail];
  free_slots(ctx);
  // H2D, walk and decode on a slot's `stream`, the results' D2H of gpd_decode_host / gpd_decode_tpv3
  // on its `stream_out`, so the next chunks' H2D never waits behind a D2H.  (Both slots' streams
  // first: which streams share a hardware queue follows the order of creation.)
  for (auto &s : ctx->slot) HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  for (auto &s : ctx->slot) HIP_TRY(hipStreamCreateWithFlags(&s.stream_out, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&ctx->tw_in, hipStreamNonBlocking));
  for (auto &s : ctx->slot) {
    for (hipEvent_t *e : {&s.ev_in, &s.ev_dec, &s.ev_out}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc(&s.h_data, bytes + 64, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&s.d_data, bytes + 64));
    HIP_TRY(hipHostMalloc(&s.h_off, pkts * 4, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(&s.h_len, pkts * 4, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&s.d_off, pkts * 4));
    HIP_TRY(hipMalloc(&s.d_len, pkts * 4));
    for (int a = 0; a < kNumRes; a++) {
      if ((a == kResExt && !ext) || (a == kResDetail && !det)) continue;
      HIP_TRY(hipHostMalloc(&s.h_res[a], pkts * kResW.w[a], hipHostMallocDefault));
      HIP_TRY(hipMalloc(&s.d_res[a], pkts * kResW.w[a]));
    }
    HIP_TRY(hipMalloc(&s.d_pw, 5ull * gpd::kPwMaxSeg * 4));
  }
  HIP_TRY(hipMalloc(&ctx->d_pw_ctl, 2 * sizeof(gpd::PwCtl)));
  HIP_TRY(hipHostMalloc(&ctx->h_pw_ctl, 2 * sizeof(gpd::PwCtl), hipHostMallocDefault));
  for (auto *ev : {ctx->ev_pw, ctx->ev_twin})
    for (int q = 0; q < 2; q++) HIP_TRY(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming));
  for (auto *ev : {ctx->ev_tw, ctx->ev_twdec})
    for (int q = 0; q < 4; q++) HIP_TRY(hipEventCreateWithFlags(&ev[q], hipEventDisableTiming));
  ctx->slot_bytes = bytes;
  ctx->slot_pkts = pkts;
  return GPD_OK;
}

gpd_result gpd::slot_result(const Slot &s, const gpd_result *out) {
  const ResPtrs o = res_ptrs(*out);
  ResPtrs d;
  for (int a = 0; a < kNumRes; a++)
    if (res_wanted(o, a)) d.p[a] = s.d_res[a];
  return res_struct(d);
}

hipError_t gpd::results_d2h(gpd_ctx *ctx, Slot &s, const gpd_result *out, uint64_t lo, uint64_t m,
                            hipStream_t stream) {
  const ResPtrs o = res_ptrs(*out);
  s.direct = !o.p[kResExt];
  for (int a = 0; a < kNumRes && s.direct; a++)
    if (o.p[a]) s.direct = ctx->is_registered(o.p[a] + lo * kResW.w[a], m * kResW.w[a]);
  for (int a = 0; a < kNumRes; a++) {
    if (!o.p[a]) continue;
    void *host = s.direct ? o.p[a] + lo * kResW.w[a] : s.h_res[a];
    const hipError_t e = hipMemcpyAsync(host, s.d_res[a], m * kResW.w[a], hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

void gpd::drain_slot(Slot &s, const gpd_result *out) {
  const uint64_t m = s.hi - s.lo;
  if (!s.direct) {
    const ResPtrs o = res_ptrs(*out);
    par_for(m, 1u << 16, [&](uint64_t a, uint64_t b) {
      for (int r = 0; r < kNumRes; r++)
        if (o.p[r]) std::memcpy(o.p[r] + (s.lo + a) * kResW.w[r], s.h_res[r] + a * kResW.w[r], (b - a) * kResW.w[r]);
    });
  }
  s.busy = false;
}

int gpd::finish_slots(gpd_ctx *ctx, const gpd_result *out, double *sync_ms, double *drain_ms) {
  for (auto &s : ctx->slot) {  // (a chunk queued ahead and not needed is waited for and dropped)
    const double t0 = now_ms();
    HIP_TRY(hipStreamSynchronize(s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream_out));
    const double t1 = now_ms();
    if (s.busy) drain_slot(s, out);
    if (sync_ms) *sync_ms += t1 - t0;
    if (drain_ms) *drain_ms += now_ms() - t1;
  }
  return GPD_OK;
}

// ---- host-memory path: chunked, double-buffered pinned H2D -> decode -> D2H ----
extern "C" int gpd_decode_host(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *out) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_decode_host: null ctx");
  if (!in || !out || !out->status || !out->layers)
    return set_error(GPD_ERR_INVALID, "gpd_decode_host: null batch/result");
  if (in->n == 0) return GPD_OK;
  if (in->n > kMaxBatchPackets)
    return set_error(GPD_ERR_INVALID, "gpd_decode_host: batch of %llu packets (max 2^32 - 256)",
                     (unsigned long long)in->n);
  DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  const uint64_t kPkts = 1u << 20, kBytes = 256ull << 20;
  int rc = alloc_slots(ctx, kBytes, kPkts, out->ext != nullptr, out->detail != nullptr);
  if (rc) return rc;
  // Each slot's chunk: H2D and decode on its stream, the results D2H on its stream_out, so the
  // next chunks' H2D never waits behind a D2H (the link carries both directions at once)
  SlotGuard guard{ctx};
  uint64_t i = 0;
  int k = 0;
  while (i < in->n) {
    auto &s = ctx->slot[k];
    if (s.busy) HIP_TRY(hipEventSynchronize(s.ev_in));  // chunk k-2's H2D read the host staging
    // Span mode: packets [i, j) lie inside one window of the source buffer of at most kBytes
    // with few gaps (the usual back-to-back batch): that window travels as it is (straight
    // from the caller's buffer when it is registered) and the offsets are rebased.
    // Otherwise the packets are repacked 16-byte aligned into the slot.
    uint64_t j = i, used = 0;
    const uint64_t lo16 = std::min<uint64_t>(in->offset[i], in->data_len) & ~15ull;
    uint64_t span_hi = lo16;
    while (j < in->n && j - i < kPkts) {
      const uint64_t o = in->offset[j], e = o + in->caplen[j];
      if (o < lo16 || e > in->data_len || e - lo16 > kBytes) break;
      span_hi = std::max(span_hi, e);
      used += in->caplen[j];
      j++;
    }
    // (a registered window travels by DMA alone, so it may carry more gap — e.g. an AF_PACKET
    // ring's frame headers — before a 16-thread host repack of the packets would be cheaper)
    const bool reg = j > i && ctx->is_registered(in->data + lo16, span_hi - lo16);
    const bool span = j > i && (span_hi - lo16) <= (reg ? 4 : 2) * used + 4096;
    uint64_t pos = 0;
    // a span whose descriptors are registered too (a capture loop pins its arrays once): they
    // travel by DMA as they are, and the kernel reads the window through a base pointer moved
    // back by lo16, so the caller's absolute offsets index it — no host pass over the chunk
    bool dreg = false;
    if (span) {
      pos = span_hi - lo16;
      const uint64_t m = j - i;
      // (the kernel's buffer end lo16 + pos must stay in the 32-bit offset range; past 4 GiB the
      // offsets are rebased instead)
      dreg = lo16 + pos <= 0xFFFFFFF0ull && ctx->is_registered((const uint8_t *)(in->offset + i), m * 4) &&
             ctx->is_registered((const uint8_t *)(in->caplen + i), m * 4);
      if (!dreg)
        par_for(m, 1u << 16, [&](uint64_t a, uint64_t b) {
          for (uint64_t p = a; p < b; p++) s.h_off[p] = (uint32_t)(in->offset[i + p] - lo16);
          std::memcpy(s.h_len + a, in->caplen + i + a, (b - a) * 4);
        });
      // (not stage_h2d: this copy splits over the par_for threads at 4 MiB per thread, the
      // captures' over the caller's thread count at 8 MiB)
      const uint64_t bytes = std::min<uint64_t>((pos + 15) & ~15ull, ((in->data_len + 15) & ~15ull) - lo16);
      if (ctx->is_registered(in->data + lo16, bytes)) {
        HIP_TRY(hipMemcpyAsync(s.d_data, in->data + lo16, bytes, hipMemcpyHostToDevice, s.stream));
      } else {
        par_for(bytes, 4u << 20, [&](uint64_t a, uint64_t b) {
          std::memcpy(s.h_data + a, in->data + lo16 + a, b - a);
        });
        HIP_TRY(hipMemcpyAsync(s.d_data, s.h_data, bytes, hipMemcpyHostToDevice, s.stream));
      }
    } else {
      j = i;
      used = 0;
      while (j < in->n && j - i < kPkts) {
        const uint32_t len = in->caplen[j];
        const uint64_t need = ((used + 15) & ~15ull) + len;
        if (need > kBytes) break;
        used = need;
        j++;
      }
      if (j == i) return set_error(GPD_ERR_INVALID, "gpd_decode_host: packet %llu larger than %llu bytes",
                                   (unsigned long long)i, (unsigned long long)kBytes);
      for (uint64_t p = i; p < j; p++) {  // positions (cheap), then the copies in parallel
        pos = (pos + 15) & ~15ull;
        s.h_off[p - i] = (uint32_t)pos;
        s.h_len[p - i] = in->caplen[p];
        pos += in->caplen[p];
      }
      par_for(j - i, 1u << 14, [&](uint64_t a, uint64_t b) {
        for (uint64_t p = a; p < b; p++)
          std::memcpy(s.h_data + s.h_off[p], in->data + in->offset[i + p], s.h_len[p]);
      });
      HIP_TRY(hipMemcpyAsync(s.d_data, s.h_data, (pos + 15) & ~15ull, hipMemcpyHostToDevice, s.stream));
    }
    const uint64_t m = j - i;
    HIP_TRY(hipMemcpyAsync(s.d_off, dreg ? in->offset + i : s.h_off, m * 4, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipMemcpyAsync(s.d_len, dreg ? in->caplen + i : s.h_len, m * 4, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipEventRecord(s.ev_in, s.stream));
    if (s.busy) {  // chunk k-2's results are back (and drained) before this decode rewrites them
      HIP_TRY(hipEventSynchronize(s.ev_out));
      drain_slot(s, out);
    }
    gpd_batch b{s.d_data, pos, s.d_off, s.d_len, m};
    if (dreg) {
      b.data = s.d_data - lo16;  // 16-aligned (lo16 is); the kernel never reads below lo16
      b.data_len = lo16 + pos;
    }
    const gpd_result r = slot_result(s, out);
    rc = decode_launch(ctx, &b, &r, s.stream, false, nullptr, 0, pos);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.ev_dec, s.stream));
    HIP_TRY(hipStreamWaitEvent(s.stream_out, s.ev_dec, 0));
    HIP_TRY(results_d2h(ctx, s, out, i, m, s.stream_out));
    HIP_TRY(hipEventRecord(s.ev_out, s.stream_out));
    s.lo = i;
    s.hi = j;
    s.busy = true;
    i = j;
    k ^= 1;
  }
  return finish_slots(ctx, out);
}
