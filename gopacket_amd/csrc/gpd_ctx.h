// gpd_ctx.h — the context behind the C-ABI, its staging slots and the one description of the
// per-packet result arrays.  Private to the host translation units (gpd_runtime.cpp,
// gpd_staging.cpp, gpd_capture.cpp, gpd_afpacket.cpp): not public ABI, and device code (.hip)
// does not include it (gpd::ctx_device / ctx_num_cus / ctx_scratch serve it).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "gpd_internal.h"

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return gpd::set_error(GPD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));    \
  } while (0)

namespace gpd {

// ---- the per-packet result arrays --------------------------------------------------------
// The one list of them: each array's index, its gpd_result member and its KParams member (the
// element width follows from the member's type).  Every loop over "the result arrays" in the
// host runtime goes through it; the order is the order of the device-to-host copies.  The
// first five are what every staged decode writes; hdr_off, ext and detail only when asked for.
enum Res { kResStatus, kResLayers, kResCsum, kResNetHash, kResTpHash, kResHdrOff, kResExt, kResDetail, kNumRes };
template <class F>
constexpr void for_each_result(F &&f) {
  f(kResStatus, &gpd_result::status, &KParams::status);
  f(kResLayers, &gpd_result::layers, &KParams::layers);
  f(kResCsum, &gpd_result::csum, &KParams::csum);
  f(kResNetHash, &gpd_result::net_hash, &KParams::net_hash);
  f(kResTpHash, &gpd_result::tp_hash, &KParams::tp_hash);
  f(kResHdrOff, &gpd_result::hdr_off, &KParams::hdr_off);
  f(kResExt, &gpd_result::ext, &KParams::ext);
  f(kResDetail, &gpd_result::detail, &KParams::detail);
}
struct ResWidths { uint64_t w[kNumRes]; };
constexpr ResWidths res_widths() {
  ResWidths W{};
  for_each_result([&W](int a, auto rm, auto) { W.w[a] = sizeof(*(std::declval<gpd_result &>().*rm)); });
  return W;
}
constexpr ResWidths kResW = res_widths();  // element bytes per array

// A gpd_result's arrays by index, as byte pointers (NULL: absent).
struct ResPtrs { uint8_t *p[kNumRes] = {}; };
inline ResPtrs res_ptrs(const gpd_result &r) {
  ResPtrs v;
  for_each_result([&](int a, auto rm, auto) { v.p[a] = reinterpret_cast<uint8_t *>(r.*rm); });
  return v;
}
inline gpd_result res_struct(const ResPtrs &v, gpd_record *records = nullptr) {
  gpd_result r{};
  for_each_result([&](int a, auto rm, auto) {
    r.*rm = reinterpret_cast<std::remove_reference_t<decltype(r.*rm)>>(v.p[a]);
  });
  r.records = records;
  return r;
}
inline void res_to_kparams(KParams &P, const gpd_result &r) {
  for_each_result([&](int, auto rm, auto km) { P.*km = r.*rm; });
  P.rec = r.records;
}
// Staged decodes give the kernel the five core arrays always and the others when `o` has them.
inline bool res_wanted(const ResPtrs &o, int a) { return a < kResHdrOff || o.p[a] != nullptr; }
// `out` with every result array (and records) moved on by d packets.
inline gpd_result shifted(const gpd_result *out, uint64_t d) {
  ResPtrs v = res_ptrs(*out);
  for (int a = 0; a < kNumRes; a++)
    if (v.p[a]) v.p[a] += d * kResW.w[a];
  return res_struct(v, out->records ? out->records + d : nullptr);
}

// Largest batch of one call: packet indices and (n + 63) / 64 stay 32-bit (gpd.h gpd_batch).
constexpr uint64_t kMaxBatchPackets = 0xFFFFFF00ull;

// nthreads <= 0: the machine's cores, at most 16.
inline int default_threads(int nthreads) {
  return nthreads > 0 ? nthreads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
}
inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Host-side copies of the staging pipeline run on up to 16 threads: fn(lo, hi) over [0, n).
template <class F>
void par_for(uint64_t n, uint64_t grain, F fn) {
  static const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const uint64_t T = std::min<uint64_t>(hw, (n + grain - 1) / grain);
  if (T <= 1) {
    fn(0, n);
    return;
  }
  std::vector<std::thread> th;
  for (uint64_t t = 1; t < T; t++) th.emplace_back([&, t] { fn(n * t / T, n * (t + 1) / T); });
  fn(0, n / T);
  for (auto &x : th) x.join();
}
// memcpy split over threads (the staging copy of an unregistered capture)
void par_memcpy(uint8_t *dst, const uint8_t *src, uint64_t n, int nthreads);

// One of the two staging slots of a context (alloc_slots / free_slots, gpd_staging.cpp).
struct Slot {
  hipStream_t stream = nullptr;      // H2D, walk and decode
  hipStream_t stream_out = nullptr;  // the D2H of gpd_decode_host and gpd_decode_tpv3
  uint8_t *h_data = nullptr, *d_data = nullptr;
  uint32_t *h_off = nullptr, *h_len = nullptr, *d_off = nullptr, *d_len = nullptr;
  uint8_t *h_res[kNumRes] = {}, *d_res[kNumRes] = {};  // result arrays (ext, detail: when asked for)
  uint32_t *d_pw = nullptr;  // the device pcap walk's per-segment arrays (5 x kPwMaxSeg)
  uint8_t *d_tw = nullptr, *h_tw = nullptr;  // the device TPACKET_V3 walk's tables + results (lazy)
  // gpd_decode_host: the chunk's H2D done (host staging reusable), decoded, results back
  hipEvent_t ev_in = nullptr, ev_dec = nullptr, ev_out = nullptr;
  uint64_t lo = 0, hi = 0;  // packet range in flight
  bool busy = false;
  bool direct = false;      // its results go straight into the caller's (registered) arrays
};

}  // namespace gpd

struct gpd_ctx {
  using Slot = gpd::Slot;
  int device = 0;
  int num_cus = 256;
  uint32_t first = GPD_LT_ETHERNET;
  uint32_t decoders = GPD_DEC_ALL;
  uint32_t options = 0;
  // the dispatch tables last loaded (LayerType values): AddDecodingLayer rebuilds the LDS image
  // from them, as the reference's parser reads the live tables at each decode
  std::vector<uint16_t> t_eth, t_proto, t_tcp, t_udp;
  uint32_t *d_image = nullptr;  // LUT + ipproto (+ hashes)
  uint16_t *d_pages = nullptr;  // PAGES fallback
  uint32_t image_words = 0, use_pages = 0;
  uint32_t eth_base = 0, tcp_base = 0, udp_base = 0, eth_bits = 0, tcp_bits = 0, udp_bits = 0;
  uint32_t eth_mult = 0, tcp_mult = 0, udp_mult = 0;
  bool fixed = false;  // tables in the fixed layout the fast kernel compiles in
  // fast-kernel fallback lists, one per stream the context is used on (count + indices)
  struct Fallback {
    uint32_t *d = nullptr;   // two flags (words 0 and 64), then the list
    uint32_t *wc = nullptr;  // two arrays of per-wave counts (one per parity)
    uint64_t cap = 0;
    uint32_t parity = 0;
  };
  std::map<hipStream_t, Fallback> fallback;
  // device scratch that grows on demand and lives with the context (ctx_scratch)
  struct Scratch {
    void *d = nullptr;
    size_t bytes = 0;
  } scratch[18];
  gpd_tuning tune{0, -1, -1, 0, -1, -1, 0, -1};  // gpd_ctx_set_tuning (all automatic by default)
  bool timing = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr;
  bool timed = false;
  bool timed_split = false;           // evm marks the fast kernel's end in the timed launch
  const uint32_t *timed_fb_wc = nullptr;  // its per-wave fallback counts (device)
  uint32_t timed_fb_waves = 0;
  // staging (two slots; a third measured 6-9 % slower on config 2's host path, r04)
  Slot slot[2];
  uint64_t slot_bytes = 0, slot_pkts = 0;
  gpd::PwCtl *d_pw_ctl = nullptr, *h_pw_ctl = nullptr;  // one control block per slot
  hipEvent_t ev_pw[2] = {nullptr, nullptr};            // a slot's chunk walked (and its block read back)
  hipStream_t tw_in = nullptr;  // TPACKET_V3 groups' bytes H2D, one after another
  hipEvent_t ev_tw[4] = {};     // TPACKET_V3 group k & 3's results back
  hipEvent_t ev_twdec[4] = {};  // ... decoded
  hipEvent_t ev_twin[2] = {};   // a slot's group bytes H2D done (its staging copy reusable)
  // host ranges pinned with gpd_host_register (H2D reads them in place)
  std::vector<std::pair<const uint8_t *, uint64_t>> registered;
  bool is_registered(const uint8_t *p, uint64_t n) const {
    for (const auto &r : registered)
      if (p >= r.first && p + n <= r.first + r.second) return true;
    return false;
  }
};

namespace gpd {

// The decode launch (gpd_runtime.cpp).  n_dev: the packet count is read on the device (at most
// in->n); geom_n: the packet count the staging choices assume (0: in->n) — both for batches
// whose records the device walk found; geom_bytes: likewise for the bytes (0: in->data_len).
int decode_launch(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *out, hipStream_t stream, bool record,
                  const uint32_t *n_dev = nullptr, uint64_t geom_n = 0, uint64_t geom_bytes = 0);

// ---- the staging slots (gpd_staging.cpp) ---------------------------------------------------
// Both slots with room for `bytes` and `pkts` (ext / det: with those arrays), their streams and
// events, the device walks' control blocks and the TPACKET_V3 copy stream; free_slots mirrors it.
int alloc_slots(gpd_ctx *ctx, uint64_t bytes, uint64_t pkts, bool ext, bool det);
void free_slots(gpd_ctx *ctx);
// The slot's device arrays as the decode's gpd_result (res_wanted of what `out` asks for).
gpd_result slot_result(const Slot &s, const gpd_result *out);
// Results of packets [lo, lo + m) device -> host on `stream`: straight into the caller's
// arrays when every one of them lies in registered memory (gpd_host_register; then the drain
// copies nothing; ext never goes direct), else into the slot's pinned arrays for drain_slot.
hipError_t results_d2h(gpd_ctx *ctx, Slot &s, const gpd_result *out, uint64_t lo, uint64_t m, hipStream_t stream);
// The slot's results (packets [s.lo, s.hi)) into `out`, unless they went direct; the slot is idle.
void drain_slot(Slot &s, const gpd_result *out);
// The end of a pipeline: both slots' streams waited for, every busy slot drained.  The time
// spent waiting and draining is added to *sync_ms / *drain_ms (may be NULL).
int finish_slots(gpd_ctx *ctx, const gpd_result *out, double *sync_ms = nullptr, double *drain_ms = nullptr);

// `bytes` at src into the slot's device buffer on `stream`: read in place when they lie in
// registered memory, else copied (in parallel) into the slot's pinned buffer first — after
// wait(), the caller's wait for whatever may still read that buffer (it differs per pipeline).
template <class Wait>
hipError_t stage_h2d(gpd_ctx *ctx, Slot &s, const uint8_t *src, uint64_t bytes, int nthreads, hipStream_t stream,
                     Wait wait) {
  if (!ctx->is_registered(src, bytes)) {
    const hipError_t e = wait();
    if (e != hipSuccess) return e;
    par_memcpy(s.h_data, src, bytes, nthreads);
    src = s.h_data;
  }
  return hipMemcpyAsync(s.d_data, src, bytes, hipMemcpyHostToDevice, stream);
}

// Error exits of the staged paths leave no slot in flight: every busy slot is waited for and
// dropped (its results belong to the failed call and are not drained anywhere), so the next
// call on the context starts from idle slots.  On success every slot was drained already.
struct SlotGuard {
  gpd_ctx *ctx;
  ~SlotGuard() {
    for (auto &s : ctx->slot)
      if (s.busy) {
        (void)hipStreamSynchronize(ctx->tw_in);
        (void)hipStreamSynchronize(s.stream);
        (void)hipStreamSynchronize(s.stream_out);
        s.busy = false;
      }
  }
};

}  // namespace gpd
