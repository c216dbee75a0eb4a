// gpd_capture.cpp — captures in host memory through the staging slots (gpd_staging.cpp): the
// pcap host walk, the chunk pipeline of the device walks (pcap and pcapng), the decode entry
// points of include/gpd_pcap.h and include/gpd_pcapng.h and their last-call diagnostics.
#include <string>

#include "gpd_ctx.h"
#include "gpd_pcapng_internal.h"

using gpd::now_ms;
using gpd::set_error;
using gpd::shifted;

// ---- pcap capture in host memory: index, then raw-byte chunks H2D -> decode -> D2H ----
// Host-clock phases of this thread's last gpd_decode_pcap(_at) call (gpd_decode_pcap_last_times).
static thread_local double g_pt_walk = 0, g_pt_walkwait = 0, g_pt_stage = 0, g_pt_sync = 0, g_pt_drain = 0,
                           g_pt_total = 0;
// ... and its device-walk chunks: walked, handed to the host, and the reasons (PwCtl::status bits)
static thread_local uint32_t g_pw_counts[7];
static thread_local uint64_t g_pw_miss[2] = {~0ull, ~0ull};  // the last refuted speculation: start, segment

extern "C" {

int gpd_decode_pcap(gpd_ctx *ctx, const uint8_t *buf, uint64_t len, uint64_t max_n,
                    const gpd_result *out, uint64_t *n_out, uint64_t *next_pos, int *stop,
                    int nthreads) {
  if (!ctx || !buf) return set_error(GPD_ERR_INVALID, "gpd_decode_pcap: null argument");
  gpd_pcap_info info;
  const int rc = gpd_pcap_header(buf, len, &info);
  if (rc) return rc;
  return gpd_decode_pcap_at(ctx, buf, len, &info, GPD_PCAP_HEADER_BYTES, max_n, out, n_out, next_pos, stop,
                            nthreads);
}

// The pcap path with the record walk on the host (gpd_pcap.cpp), one part ahead of the chunks.
static int decode_pcap_host_walk(gpd_ctx *ctx, const uint8_t *buf, uint64_t len, const gpd_pcap_info *info,
                                 uint64_t pos, uint64_t max_n, const gpd_result *out, uint64_t *n_out,
                                 uint64_t *next_pos, int *stop, int nthreads) {
  *n_out = 0;
  if (next_pos) *next_pos = pos;
  if (stop) *stop = GPD_PCAP_STOP_LIMIT;
  if (max_n == 0) return GPD_OK;
  const uint64_t kPkts = 1u << 20;
  // staging chunks of up to 256 MiB; slots of 64 MiB or more that the device walk already holds
  // serve as they are when a record fits them (a stretch the device walk hands over: pinned
  // slots re-allocated in the middle of a replay cost ~130 ms, r04)
  const uint64_t kBytes = ctx->slot_bytes >= (64ull << 20) && ctx->slot_bytes >= 64ull + info->snaplen
                              ? std::min<uint64_t>(ctx->slot_bytes, 256ull << 20) : 256ull << 20;
  const uint64_t kPart = 1u << 21;  // records per walked part (the first, walked before any
  const uint64_t kPart0 = 1u << 19; // transfer can start, is smaller)
  int rc = gpd::alloc_slots(ctx, kBytes, kPkts, false, out->detail != nullptr);
  if (rc) return rc;
  gpd::SlotGuard guard{ctx};
  // The record walk runs one part (kPart records) ahead of the transfers, on a helper thread:
  // while part q's chunks travel and decode, part q+1 is walked.  Two parts' record positions
  // and capture lengths are kept per calling thread across calls (a replay or capture loop
  // calls again and again; fresh pages for 12 B per record would cost more than the walk).
  struct Part {
    gpd::PcapResult W;
    std::vector<uint64_t> rp;
    std::vector<uint32_t> rcap;
    int rc = 0;
    std::string err;
  };
  static thread_local Part part[2];
  double walk_ms = 0;  // (written by the walking thread, read after its join)
  auto walk_part = [&](Part &P, uint64_t at, uint64_t m) {
    const double t0 = now_ms();
    if (P.rp.size() < m) {
      P.rp.resize(m);
      P.rcap.resize(m);
    }
    gpd::PcapOut o;  // positions and capture lengths only (what a decode needs)
    o.pos64 = P.rp.data();
    o.cap = P.rcap.data();
    P.rc = gpd::pcap_index_flat(buf, len, *info, at, m, nthreads, o, P.W);
    P.err = P.rc ? std::string(gpd_last_error_string()) : std::string();  // (the walker's thread)
    walk_ms += now_ms() - t0;
  };
  uint64_t done = 0;  // records decoded (the output index of the next one)
  int q = 0;
  walk_part(part[0], pos, std::min(kPart0, max_n));
  struct Joiner {  // every exit, errors included, waits for the walk running ahead
    std::thread t;
    ~Joiner() {
      if (t.joinable()) t.join();
    }
  } ahead;
  int k = 0;
  for (;;) {
    Part &cur = part[q];
    const uint64_t n = cur.W.n;
    const bool more = cur.rc == GPD_OK && cur.W.stop == GPD_PCAP_STOP_LIMIT && n > 0 && done + n < max_n;
    if (more)  // walk the next part while this one is staged
      ahead.t = std::thread(walk_part, std::ref(part[q ^ 1]), cur.W.next_pos, std::min(kPart, max_n - done - n));
    uint64_t i = 0;
    while (i < n) {
      auto &s = ctx->slot[k];
      if (s.busy) {
        const double t0 = now_ms();
        HIP_TRY(hipStreamSynchronize(s.stream));
        const double t1 = now_ms();
        gpd::drain_slot(s, out);
        g_pt_sync += t1 - t0;
        g_pt_drain += now_ms() - t1;
      }
      const double t_stage = now_ms();
      // records [i, j) whose bytes (from the first one's data, rounded down to 16) fit the slot
      const uint64_t base = (cur.rp[i] + GPD_PCAP_RECORD_BYTES) & ~15ull;
      uint64_t j = i;
      while (j < n && j - i < kPkts && cur.rp[j] + GPD_PCAP_RECORD_BYTES + cur.rcap[j] - base <= kBytes) j++;
      if (j == i)
        return set_error(GPD_ERR_INVALID, "gpd_decode_pcap: record %llu larger than %llu bytes",
                         (unsigned long long)(done + i), (unsigned long long)kBytes);
      const uint64_t m = j - i;
      const uint64_t end = cur.rp[j - 1] + GPD_PCAP_RECORD_BYTES + cur.rcap[j - 1];
      const uint64_t span = end - base;
      // (plain pointers: the worker threads would see their own thread_local vectors)
      const uint64_t *RP = cur.rp.data() + i;
      const uint32_t *RC = cur.rcap.data() + i;
      gpd::par_for(m, 1u << 16, [&](uint64_t a, uint64_t b) {
        for (uint64_t p = a; p < b; p++) s.h_off[p] = (uint32_t)(RP[p] + GPD_PCAP_RECORD_BYTES - base);
        std::memcpy(s.h_len + a, RC + a, (b - a) * 4);
      });
      // (a shard registers only its own bytes; the slot was waited for above: nothing to wait for)
      hipError_t e = gpd::stage_h2d(ctx, s, buf + base, span, nthreads, s.stream, [] { return hipSuccess; });
      if (e == hipSuccess) e = hipMemcpyAsync(s.d_off, s.h_off, m * 4, hipMemcpyHostToDevice, s.stream);
      if (e == hipSuccess) e = hipMemcpyAsync(s.d_len, s.h_len, m * 4, hipMemcpyHostToDevice, s.stream);
      if (e != hipSuccess) return set_error(GPD_ERR_HIP, "gpd_decode_pcap: H2D: %s", hipGetErrorString(e));
      gpd_batch b{s.d_data, span, s.d_off, s.d_len, m};
      const gpd_result r = gpd::slot_result(s, out);
      rc = gpd::decode_launch(ctx, &b, &r, s.stream, false);
      if (rc) return rc;
      e = gpd::results_d2h(ctx, s, out, done + i, m, s.stream);
      if (e != hipSuccess) return set_error(GPD_ERR_HIP, "gpd_decode_pcap: D2H: %s", hipGetErrorString(e));
      g_pt_stage += now_ms() - t_stage;
      s.lo = done + i;
      s.hi = done + j;
      s.busy = true;
      i = j;
      k ^= 1;
    }
    done += n;
    *n_out = done;
    if (next_pos) *next_pos = cur.W.next_pos;
    if (stop) *stop = cur.W.stop;
    if (!more) {
      if (cur.rc) {  // the walk stopped at a record the reference rejects: decode what preceded it
        if ((rc = gpd::finish_slots(ctx, out))) return rc;
        return set_error(cur.rc, "%s", cur.err.c_str());
      }
      break;
    }
    const double tj = now_ms();
    ahead.t.join();
    g_pt_walkwait += now_ms() - tj;
    q ^= 1;
  }
  if ((rc = gpd::finish_slots(ctx, out, &g_pt_sync, &g_pt_drain))) return rc;
  g_pt_walk += walk_ms;
  return GPD_OK;
}

}  // extern "C"

// The chunk pipeline of the device walks (gpd_segwalk.h; pcap and pcapng): the capture travels
// in fixed byte chunks (plus a margin: the longest record or block past them) on two slots,
// each chunk's packets are found in HBM (the walk of chunk k waits for chunk k-1's, which hands
// it its first header), decoded there, and their results copied back.  The host reads one
// control block per chunk: how many packets it held and how its walk ended.
template <class Args>
struct SegFormat {
  const char *what;                // the error texts' prefix
  uint64_t chunk, margin;          // bytes a chunk owns; bytes past them that travel with it
  uint64_t cap_pkts;               // packets a chunk can hold
  uint64_t mean;                   // the mean record or block size (the decode's staging choices)
  Args state;                      // the format's fields (the chunk's are filled in here)
  hipError_t (*walk)(const Args &, hipStream_t);
  hipError_t (*fill)(const Args &, hipStream_t);
};
struct SegChunk {                  // a walked chunk, as the format's on_chunk sees it
  gpd::PwCtl c;                    // its control block
  uint64_t B, entry, own;          // its base, its first header (relative), the bytes it owns
  bool last;                       // it ends the capture
  uint64_t take, done;             // packets taken from it; packets taken so far, those included
  gpd_ctx::Slot *slot;             // where its arrays lie
};
// Walks from `pos` until on_chunk(chunk, &more) leaves `more` false (or fails); on_chunk sees
// every walked chunk after its results (none when the chunk is the host's: status & 1) are on
// their way back.  *handled packets were decoded into `out`.
template <class Args, class OnChunk>
static int seg_device_walk(gpd_ctx *ctx, const uint8_t *buf, uint64_t len, uint64_t pos, uint64_t max_n,
                           const gpd_result *out, int nthreads, const SegFormat<Args> &F, OnChunk on_chunk,
                           uint64_t *handled) {
  *handled = 0;
  int rc = gpd::alloc_slots(ctx, std::max<uint64_t>(ctx->slot_bytes, F.chunk + F.margin + 64),
                       std::max<uint64_t>(ctx->slot_pkts, F.cap_pkts), false, out->detail != nullptr);
  if (rc) return rc;
  gpd::SlotGuard guard{ctx};
  // Chunk k's work on slot k & 1: its bytes H2D, then (after chunk k-1's walk) its walk, its
  // control block back to the host, its fill and its decode.  The next chunk is queued before
  // the host waits for this one's count, so the copy engine never waits for a walk.
  auto issue = [&](int k, uint64_t B, uint64_t entry0) -> int {
    auto &s = ctx->slot[k & 1];
    if (s.busy) {
      HIP_TRY(hipStreamSynchronize(s.stream));
      gpd::drain_slot(s, out);
    }
    const uint64_t own = std::min<uint64_t>(F.chunk, len - B);
    const uint64_t T = std::min<uint64_t>(own + F.margin, len - B);
    const bool last = B + own >= len;
    gpd::PwCtl *dc = ctx->d_pw_ctl + (k & 1), *hc = ctx->h_pw_ctl + (k & 1);
    HIP_TRY(gpd::stage_h2d(ctx, s, buf + B, T, nthreads, s.stream, [&] {
      return hipStreamSynchronize(s.stream);  // (its staging buffer may still be read)
    }));
    if (k == 0) {
      hc->entry = (uint32_t)entry0;
      HIP_TRY(hipMemcpyAsync(&dc->entry, &hc->entry, 4, hipMemcpyHostToDevice, s.stream));
    } else {
      HIP_TRY(hipStreamWaitEvent(s.stream, ctx->ev_pw[(k - 1) & 1], 0));
    }
    Args A = F.state;
    A.d = s.d_data;
    A.T = (uint32_t)T;
    A.own_end = (uint32_t)own;
    A.nseg = (uint32_t)((own + gpd::kPwSeg - 1) / gpd::kPwSeg);
    A.last = last;
    A.ctl = dc;
    A.ctl_next = last ? nullptr : ctx->d_pw_ctl + ((k + 1) & 1);
    A.st = s.d_pw;
    A.ex = s.d_pw + gpd::kPwMaxSeg;
    A.ct = s.d_pw + 2 * gpd::kPwMaxSeg;
    A.bad = s.d_pw + 3 * gpd::kPwMaxSeg;
    A.base = s.d_pw + 4 * gpd::kPwMaxSeg;
    A.off = s.d_off;
    A.len = s.d_len;
    hipError_t e = F.walk(A, s.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hc, dc, sizeof(gpd::PwCtl), hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess) e = hipEventRecord(ctx->ev_pw[k & 1], s.stream);
    if (e == hipSuccess) e = F.fill(A, s.stream);
    if (e != hipSuccess) return set_error(GPD_ERR_HIP, "%s: device walk: %s", F.what, hipGetErrorString(e));
    gpd_batch b{s.d_data, T, s.d_off, s.d_len, F.cap_pkts};
    const gpd_result r = gpd::slot_result(s, out);
    return gpd::decode_launch(ctx, &b, &r, s.stream, false, &dc->n, std::max<uint64_t>(1, own / F.mean));
  };
  uint64_t B = pos & ~15ull;  // chunk base (16-byte aligned: the decoder's batch buffer)
  uint64_t entry = pos - B;   // its first header
  uint64_t done = 0;
  rc = issue(0, B, entry);
  if (rc) return rc;
  for (int k = 0;; k++) {
    auto &s = ctx->slot[k & 1];
    const uint64_t own = std::min<uint64_t>(F.chunk, len - B);
    const bool last = B + own >= len;
    // queue the next chunk now unless this one should end the call (its packets, estimated
    // from the mean size, cover what is left)
    const bool ahead = !last && done + own / F.mean < max_n;
    if (ahead && (rc = issue(k + 1, B + own, 0))) return rc;
    HIP_TRY(hipEventSynchronize(ctx->ev_pw[k & 1]));  // chunk k walked: its count
    const gpd::PwCtl c = ctx->h_pw_ctl[k & 1];
    uint64_t take = 0;
    if (!(c.status & 1u)) {  // (else the host walks from this chunk's entry: its decode saw 0 packets)
      take = std::min<uint64_t>(c.n, max_n - done);
      hipError_t e = gpd::results_d2h(ctx, s, out, done, take, s.stream);
      if (e != hipSuccess) return set_error(GPD_ERR_HIP, "%s: D2H: %s", F.what, hipGetErrorString(e));
      s.lo = done;
      s.hi = done + take;
      s.busy = take > 0;
      done += take;
    }
    bool more = false;
    if ((rc = on_chunk(SegChunk{c, B, entry, own, last, take, done, &s}, &more))) return rc;
    if (!more) break;
    entry = c.next - own;
    B += own;
    if (!ahead && (rc = issue(k + 1, B, 0))) return rc;
  }
  if ((rc = gpd::finish_slots(ctx, out))) return rc;
  *handled = done;
  return GPD_OK;
}

extern "C" {

// The pcap path with the record walk on the device (gpd_pcapwalk.hip): chunks of 64 MiB.
// *handled records were decoded; *resume is the record header where the host walk must take
// over (a chunk with status 1: a rejected record, a partial record at the end, a speculation
// the walk missed), UINT64_MAX when the call is complete.
static int decode_device_walk(gpd_ctx *ctx, const uint8_t *buf, uint64_t len, const gpd_pcap_info &I,
                                   uint64_t pos, uint64_t max_n, const gpd_result *out, int nthreads,
                                   uint64_t *handled, uint64_t *resume, uint64_t *next_pos, int *stop,
                                   bool *ineligible) {
  SegFormat<gpd::PwArgs> F{"gpd_decode_pcap"};
  F.chunk = (uint64_t)gpd::kPwSeg * gpd::kPwMaxSeg;
  F.margin = (16ull + I.snaplen + 31ull) & ~15ull;  // the longest record past a chunk
  F.cap_pkts = F.chunk / GPD_PCAP_RECORD_BYTES;     // records a chunk can hold
  *handled = 0;
  *resume = pos;
  // (records that long, or a capture whose first records cannot be indexed: the host walk,
  // for the rest of the call — *ineligible)
  *ineligible = true;
  if (I.snaplen > (16u << 20)) return GPD_OK;
  // the mean record size: the first records, walked here
  {
    uint64_t sp[64];
    uint32_t sc[64];
    gpd::PcapOut o;
    o.pos64 = sp;
    o.cap = sc;
    gpd::PcapResult R;
    if (gpd::pcap_index_flat(buf, len, I, pos, 64, 1, o, R) != GPD_OK || R.n == 0) return GPD_OK;
    F.mean = std::max<uint64_t>(16, (R.next_pos - pos) / R.n);
  }
  *ineligible = false;
  F.state.snaplen = I.snaplen;
  F.state.be = I.big_endian != 0;
  F.state.nano = I.nano != 0;
  F.walk = gpd::launch_pcap_walk;
  F.fill = gpd::launch_pcap_fill;
  *resume = UINT64_MAX;
  return seg_device_walk(ctx, buf, len, pos, max_n, out, nthreads, F, [&](const SegChunk &k, bool *more) -> int {
    const gpd::PwCtl &c = k.c;
    g_pw_counts[0]++;
    g_pw_counts[6] += c.pad[0];
    if (c.miss_at != 0xFFFFFFFFu) {
      g_pw_miss[0] = k.B + c.miss_st;
      g_pw_miss[1] = k.B + (uint64_t)c.miss_at * gpd::kPwSeg;
    }
    if (c.status != 0) {  // the host walks from this chunk's entry
      g_pw_counts[1]++;
      for (int b = 0; b < 4; b++) g_pw_counts[2 + b] += (c.status >> (b + 1)) & 1u;
      *resume = k.B + k.entry;
    } else if (k.take < c.n) {  // the bound falls inside this chunk: the header of the record after it
      auto &s = *k.slot;
      HIP_TRY(hipMemcpyAsync(s.h_off, s.d_off + k.take, 4, hipMemcpyDeviceToHost, s.stream));
      HIP_TRY(hipStreamSynchronize(s.stream));
      if (next_pos) *next_pos = k.B + s.h_off[0] - GPD_PCAP_RECORD_BYTES;
      if (stop) *stop = GPD_PCAP_STOP_LIMIT;
    } else if (k.done == max_n) {
      if (next_pos) *next_pos = k.B + c.next;
      if (stop) *stop = GPD_PCAP_STOP_LIMIT;
    } else if (k.last) {  // status 0 on the last chunk: the walk ended exactly at the capture's end
      if (next_pos) *next_pos = len;
      if (stop) *stop = GPD_PCAP_STOP_EOF;
    } else {
      *more = true;
    }
    return GPD_OK;
  }, handled);
}

// Records whose header starts in [pos, pos + span), as the ReadPacketData loop finds them, up to
// the first one it would reject (the host walk then stops there with the reference's error).
static uint64_t count_records(const uint8_t *buf, uint64_t len, const gpd_pcap_info &I, uint64_t pos,
                              uint64_t span, uint64_t max_n) {
  auto rd = [&](uint64_t p) {
    uint32_t v;
    std::memcpy(&v, buf + p, 4);
    return I.big_endian ? __builtin_bswap32(v) : v;
  };
  uint64_t n = 0, p = pos;
  while (n < max_n && p < pos + span && p + GPD_PCAP_RECORD_BYTES <= len) {
    const uint32_t cap = rd(p + 8), wire = rd(p + 12);
    if (cap > I.snaplen || cap > wire || p + GPD_PCAP_RECORD_BYTES + cap > len) break;
    p += GPD_PCAP_RECORD_BYTES + cap;
    n++;
  }
  return n;
}

int gpd_decode_pcap_at(gpd_ctx *ctx, const uint8_t *buf, uint64_t len, const gpd_pcap_info *info,
                       uint64_t pos, uint64_t max_n, const gpd_result *out, uint64_t *n_out,
                       uint64_t *next_pos, int *stop, int nthreads) {
  if (!ctx || !buf || !info || !out || !out->status || !out->layers || !n_out)
    return set_error(GPD_ERR_INVALID, "gpd_decode_pcap: null argument");
  if (out->ext) return set_error(GPD_ERR_INVALID, "gpd_decode_pcap: ext records not supported");
  if (out->records) return set_error(GPD_ERR_INVALID, "gpd_decode_pcap: results as SoA arrays only");
  if (pos > len) return set_error(GPD_ERR_INVALID, "gpd_decode_pcap_at: pos beyond the buffer");
  nthreads = gpd::default_threads(nthreads);
  // this call's diagnostics (gpd_decode_pcap_last_*), reset before any early return
  const double t_call = now_ms();
  g_pt_walk = g_pt_walkwait = g_pt_stage = g_pt_sync = g_pt_drain = 0;
  for (auto &c : g_pw_counts) c = 0;
  g_pw_miss[0] = g_pw_miss[1] = ~0ull;
  struct Total {
    double t;
    ~Total() { g_pt_total = now_ms() - t; }
  } total{t_call};
  *n_out = 0;
  if (next_pos) *next_pos = pos;
  if (stop) *stop = GPD_PCAP_STOP_LIMIT;
  if (max_n == 0) return GPD_OK;
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  bool dw = ctx->tune.device_walk != 0;
  uint64_t done = 0, at = pos;
  for (;;) {
    if (dw) {
      uint64_t resume, handled = 0;
      bool ineligible = false;
      const gpd_result r = shifted(out, done);
      const int rc = decode_device_walk(ctx, buf, len, *info, at, max_n - done, &r, nthreads, &handled,
                                        &resume, next_pos, stop, &ineligible);
      done += handled;
      *n_out = done;
      if (rc) return rc;
      if (resume == UINT64_MAX) return GPD_OK;
      at = resume;
      if (ineligible) dw = false;  // one unbounded (pipelined) host walk does the rest
    }
    // The host walk from `at`: all of the call without the device walk; else only the chunk
    // the device walk could not vouch for (a record the reference rejects, a capture ending
    // inside a record, a speculation its stitch refuted), and then the device walk again
    // (one refuted speculation used to send the rest of the call to the host walk: r04, a
    // 2^24-record replay call 28 -> 200 ms)
    uint64_t lim = max_n - done;
    if (dw) {
      constexpr uint64_t kSpan = (uint64_t)gpd::kPwSeg * gpd::kPwMaxSeg;  // the device walk's chunk
      lim = std::min(lim, count_records(buf, len, *info, at, kSpan, lim) + 1u);
    }
    const gpd_result r = shifted(out, done);
    uint64_t k = 0, nxt = at;
    int st = GPD_PCAP_STOP_LIMIT;
    const int rc = decode_pcap_host_walk(ctx, buf, len, info, at, lim, &r, &k, &nxt, &st, nthreads);
    done += k;
    *n_out = done;
    if (next_pos) *next_pos = nxt;
    if (stop) *stop = st;
    if (rc || !dw || st != GPD_PCAP_STOP_LIMIT || done == max_n) return rc;
    at = nxt;
  }
}

void gpd_decode_pcap_last_walk_miss(uint64_t *pos2) {
  if (!pos2) return;
  pos2[0] = g_pw_miss[0];
  pos2[1] = g_pw_miss[1];
}

void gpd_decode_pcap_last_walk_counts(uint32_t *c7) {
  if (!c7) return;
  for (int k = 0; k < 7; k++) c7[k] = g_pw_counts[k];
}

void gpd_decode_pcap_last_times(double *ms6) {
  if (!ms6) return;
  ms6[0] = g_pt_total;     // the whole call
  ms6[1] = g_pt_walk;      // record walks (the first on the caller, the rest ahead on a helper)
  ms6[2] = g_pt_walkwait;  // waiting for a walk running ahead
  ms6[3] = g_pt_stage;     // descriptor rebase, staging copies, issuing transfers and launches
  ms6[4] = g_pt_sync;      // waiting for a slot's transfers and decode
  ms6[5] = g_pt_drain;     // copying a slot's results out (none with registered result arrays)
}

}  // extern "C"

// ---- pcapng capture in host memory (include/gpd_pcapng.h): raw-byte chunks H2D -> block walk
// on the device -> decode -> D2H, between the blocks that change the reader's state ----
namespace {

thread_local uint32_t g_ng_counts[8];

enum NgHow { kNgLimit, kNgEof, kNgState, kNgBlock, kNgHostChunk };

// The reader's next packets (at most lim) through the sequential host walk, decoded with
// gpd_decode_host in batches.  *k: packets decoded; *st: the GPD_PCAPNG_STOP_* of the walk.
int ng_decode_host_walk(gpd_ctx *ctx, gpd_pcapng_reader *r, uint64_t lim, const gpd_result *out, uint64_t *k,
                        int *st) {
  thread_local std::vector<uint32_t> off, cap;
  constexpr uint64_t kBatch = 1u << 20;
  *k = 0;
  *st = GPD_PCAPNG_STOP_LIMIT;
  while (*k < lim && *st == GPD_PCAPNG_STOP_LIMIT) {
    const uint64_t m = std::min(lim - *k, kBatch);
    if (off.size() < m) {
      off.resize(m);
      cap.resize(m);
    }
    uint64_t n = 0;
    const int rc = gpd_pcapng_index(r, m, off.data(), cap.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &n, st);
    if (rc != GPD_OK && rc != GPD_ERR_PCAPNG) return rc;
    if (n) {
      gpd_batch b{r->buf, r->len, off.data(), cap.data(), n};
      const gpd_result o = shifted(out, *k);
      const int rd = gpd_decode_host(ctx, &b, &o);
      if (rd) return rd;
      *k += n;
    }
  }
  return GPD_OK;
}

// The device walk from the reader's position while no block changes its state: at most max_n
// packets decoded into `out`.  *how tells why it returned and the reader stands accordingly:
//   kNgLimit      max_n packets done; the reader at the block after the last of them
//   kNgEof        the capture ended exactly after a block (the reader is stopped: EOF)
//   kNgState      at a section header, interface description or statistics block
//   kNgBlock      at a block the device does not vouch for
//   kNgHostChunk  at the entry of a chunk the device gave up (*chunk_end: where that chunk ends)
int ng_device_walk(gpd_ctx *ctx, gpd_pcapng_reader *r, uint64_t max_n, const gpd_result *out, int nthreads,
                   uint64_t *handled, NgHow *how, uint64_t *chunk_end) {
  const uint8_t *buf = r->buf;
  const uint64_t len = r->len;
  SegFormat<gpd::NgArgs> F{"gpd_decode_pcapng"};
  F.chunk = r->opts.chunk_bytes ? r->opts.chunk_bytes : (uint64_t)gpd::kPwSeg * gpd::kPwMaxSeg;
  F.margin = 128u << 10;                         // a block may run this far past its chunk
  F.cap_pkts = (F.chunk + F.margin) / 16 + 64;   // a packet block takes 16 bytes or more
  const bool be = r->big_endian;
  auto rd = [&](uint64_t p) {
    uint32_t v;
    std::memcpy(&v, buf + p, 4);
    return be ? __builtin_bswap32(v) : v;
  };
  // the mean block size: the first blocks, read here
  F.mean = 96;
  {
    uint64_t p = r->pos, nb = 0;
    while (nb < 64 && p + 12 <= len) {
      const uint32_t total = rd(p + 4);
      if (total < 12 || (total & 3) || p + total > len) break;
      p += total;
      nb++;
    }
    if (nb) F.mean = std::max<uint64_t>(16, (p - r->pos) / nb);
  }
  // the chunk state: what the walk needs of the reader's, constant until a state-changing block
  gpd::NgArgs &S = F.state;
  S.nif = (uint32_t)r->ifaces.size();
  for (uint32_t i = 0; i < S.nif; i++)
    if (r->ifaces[i].linktype == r->linktype) S.keep |= 1u << i;
  S.snaplen0 = S.nif ? r->ifaces[0].snaplen : 0;
  S.be = be;
  S.drop_is_error = r->opts.error_on_mismatching_linktype != 0;
  F.walk = gpd::launch_ng_walk;
  F.fill = gpd::launch_ng_fill;
  *how = kNgLimit;
  return seg_device_walk(ctx, buf, len, r->pos, max_n, out, nthreads, F, [&](const SegChunk &k, bool *more) -> int {
    const gpd::PwCtl &c = k.c;
    g_ng_counts[0]++;
    g_ng_counts[7] += c.pad[0];
    if (c.status & 1u) {  // the host walks this chunk from its entry
      g_ng_counts[1]++;
      g_ng_counts[3] += (c.status >> 1) & 1u;
      g_ng_counts[5] += (c.status >> 3) & 1u;
      g_ng_counts[6] += (c.status >> 4) & 1u;
      r->pos = k.B + k.entry;
      *chunk_end = k.B + k.own;
      *how = kNgHostChunk;
      return GPD_OK;
    }
    if (k.take < c.n) {  // the bound falls inside this chunk: the reader walks to it from the entry
      r->pos = k.B + k.entry;
      gpd::NgPacket p;
      for (uint64_t i = 0; i < k.take; i++)
        if (r->next_packet(&p)) return set_error(GPD_ERR_INVALID, "gpd_decode_pcapng: host and device walks disagree");
      *how = kNgLimit;
      return GPD_OK;
    }
    r->pos = k.B + c.next;
    if (k.done == max_n) {
      *how = kNgLimit;
    } else if (c.status & (gpd::kNgTailState | gpd::kNgTailBlock)) {
      g_ng_counts[2]++;
      g_ng_counts[4] += (c.status & gpd::kNgTailBlock) != 0;
      *how = (c.status & gpd::kNgTailState) ? kNgState : kNgBlock;
    } else if (k.last) {  // status 0 on the last chunk: the walk ended exactly at the capture's end
      *how = kNgEof;
    } else {
      *more = true;
    }
    return GPD_OK;
  }, handled);
}

}  // namespace

extern "C" {

int gpd_decode_pcapng(gpd_ctx *ctx, gpd_pcapng_reader *r, uint64_t max_n, const gpd_result *out, uint64_t *n_out,
                      int *stop, int nthreads) {
  if (!ctx || !r || !out || !out->status || !out->layers || !n_out)
    return set_error(GPD_ERR_INVALID, "gpd_decode_pcapng: null argument");
  if (out->ext) return set_error(GPD_ERR_INVALID, "gpd_decode_pcapng: ext records not supported");
  if (out->records) return set_error(GPD_ERR_INVALID, "gpd_decode_pcapng: results as SoA arrays only");
  if (r->opts.want_mixed_linktype)
    return set_error(GPD_ERR_INVALID, "gpd_decode_pcapng: a reader with want_mixed_linktype (a context has one first layer)");
  nthreads = gpd::default_threads(nthreads);
  for (auto &c : g_ng_counts) c = 0;
  *n_out = 0;
  if (stop) *stop = GPD_PCAPNG_STOP_LIMIT;
  if (max_n == 0) return GPD_OK;
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  uint64_t done = 0;
  auto finish = [&](int st) {
    *n_out = done;
    if (stop) *stop = st;
    return r->result(st);
  };
  const bool dw = r->opts.device_walk != 0;
  for (;;) {
    if (r->stop) return finish(r->stop);
    if (done == max_n) return finish(GPD_PCAPNG_STOP_LIMIT);
    uint64_t lim = max_n - done;  // packets the host walk takes next
    uint64_t until = UINT64_MAX;  // ... or until the reader stands here
    // (state-changing blocks right here are the reader's: no chunk travels only to stop at them)
    if (dw && r->absorb_state_blocks()) continue;
    if (dw && r->ifaces.size() <= gpd::kNgMaxIfaces && r->pos < r->len) {
      uint64_t handled = 0, chunk_end = 0;
      NgHow how = kNgLimit;
      const gpd_result o = shifted(out, done);
      const int rc = ng_device_walk(ctx, r, max_n - done, &o, nthreads, &handled, &how, &chunk_end);
      done += handled;
      *n_out = done;
      if (rc) return rc;
      if (how == kNgLimit) continue;
      if (how == kNgEof) {
        r->pos = r->blk_pos = r->len;
        r->stop = GPD_PCAPNG_STOP_EOF;
        r->err = "EOF";
        continue;
      }
      if (how == kNgState) {  // the reader takes the state-changing blocks; the device goes on behind them
        r->absorb_state_blocks();
        continue;
      }
      if (how == kNgBlock) lim = 1;
      if (how == kNgHostChunk) until = chunk_end;
    }
    // The host walk: all of the call without the device walk; else the one packet behind a
    // block the device does not vouch for, or the chunk it gave up, and then the device again.
    while (lim && !r->stop && r->pos < until) {
      const gpd_result o = shifted(out, done);
      uint64_t k = 0;
      int st = GPD_PCAPNG_STOP_LIMIT;
      const int rc = ng_decode_host_walk(ctx, r, std::min<uint64_t>(lim, until == UINT64_MAX ? lim : 256), &o, &k, &st);
      done += k;
      lim -= k;
      *n_out = done;
      if (rc) return rc;
    }
  }
}

void gpd_decode_pcapng_last_walk_counts(uint32_t *c8) {
  if (!c8) return;
  for (int k = 0; k < 8; k++) c8[k] = g_ng_counts[k];
}

}  // extern "C"
