// gpd_pcapngwrite.hip — the blocks of a pcapng stream (pcapgo.NgWriter, pcapgo/ngwrite.go):
// section, interface and statistics blocks built on the host, and the kept packets of a device
// batch as enhanced packet blocks built on the device: include/gpd_pcapngwrite.h.
//
// The device part is the stream compaction of gpd_write_scan.h, shared with the pcap writer, over
// the record form NgForm: packet i takes 32 + round_up(caplen, 4) bytes.  The prefix and every
// record are multiples of 4 bytes, so each of a chunk's four words belongs to one record and is a
// header word, a data word (its tail bytes zero where the padding starts) or the trailer; a
// record is at least 32 bytes, so a chunk overlaps at most two.  The chunk hanging over a run's
// end takes at most 12 bytes of the next kept record's 28-byte header.  The stream's ragged last
// chunk is written with word stores.  A packet is rejected for ifindex >= n_ifaces or caplen >
// Length; which of the two it failed is read off that packet afterwards, the interface check
// first as in ngwrite.go:357-365.
//
// The prefix (host bytes) is staged into the context's scratch ahead of the scan, whose
// synchronisation also ends the caller's obligation to keep it, and copied to `out` device to
// device ahead of the copy kernel.  The chunk in which the prefix ends and the records begin is
// the first run's: the (at most three) prefix words in it travel as kernel arguments.
#include <hip/hip_runtime.h>

#include <cstring>

#include "gpd_internal.h"
#include "gpd_write_scan.h"
#include "../../include/gpd_pcapngwrite.h"

namespace gpd {
namespace {

constexpr uint32_t kHead = 28;                      // bytes of a record in front of its data
constexpr uint32_t kEnhanced = GPD_PCAPNG_BLOCK_ENHANCED;

// words [s, s + 4) of the 8 words lo:hi, s in 0..3
__device__ inline v4u words_from(v4u lo, v4u hi, uint32_t s) {
  uint32_t x0 = lo.x, x1 = lo.y, x2 = lo.z, x3 = lo.w, x4 = hi.x, x5 = hi.y, x6 = hi.z;
  if (s & 2u) {
    x0 = x2, x1 = x3, x2 = x4, x3 = x5, x4 = x6;
  }
  if (s & 1u) {
    x0 = x1, x1 = x2, x2 = x3, x3 = x4;
  }
  return v4u{x0, x1, x2, x3};
}
__device__ inline uint32_t pad4(uint32_t len) { return (len + 3u) & ~3u; }
// the block's total length field, in 32 bits as ngwrite.go:367-369 computes it
__device__ inline uint32_t rec_total(uint32_t len) { return 32u + pad4(len); }

struct NgForm {
  static constexpr bool kIndexed = false, kRunEndsInChunk = true, kLeads = true;
  static constexpr uint32_t kMaxRecs = 2;  // records are >= 32 bytes
  static __device__ uint64_t size(uint32_t len) { return 32ull + (((uint64_t)len + 3ull) & ~3ull); }
  // ngwrite.go:357-359 and :363-365
  static __device__ bool rejects(const WriteArgs &A, uint32_t i, uint32_t len) {
    return (A.ifindex ? A.ifindex[i] : 0u) >= A.n_ifaces || (A.wirelen && len > A.wirelen[i]);
  }
  // header words 2, 3, 4 and 6 (0 and 1 follow from len, 5 is len)
  static __device__ void fields(const WriteArgs &A, uint32_t i, uint32_t len, uint32_t f[4]) {
    const uint64_t ts = A.ts[i];
    f[0] = A.ifindex ? A.ifindex[i] : 0u;
    f[1] = (uint32_t)(ts >> 32);
    f[2] = (uint32_t)ts;
    f[3] = A.wirelen ? A.wirelen[i] : len;
  }
  static __device__ v4u next_head(const WriteArgs &A, uint32_t nx, uint32_t nlen) {  // (12 bytes at most)
    return v4u{kEnhanced, rec_total(nlen), A.ifindex ? A.ifindex[nx] : 0u, 0u};
  }
  static __device__ v4u span(v4u lo, v4u hi, uint32_t s) { return words_from(lo, hi, s >> 2); }
  static __device__ uint64_t first_chunk(uint64_t P0) { return P0 >> 4; }  // the chunk the prefix ends in
  // the prefix's last words (the words from P0 on are zero in fh)
  static __device__ uint64_t lead(const WriteArgs &A, uint64_t, uint64_t, uint64_t P0, v4u &V) {
    V = v4u{A.fh[0], A.fh[1], A.fh[2], 0u};
    return P0;
  }
  static __device__ uint64_t place(const WriteArgs &A, const WriteRec &q, int64_t d, v4u &V) {  // d: a multiple of 4
    const v4u z{0u, 0u, 0u, 0u};
    const uint32_t tot = rec_total(q.len);
    if (d < (int64_t)kHead) {  // header words
      const v4u H0{kEnhanced, tot, q.f[0], q.f[1]}, H1{q.f[2], q.len, q.f[3], 0u};
      V |= d < 0 ? words_from(z, H0, (uint32_t)(16 + d) >> 2)
                 : d < 16 ? words_from(H0, H1, (uint32_t)d >> 2) : words_from(H1, z, (uint32_t)(d - 16) >> 2);
    }
    const int64_t e = (int64_t)kHead + (int64_t)q.len - d;  // the data's end, in the chunk's bytes
    const int64_t k0 = d < (int64_t)kHead ? (int64_t)kHead - d : 0, k1 = e < 16 ? e : 16;
    if (k1 > k0)
      V |= src16_of(A.data, A.lim, (int64_t)q.off + d - (int64_t)kHead) & byte_mask((int32_t)k0, (int32_t)k1);
    const int64_t tj = (int64_t)kHead + (int64_t)pad4(q.len) - d;  // the trailer, in the chunk's bytes
    V.x |= tj == 0 ? tot : 0u;
    V.y |= tj == 4 ? tot : 0u;
    V.z |= tj == 8 ? tot : 0u;
    V.w |= tj == 12 ? tot : 0u;
    return q.pos + size(q.len);
  }
  static __device__ void store_tail(uint8_t *p, v4u V, uint32_t vend) {  // one to three words
    uint32_t *o = reinterpret_cast<uint32_t *>(p);
    o[0] = V.x;
    if (vend > 4u) o[1] = V.y;
    if (vend > 8u) o[2] = V.z;
  }
};

// ---- the host-built blocks --------------------------------------------------------------------
// A block under construction: counts always, writes when there is a buffer.
struct Sink {
  uint8_t *p;
  uint64_t n = 0;
  explicit Sink(uint8_t *out) : p(out) {}
  void bytes(const uint8_t *src, size_t k) {  // src NULL: zeros
    if (p && k) {
      if (src) std::memcpy(p + n, src, k);
      else std::memset(p + n, 0, k);
    }
    n += k;
  }
  void u16(uint16_t v) {
    const uint8_t b[2] = {(uint8_t)v, (uint8_t)(v >> 8)};
    bytes(b, 2);
  }
  void u32(uint32_t v) {
    const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    bytes(b, 4);
  }
  // writeOptions :125-150 for a string or []byte value, with `lead` zero bytes in front
  void opt_str(uint16_t code, const uint8_t *s, uint32_t len, uint32_t lead = 0) {
    const uint32_t k = len + lead;
    u16(code);
    u16((uint16_t)k);
    bytes(nullptr, lead);
    bytes(s, len);
    bytes(nullptr, (4u - (k & 3u)) & 3u);
  }
  void opt_time(uint16_t code, uint64_t ts) {  // :151-157: high word first
    u16(code);
    u16(8);
    u32((uint32_t)(ts >> 32));
    u32((uint32_t)ts);
  }
  void opt_u64(uint16_t code, uint64_t v) {  // :158-162
    u16(code);
    u16(8);
    u32((uint32_t)v);
    u32((uint32_t)(v >> 32));
  }
  void opt_u8(uint16_t code, uint8_t v) {  // :168-173: one byte stored in four
    u16(code);
    u16(1);
    u32(v);
  }
};

// A string of the struct as (pointer or NULL for zeros, length); false when it lies outside strs
// or is too long for an option.
bool str_of(const gpd_pcapng_str &s, const uint8_t *strs, uint64_t strs_len, uint32_t max_len, const uint8_t **p) {
  *p = nullptr;
  if (s.len == 0) return true;
  if (s.len > max_len) return false;
  if (s.off == ~0ull) return true;
  if (!strs || s.off > strs_len || s.len > strs_len - s.off) return false;
  *p = strs + s.off;
  return true;
}

// Runs `emit` to size the block and, when there is a buffer that holds it, again to write it.
template <class F>
int build_block(const char *who, uint8_t *out, uint64_t out_cap, uint64_t *len, F emit) {
  Sink count(nullptr);
  emit(count);
  *len = count.n;
  if (!out) {
    if (out_cap) return set_error(GPD_ERR_INVALID, "%s: null out with out_cap %llu", who, (unsigned long long)out_cap);
    return GPD_OK;
  }
  if (count.n > out_cap)
    return set_error(GPD_ERR_INVALID, "%s: the block takes %llu bytes, out_cap is %llu", who,
                     (unsigned long long)count.n, (unsigned long long)out_cap);
  Sink w(out);
  emit(w);
  return GPD_OK;
}

}  // namespace
}  // namespace gpd

extern "C" {

int gpd_pcapng_section_block(const gpd_pcapng_section_info *info, const uint8_t *strs, uint64_t strs_len,
                             uint8_t *out, uint64_t out_cap, uint64_t *len) {
  using namespace gpd;
  const char *who = "gpd_pcapng_section_block";
  if (!info || !len) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *len = 0;
  if (info->big_endian)
    return set_error(GPD_ERR_INVALID, "%s: a big-endian section is not written (NgWriter is little-endian only)", who);
  // ngwrite.go:191-210: application, comment, hardware, OS
  const gpd_pcapng_str *s[4] = {&info->application, &info->comment, &info->hardware, &info->os};
  const uint16_t code[4] = {4, 1, 2, 3};
  const uint8_t *p[4];
  for (int k = 0; k < 4; k++)
    if (!str_of(*s[k], strs, strs_len, 65535u, &p[k]))
      return set_error(GPD_ERR_INVALID, "%s: a string lies outside strs or is longer than 65535 bytes", who);
  return build_block(who, out, out_cap, len, [&](Sink &b) {
    uint32_t opts = 0;
    for (int k = 0; k < 4; k++)
      if (s[k]->len) opts += 4u + ((s[k]->len + 3u) & ~3u);
    if (opts) opts += 4;
    const uint32_t total = opts + 24u + 4u;
    b.u32(GPD_PCAPNG_BLOCK_SECTION);
    b.u32(total);
    b.u32(GPD_PCAPNG_BYTE_ORDER);
    b.u16(1);  // ngVersionMajor, ngVersionMinor
    b.u16(0);
    b.u32(0xFFFFFFFFu);  // section length: unspecified
    b.u32(0xFFFFFFFFu);
    for (int k = 0; k < 4; k++)
      if (s[k]->len) b.opt_str(code[k], p[k], s[k]->len);
    if (opts) b.u32(0);  // end of options
    b.u32(total);
  });
}

int gpd_pcapng_interface_block(const gpd_pcapng_iface *intf, const uint8_t *strs, uint64_t strs_len,
                               uint8_t *out, uint64_t out_cap, uint64_t *len) {
  using namespace gpd;
  const char *who = "gpd_pcapng_interface_block";
  if (!intf || !len) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *len = 0;
  // ngwrite.go:243-267: name, comment, description, filter (a zero byte in front), OS
  const gpd_pcapng_str *s[5] = {&intf->name, &intf->comment, &intf->description, &intf->filter, &intf->os};
  const uint16_t code[5] = {2, 1, 3, 11, 12};
  const uint32_t lead[5] = {0, 0, 0, 1, 0};
  const uint8_t *p[5];
  for (int k = 0; k < 5; k++)
    if (!str_of(*s[k], strs, strs_len, 65535u - lead[k], &p[k]))
      return set_error(GPD_ERR_INVALID, "%s: a string lies outside strs or is too long for a 16-bit option length", who);
  return build_block(who, out, out_cap, len, [&](Sink &b) {
    uint32_t opts = 0;
    for (int k = 0; k < 5; k++)
      if (s[k]->len) opts += 4u + ((s[k]->len + lead[k] + 3u) & ~3u);
    if (intf->ts_offset) opts += 12;
    opts += 8 + 4;  // if_tsresol, end of options
    const uint32_t total = opts + 16u + 4u;
    b.u32(GPD_PCAPNG_BLOCK_INTERFACE);
    b.u32(total);
    b.u16((uint16_t)intf->linktype);
    b.u16(0);  // reserved
    b.u32(intf->snaplen);
    for (int k = 0; k < 5; k++)
      if (s[k]->len) b.opt_str(code[k], p[k], s[k]->len, lead[k]);
    if (intf->ts_offset) b.opt_u64(14, intf->ts_offset);
    b.opt_u8(9, 9);  // :273-274: nanoseconds, whatever the interface says
    b.u32(0);        // end of options
    b.u32(total);
  });
}

int gpd_pcapng_stats_block(int64_t intf, uint32_t n_ifaces, const gpd_pcapng_stats *stats,
                           uint8_t *out, uint64_t out_cap, uint64_t *len) {
  using namespace gpd;
  const char *who = "gpd_pcapng_stats_block";
  if (!stats || !len) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *len = 0;
  if (intf < 0 || intf >= (int64_t)n_ifaces)  // ngwrite.go:302-304
    return set_error(GPD_ERR_PCAP, "Can't send statistics for non existent interface %lld; have only %u interfaces",
                     (long long)intf, n_ifaces);
  return build_block(who, out, out_cap, len, [&](Sink &b) {
    const bool dropped = stats->packets_dropped != GPD_PCAPNG_NO_VALUE64;
    const bool received = stats->packets_received != GPD_PCAPNG_NO_VALUE64;
    uint32_t opts = 12u * ((stats->has_start_time != 0) + (stats->has_end_time != 0) + dropped + received);
    if (opts) opts += 4;
    const uint32_t total = opts + 24u;
    const uint64_t ts = stats->has_last_update ? stats->last_update : 0ull;  // :332-335
    b.u32(GPD_PCAPNG_BLOCK_STATS);
    b.u32(total);
    b.u32((uint32_t)intf);
    b.u32((uint32_t)(ts >> 32));
    b.u32((uint32_t)ts);
    if (stats->has_start_time) b.opt_time(2, stats->start_time);
    if (stats->has_end_time) b.opt_time(3, stats->end_time);
    if (dropped) b.opt_u64(5, stats->packets_dropped);
    if (received) b.opt_u64(4, stats->packets_received);
    if (opts) b.u32(0);  // end of options
    b.u32(total);
  });
}

int gpd_pcapng_write(gpd_ctx *ctx, const gpd_batch *in, const uint64_t *ts_ns, const uint32_t *wirelen,
                     const uint32_t *ifindex, uint32_t n_ifaces, const uint8_t *keep,
                     const uint8_t *prefix, uint32_t prefix_len, uint8_t *out, uint64_t out_cap,
                     uint64_t *n_written, uint64_t *bytes, uint64_t *bad_index, uint32_t *bad_reason,
                     void *stream) {
  using namespace gpd;
  const char *who = "gpd_pcapng_write";
  int rc = check_in(who, ctx, in);
  if (rc) return rc;
  if (!n_written || !bytes || !bad_index || !bad_reason)
    return set_error(GPD_ERR_INVALID, "%s: null result pointer", who);
  *n_written = 0;
  *bytes = 0;
  *bad_index = ~0ull;
  *bad_reason = GPD_PCAPNGW_BAD_NONE;
  if (in->n && !ts_ns) return set_error(GPD_ERR_INVALID, "%s: ts_ns is required", who);
  if ((prefix_len & 3u) || prefix_len > GPD_PCAPNGW_MAX_PREFIX || (!prefix && prefix_len))
    return set_error(GPD_ERR_INVALID, "%s: prefix must hold prefix_len bytes, a multiple of 4 and at most %u (got %u)",
                     who, GPD_PCAPNGW_MAX_PREFIX, prefix_len);
  if ((!out && out_cap) || ((uintptr_t)out & 15u))
    return set_error(GPD_ERR_INVALID, "%s: out must be a 16-byte aligned buffer of out_cap bytes", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  WriteArgs A{};
  fill_in(A, in, keep);
  A.ts = ts_ns;
  A.wirelen = wirelen;
  A.ifindex = ifindex;
  A.n_ifaces = n_ifaces;
  A.base0 = prefix_len;
  if (prefix_len & 15u) std::memcpy(A.fh, prefix + (prefix_len & ~15u), prefix_len & 15u);
  A.out = out;
  uint64_t res[5] = {A.base0, 0, ~0ull, 0, 0};
  uint8_t *staged = nullptr;
  if (A.n || (out && A.base0)) {  // (an empty batch with a prefix: stage, synchronise, copy; no kernels)
    const bool with_bad = wirelen || ifindex || n_ifaces == 0;
    rc = carve_and_scan(ctx, who, A, with_bad ? bad_kernel<NgForm> : nullptr, sum_kernel<NgForm>, prefix,
                        out ? A.base0 : 0u, &staged, s, res);
    if (rc) return rc;
  }
  *bytes = res[0];
  *n_written = res[1];
  *bad_index = res[2];
  if (out || out_cap) {
    rc = check_stream_cap(who, res, out_cap);
    if (rc) return rc;
    if (A.base0) GPD_TRY(hipMemcpyAsync(out, staged, A.base0, hipMemcpyDeviceToDevice, s));
    if (res[1]) {
      hipLaunchKernelGGL(copy_kernel<NgForm>, dim3((A.nwave + kCopyWaves - 1u) / kCopyWaves), dim3(64 * kCopyWaves),
                         0, s, A);
      GPD_TRY(hipGetLastError());
    }
  }
  if (res[2] != ~0ull) {
    if ((uint32_t)res[4] >= n_ifaces) {  // ngwrite.go:357-359 comes first
      *bad_reason = GPD_PCAPNGW_BAD_IFACE;
      return set_error(GPD_ERR_PCAP, "Can't send statistics for non existent interface %u; have only %u interfaces",
                       (uint32_t)res[4], n_ifaces);
    }
    *bad_reason = GPD_PCAPNGW_BAD_LENGTH;
    return set_error(GPD_ERR_PCAP, "invalid capture info (packet %llu: capture length %u, length %u):  capture length > length",
                     (unsigned long long)res[2], (uint32_t)res[3], (uint32_t)(res[3] >> 32));
  }
  return GPD_OK;
}

}  // extern "C"
