// gpd_pcapwrite.hip — the kept packets of a device batch as a pcap stream (pcapgo.Writer,
// pcapgo/write.go:80-129) or as a new dense batch: include/gpd_pcapwrite.h.
//
// A stream compaction over variable-length records: the scan, the chunk loop and the host
// helpers are gpd_write_scan.h's, shared with the pcapng writer.  Here are the two record forms.
// Packet i takes a slot of 16 + caplen bytes (PcapForm) or round_up(caplen, 16) bytes
// (BatchForm).  A pcap chunk is put together from the header words and the source bytes of the
// (at most two) records it overlaps; the file header travels as kernel arguments and is written
// by the wave whose run starts the records; the stream's ragged last chunk is written with byte
// stores.  A batch slot is 16-aligned: one record per chunk, its bytes, then zeros, and no run
// ends inside a chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "gpd_internal.h"
#include "gpd_write_scan.h"
#include "../../include/gpd_pcapwrite.h"

namespace gpd {
namespace {

constexpr uint32_t kFileHeader = 24;

struct PcapForm {
  static constexpr bool kIndexed = false, kRunEndsInChunk = true, kLeads = true;
  static constexpr uint32_t kMaxRecs = 2;  // records are >= 16 bytes
  static __device__ uint64_t size(uint32_t len) { return 16ull + len; }
  // write.go:121-123 (launched only with a Length array)
  static __device__ bool rejects(const WriteArgs &A, uint32_t i, uint32_t len) { return len > A.wirelen[i]; }
  static __device__ v4u head(const WriteArgs &A, uint32_t i, uint32_t len) {  // the pcap record header
    const uint64_t ts = A.ts[i];
    return v4u{(uint32_t)(ts / 1000000000ull), (uint32_t)(ts % 1000000000ull) / A.scaler, len,
               A.wirelen ? A.wirelen[i] : len};
  }
  static __device__ void fields(const WriteArgs &A, uint32_t i, uint32_t len, uint32_t f[4]) {
    const v4u h = head(A, i, len);
    f[0] = h.x, f[1] = h.y, f[2] = h.z, f[3] = h.w;
  }
  static __device__ v4u next_head(const WriteArgs &A, uint32_t nx, uint32_t nlen) { return head(A, nx, nlen); }
  static __device__ v4u span(v4u lo, v4u hi, uint32_t s) { return bytes_from(lo, hi, s); }
  static __device__ uint64_t first_chunk(uint64_t) { return 0ull; }
  // the file header's 24 bytes: chunk 0, and bytes 0..7 of chunk 1
  static __device__ uint64_t lead(const WriteArgs &A, uint64_t cb, uint64_t ce, uint64_t P0, v4u &V) {
    V = cb == 0ull ? v4u{A.fh[0], A.fh[1], A.fh[2], A.fh[3]} : v4u{A.fh[4], A.fh[5], 0u, 0u};
    return ce < P0 ? ce : P0;
  }
  static __device__ uint64_t place(const WriteArgs &A, const WriteRec &q, int64_t d, v4u &V) {
    const v4u z{0u, 0u, 0u, 0u}, H{q.f[0], q.f[1], q.f[2], q.f[3]};
    if (d < 16) V |= d >= 0 ? bytes_from(H, z, (uint32_t)d) : bytes_from(z, H, (uint32_t)(16 + d));
    const int64_t e = 16 + (int64_t)q.len - d;  // the record's end, in the chunk's bytes
    const int64_t k0 = d < 16 ? 16 - d : 0, k1 = e < 16 ? e : 16;
    if (k1 > k0) V |= src16_of(A.data, A.lim, (int64_t)q.off + d - 16) & byte_mask((int32_t)k0, (int32_t)k1);
    return q.pos + 16ull + q.len;
  }
  static __device__ void store_tail(uint8_t *p, v4u V, uint32_t vend) {
    const uint32_t wds[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
    for (uint32_t b = 0; b < 16u; ++b)
      if (b < vend) p[b] = (uint8_t)(wds[b >> 2] >> ((b & 3u) * 8u));
  }
};

struct BatchForm {
  static constexpr bool kIndexed = true, kRunEndsInChunk = false, kLeads = false;
  static constexpr uint32_t kMaxRecs = 1;  // slots are chunks
  static __device__ uint64_t size(uint32_t len) { return ((uint64_t)len + 15ull) & ~15ull; }
  static __device__ void fields(const WriteArgs &, uint32_t, uint32_t, uint32_t[4]) {}
  static __device__ uint64_t first_chunk(uint64_t P0) { return (P0 + 15ull) >> 4; }
  static __device__ uint64_t place(const WriteArgs &A, const WriteRec &q, int64_t d, v4u &V) {
    const int64_t e = (int64_t)q.len - d, k1 = e < 16 ? e : 16;  // its bytes, then zeros
    if (k1 > 0) V |= src16_of(A.data, A.lim, (int64_t)q.off + d) & byte_mask(0, (int32_t)k1);
    return q.pos + size(q.len);
  }
};

// A stream of nothing but the file header.
__global__ __launch_bounds__(64) void pw_head_kernel(WriteArgs A) {
  const uint32_t t = threadIdx.x;
  if (t < kFileHeader) A.out[t] = (uint8_t)(A.fh[t >> 2] >> ((t & 3u) * 8u));
}

void file_header_words(uint32_t flags, uint32_t snaplen, uint32_t linktype, uint32_t w[6]) {
  w[0] = (flags & GPD_PCAPW_NANOS) ? 0xA1B23C4Du : 0xA1B2C3D4u;  // write.go:82-86
  w[1] = 2u | (4u << 16);                                        // versionMajor, versionMinor
  w[2] = w[3] = 0;                                               // timezone, sigfigs
  w[4] = snaplen;
  w[5] = linktype;
}

}  // namespace
}  // namespace gpd

extern "C" {

int gpd_pcap_file_header(uint32_t flags, uint32_t snaplen, uint32_t linktype, uint8_t out[24]) {
  if (!out) return gpd::set_error(GPD_ERR_INVALID, "gpd_pcap_file_header: null out");
  if (flags & ~(GPD_PCAPW_NANOS | GPD_PCAPW_FILE_HEADER))
    return gpd::set_error(GPD_ERR_INVALID, "gpd_pcap_file_header: unknown flags 0x%x", flags);
  uint32_t w[6];
  gpd::file_header_words(flags, snaplen, linktype, w);
  for (int k = 0; k < 24; k++) out[k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));  // little-endian
  return GPD_OK;
}

int gpd_pcap_write(gpd_ctx *ctx, const gpd_batch *in, const uint64_t *ts_ns, const uint32_t *wirelen,
                   const uint8_t *keep, uint32_t flags, uint32_t snaplen, uint32_t linktype,
                   uint8_t *out, uint64_t out_cap,
                   uint64_t *n_written, uint64_t *bytes, uint64_t *bad_index, void *stream) {
  using namespace gpd;
  const char *who = "gpd_pcap_write";
  int rc = check_in(who, ctx, in);
  if (rc) return rc;
  if (!n_written || !bytes || !bad_index) return set_error(GPD_ERR_INVALID, "%s: null result pointer", who);
  *n_written = 0;
  *bytes = 0;
  *bad_index = ~0ull;
  if (flags & ~(GPD_PCAPW_NANOS | GPD_PCAPW_FILE_HEADER))
    return set_error(GPD_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
  if (in->n && !ts_ns)
    return set_error(GPD_ERR_INVALID, "%s: ts_ns is required (a zero Timestamp's time.Now() is the caller's)", who);
  if ((!out && out_cap) || ((uintptr_t)out & 15u))
    return set_error(GPD_ERR_INVALID, "%s: out must be a 16-byte aligned buffer of out_cap bytes", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  WriteArgs A{};
  fill_in(A, in, keep);
  A.ts = ts_ns;
  A.wirelen = wirelen;
  A.scaler = (flags & GPD_PCAPW_NANOS) ? 1u : 1000u;
  A.base0 = (flags & GPD_PCAPW_FILE_HEADER) ? kFileHeader : 0u;
  file_header_words(flags, snaplen, linktype, A.fh);
  A.out = out;
  uint64_t res[5] = {A.base0, 0, ~0ull, 0, 0};
  if (A.n) {
    rc = carve_and_scan(ctx, who, A, wirelen ? bad_kernel<PcapForm> : nullptr, sum_kernel<PcapForm>, nullptr, 0,
                        nullptr, s, res);
    if (rc) return rc;
  }
  *bytes = res[0];
  *n_written = res[1];
  *bad_index = res[2];
  if (out || out_cap) {
    rc = check_stream_cap(who, res, out_cap);
    if (rc) return rc;
    if (res[1]) {
      hipLaunchKernelGGL(copy_kernel<PcapForm>, dim3((A.nwave + kCopyWaves - 1u) / kCopyWaves),
                         dim3(64 * kCopyWaves), 0, s, A);
      GPD_TRY(hipGetLastError());
    } else if (A.base0) {
      hipLaunchKernelGGL(pw_head_kernel, dim3(1), dim3(64), 0, s, A);
      GPD_TRY(hipGetLastError());
    }
  }
  if (res[2] != ~0ull)
    return set_error(GPD_ERR_PCAP, "invalid capture info (packet %llu: capture length %u, length %u):  capture length > length",
                     (unsigned long long)res[2], (uint32_t)res[3], (uint32_t)(res[3] >> 32));
  return GPD_OK;
}

int gpd_batch_select(gpd_ctx *ctx, const gpd_batch *in, const uint8_t *keep,
                     uint8_t *out_data, uint64_t out_cap, uint32_t *out_offset, uint32_t *out_caplen,
                     uint32_t *out_index, uint64_t max_out, uint64_t *n_out, uint64_t *bytes, void *stream) {
  using namespace gpd;
  const char *who = "gpd_batch_select";
  int rc = check_in(who, ctx, in);
  if (rc) return rc;
  if (!n_out || !bytes) return set_error(GPD_ERR_INVALID, "%s: null result pointer", who);
  *n_out = 0;
  *bytes = 0;
  const bool sizing = !out_data && !out_cap;
  if (!sizing && (!out_data || ((uintptr_t)out_data & 15u)))
    return set_error(GPD_ERR_INVALID, "%s: out_data must be a 16-byte aligned buffer of out_cap bytes", who);
  if (in->n == 0) return GPD_OK;
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  const hipStream_t s = (hipStream_t)stream;
  WriteArgs A{};
  fill_in(A, in, keep);
  A.out = out_data;
  A.o_off = out_offset;
  A.o_len = out_caplen;
  A.o_idx = out_index;
  uint64_t res[5];
  rc = carve_and_scan(ctx, who, A, nullptr, sum_kernel<BatchForm>, nullptr, 0, nullptr, s, res);
  if (rc) return rc;
  *bytes = res[0];
  *n_out = res[1];
  if (res[0] >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: the kept packets take %llu bytes, beyond the 32-bit offset range", who,
                     (unsigned long long)res[0]);
  if (sizing) return GPD_OK;
  if (res[0] > out_cap || res[1] > max_out)
    return set_error(GPD_ERR_INVALID, "%s: %llu packets in %llu bytes, out_cap is %llu and max_out %llu", who,
                     (unsigned long long)res[1], (unsigned long long)res[0], (unsigned long long)out_cap,
                     (unsigned long long)max_out);
  if (res[1] == 0) return GPD_OK;
  if (!out_offset || !out_caplen) return set_error(GPD_ERR_INVALID, "%s: null out_offset / out_caplen", who);
  hipLaunchKernelGGL(copy_kernel<BatchForm>, dim3((A.nwave + kCopyWaves - 1u) / kCopyWaves), dim3(64 * kCopyWaves),
                     0, s, A);
  GPD_TRY(hipGetLastError());
  return GPD_OK;
}

}  // extern "C"
