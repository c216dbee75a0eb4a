// tcpstream_errpath.cpp — the host part of gpd_tcp_assemble (include/gpd_tcpstream.h) on its
// no-device paths: every argument check returns before the context or the device is touched.
// A stand-alone program for a host sanitizer build, linked with gpd_tcpstream.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/tcpstream_errpath.cpp gopacket_amd/csrc/gpd_tcpstream.hip -o tcpstream_errpath
//
// The runtime functions the entry point calls after its checks are stubbed here; reaching one is
// a failure.  Prints "ok" and exits 0 when every path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_tcpstream.h"

static char g_err[256];
static int g_reached;

namespace gpd {
int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
int ctx_device(const gpd_ctx *) { return ++g_reached, 0; }
int ctx_num_cus(const gpd_ctx *) { return ++g_reached, 1; }
void *ctx_scratch(gpd_ctx *, int, size_t) { return ++g_reached, nullptr; }
}  // namespace gpd

extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

static int fails;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("line %d: %s  (last error: %s)\n", __LINE__, #cond, g_err); \
      ++fails;                                                              \
    }                                                                       \
  } while (0)

int main() {
  alignas(16) static unsigned char ctx_bytes[64];  // never read: the checks come first
  gpd_ctx *ctx = reinterpret_cast<gpd_ctx *>(ctx_bytes);
  alignas(16) static unsigned char seg_bytes[8 * 32 + 16], group_bytes[8 * 16 + 16];
  alignas(16) static unsigned char rec_bytes[8 * 32 + 16], stream_bytes[8 * 48 + 16], out_bytes[256 + 16];
  auto *segs = reinterpret_cast<gpd_tcp_seg *>(seg_bytes);
  auto *groups = reinterpret_cast<gpd_tcp_group *>(group_bytes);
  auto *recs = reinterpret_cast<gpd_tcp_reasm *>(rec_bytes);
  auto *streams = reinterpret_cast<gpd_tcp_stream *>(stream_bytes);
  uint8_t *bytes = out_bytes;
  static uint8_t data[64];
  static uint32_t off[4], cap[4];
  static gpd_tcp_conn state[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  const gpd_tcp_asm_opts opts{4, 0};
  uint64_t out[4] = {7, 7, 7, 7};
  auto untouched = [&] { return out[0] == 7 && out[1] == 7 && out[2] == 7 && out[3] == 7; };
  auto zeroed = [&] { return out[0] == 0 && out[1] == 0 && out[2] == 0 && out[3] == 0; };
  auto mark = [&] { out[0] = out[1] = out[2] = out[3] = 7; };
#define CALL(ctx_, in_, segs_, count_, groups_, ng_, opts_, recs_, mr_, streams_, bytes_, mb_, out_) \
  gpd_tcp_assemble(ctx_, in_, segs_, count_, groups_, ng_, state, 4, opts_, recs_, mr_, streams_, bytes_, mb_, out_, nullptr)

  // null arguments: nothing written before the pointers are known good
  EXPECT(CALL(nullptr, &in, segs, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, nullptr, segs, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, nullptr, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(untouched());
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, nullptr) == GPD_ERR_INVALID);
  // the limits
  gpd_batch big = in;
  big.n = 0xFFFFFF01ull;
  EXPECT(CALL(ctx, &big, segs, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr && zeroed());
  EXPECT(CALL(ctx, &in, segs, 0x80000000ull, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^31") != nullptr);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 5, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "groups") != nullptr);
  // output arrays: null with a capacity, bytes without records, records without streams, misaligned
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, nullptr, 8, streams, nullptr, 0, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, recs, 8, streams, nullptr, 256, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, nullptr, 0, streams, bytes, 0, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, recs, 8, nullptr, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, reinterpret_cast<gpd_tcp_reasm *>(rec_bytes + 8), 8, streams, bytes,
              256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, recs, 8, reinterpret_cast<gpd_tcp_stream *>(stream_bytes + 4), bytes,
              256, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, groups, 2, &opts, recs, 8, streams, out_bytes + 1, 255, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, reinterpret_cast<gpd_tcp_seg *>(seg_bytes + 4), 4, groups, 2, &opts, recs, 8, streams, bytes,
              256, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, reinterpret_cast<gpd_tcp_group *>(group_bytes + 8), 2, &opts, recs, 8, streams, bytes,
              256, out) == GPD_ERR_INVALID);
  // nothing to assemble: a no-op with every count 0, sized or not, before the batch is looked at
  mark();
  EXPECT(CALL(ctx, &in, segs, 0, groups, 0, &opts, recs, 8, streams, bytes, 256, out) == GPD_OK && zeroed());
  mark();
  EXPECT(CALL(ctx, &in, nullptr, 0, nullptr, 0, &opts, nullptr, 0, nullptr, nullptr, 0, out) == GPD_OK && zeroed());
  mark();
  EXPECT(CALL(ctx, &in, segs, 4, groups, 0, &opts, recs, 8, streams, bytes, 256, out) == GPD_OK && zeroed());
  // segments without their arrays, and the batch they point into
  EXPECT(CALL(ctx, &in, nullptr, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(CALL(ctx, &in, segs, 4, nullptr, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(CALL(ctx, &nodata, segs, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch nooff = in;
  nooff.offset = nullptr;
  EXPECT(CALL(ctx, &nooff, segs, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(CALL(ctx, &wide, segs, 4, groups, 2, &opts, recs, 8, streams, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "32-bit") != nullptr && zeroed());
  EXPECT(g_reached == 0);  // no path above went past the checks
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
