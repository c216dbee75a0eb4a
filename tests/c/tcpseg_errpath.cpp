// tcpseg_errpath.cpp — the host part of gpd_tcp_segments (include/gpd_tcpassembly.h) on its
// no-device paths: every argument check returns before the context or the device is touched.
// A stand-alone program for a host sanitizer build, linked with gpd_tcpseg.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/tcpseg_errpath.cpp gopacket_amd/csrc/gpd_tcpseg.hip -o tcpseg_errpath
//
// The four runtime functions the entry point calls after its checks are stubbed here; reaching
// one is a failure.  Prints "ok" and exits 0 when every path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_tcpassembly.h"

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
void ctx_fill_kparams(const gpd_ctx *, KParams &) { ++g_reached; }
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
  alignas(16) static unsigned char seg_bytes[64 * 32 + 16], group_bytes[64 * 16];
  auto *segs = reinterpret_cast<gpd_tcp_seg *>(seg_bytes);
  auto *groups = reinterpret_cast<gpd_tcp_group *>(group_bytes);
  static uint8_t data[64];
  static uint32_t off[4], cap[4], st[4], ho[4], fid[4];
  static uint64_t lw[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  gpd_result res{};
  res.status = st;
  res.layers = lw;
  res.hdr_off = ho;
  uint64_t cnt = 7, ng = 7, un = 7;

  // null arguments
  EXPECT(gpd_tcp_segments(nullptr, &in, &res, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_segments(ctx, nullptr, &res, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_segments(ctx, &in, nullptr, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_segments(ctx, &in, &res, nullptr, 0, segs, groups, 64, nullptr, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_segments(ctx, &in, &res, nullptr, 0, segs, groups, 64, &cnt, nullptr, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_segments(ctx, &in, &res, nullptr, 0, segs, groups, 64, &cnt, &ng, nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(cnt == 7 && ng == 7 && un == 7);  // nothing written before the pointers are known good
  // an empty batch: a no-op with every count 0, grouped or not, sized or not
  gpd_batch empty{nullptr, 0, nullptr, nullptr, 0};
  EXPECT(gpd_tcp_segments(ctx, &empty, &res, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_OK);
  EXPECT(cnt == 0 && ng == 0 && un == 0);
  cnt = ng = un = 7;
  EXPECT(gpd_tcp_segments(ctx, &empty, &res, fid, 128, nullptr, nullptr, 0, &cnt, &ng, &un, nullptr) == GPD_OK);
  EXPECT(cnt == 0 && ng == 0 && un == 0);
  // a batch past 2^32 - 256 packets
  gpd_batch big = in;
  big.n = 0xFFFFFF01ull;
  EXPECT(gpd_tcp_segments(ctx, &big, &res, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  // output arrays: null with a capacity, grouping without groups[], misaligned
  EXPECT(gpd_tcp_segments(ctx, &in, &res, nullptr, 0, nullptr, nullptr, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_segments(ctx, &in, &res, fid, 128, segs, nullptr, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_segments(ctx, &in, &res, nullptr, 0, reinterpret_cast<gpd_tcp_seg *>(seg_bytes + 4), groups, 64, &cnt,
                          &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  // the batch and the results it needs
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(gpd_tcp_segments(ctx, &nodata, &res, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(gpd_tcp_segments(ctx, &wide, &res, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  gpd_result nohdr = res;
  nohdr.hdr_off = nullptr;
  EXPECT(gpd_tcp_segments(ctx, &in, &nohdr, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  gpd_result nost = res;
  nost.status = nullptr;
  EXPECT(gpd_tcp_segments(ctx, &in, &nost, nullptr, 0, segs, groups, 64, &cnt, &ng, &un, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "hdr_off") != nullptr);
  EXPECT(cnt == 0 && ng == 0 && un == 0);
  EXPECT(g_reached == 0);  // no path above went past the checks
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
