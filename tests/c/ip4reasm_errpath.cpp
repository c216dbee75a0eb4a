// ip4reasm_errpath.cpp — the host part of the IPv4 defragmentation's entry points
// (include/gpd_ip4reasm.h) on their no-device paths: every argument check returns before the
// device is touched, and an empty defragmenter answers stats and discard without one.
// A stand-alone program for a host sanitizer build, linked with gpd_ip4reasm.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/ip4reasm_errpath.cpp gopacket_amd/csrc/gpd_ip4reasm.hip -o ip4reasm_errpath
//
// The runtime functions the entry points call are stubbed here.  Prints "ok" and exits 0 when
// every path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_ip4reasm.h"

static char g_err[256];

namespace gpd {
int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
int ctx_device(const gpd_ctx *) { return 0; }
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
  alignas(16) static unsigned char ctx_bytes[64];  // never read
  gpd_ctx *ctx = reinterpret_cast<gpd_ctx *>(ctx_bytes);
  gpd_ip4_defrag *d = nullptr;
  EXPECT(gpd_ip4_defrag_create(nullptr, &d) == GPD_ERR_INVALID);
  EXPECT(gpd_ip4_defrag_create(ctx, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_ip4_defrag_create(ctx, &d) == GPD_OK && d != nullptr);
  if (!d) return 1;

  alignas(16) static unsigned char frag_bytes[4 * 32 + 16], oc_bytes[4 * 8 + 16], dg_bytes[4 * 32 + 16];
  alignas(16) static unsigned char out_bytes[256 + 16];
  alignas(16) static uint32_t off_out[8], cap_out[8];
  auto *frags = reinterpret_cast<gpd_ip4_frag *>(frag_bytes);
  auto *oc = reinterpret_cast<gpd_ip4_outcome *>(oc_bytes);
  auto *dg = reinterpret_cast<gpd_ip4_dgram *>(dg_bytes);
  uint8_t *bytes = out_bytes;
  static uint8_t data[64];
  static uint32_t off[4], cap[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  uint64_t out[4] = {7, 7, 7, 7};
  auto untouched = [&] { return out[0] == 7 && out[1] == 7 && out[2] == 7 && out[3] == 7; };
  auto zeroed = [&] { return out[0] == 0 && out[1] == 0 && out[2] == 0 && out[3] == 0; };
  auto mark = [&] { out[0] = out[1] = out[2] = out[3] = 7; };
#define RUN(d_, in_, frags_, count_, oc_, dg_, md_, off_, cap_, bytes_, mb_, out_) \
  gpd_ip4_defrag_run(d_, in_, frags_, count_, nullptr, 0, oc_, dg_, md_, off_, cap_, bytes_, mb_, out_, nullptr)

  // null arguments: nothing written before the pointers are known good
  EXPECT(RUN(nullptr, &in, frags, 4, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, nullptr, frags, 4, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(untouched());
  EXPECT(RUN(d, &in, frags, 4, oc, dg, 4, off_out, cap_out, bytes, 256, nullptr) == GPD_ERR_INVALID);
  // the limits
  gpd_batch big = in;
  big.n = 0xFFFFFF01ull;
  EXPECT(RUN(d, &big, frags, 4, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr && zeroed());
  EXPECT(RUN(d, &in, frags, 5, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);  // more records than packets
  big.n = 0xFFFFFF00ull;
  EXPECT(RUN(d, &big, frags, 0x80000000ull, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^31") != nullptr);
  // output arrays: null with a capacity, bytes without records, records without outcomes,
  // bytes without the batch's descriptors, misaligned
  EXPECT(RUN(d, &in, frags, 4, oc, nullptr, 4, off_out, cap_out, nullptr, 0, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, oc, dg, 4, off_out, cap_out, nullptr, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, oc, nullptr, 0, off_out, cap_out, bytes, 0, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, nullptr, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, oc, dg, 4, nullptr, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, oc, dg, 4, off_out, nullptr, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, reinterpret_cast<gpd_ip4_outcome *>(oc_bytes + 8), dg, 4, off_out, cap_out, bytes, 256,
             out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  EXPECT(RUN(d, &in, frags, 4, oc, reinterpret_cast<gpd_ip4_dgram *>(dg_bytes + 4), 4, off_out, cap_out, bytes, 256,
             out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, oc, dg, 4, off_out + 1, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, oc, dg, 4, off_out, cap_out + 2, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, frags, 4, oc, dg, 4, off_out, cap_out, out_bytes + 1, 255, out) == GPD_ERR_INVALID);
  EXPECT(RUN(d, &in, reinterpret_cast<gpd_ip4_frag *>(frag_bytes + 4), 4, oc, dg, 4, off_out, cap_out, bytes, 256,
             out) == GPD_ERR_INVALID);
  // nothing handed over: a no-op, sized or not, before the batch is looked at
  mark();
  EXPECT(RUN(d, &in, frags, 0, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_OK && zeroed());
  mark();
  EXPECT(RUN(d, &in, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, out) == GPD_OK && zeroed());
  // records without their array, and the batch they point into
  EXPECT(RUN(d, &in, nullptr, 4, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(RUN(d, &nodata, frags, 4, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch nooff = in;
  nooff.offset = nullptr;
  EXPECT(RUN(d, &nooff, frags, 4, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(RUN(d, &wide, frags, 4, oc, dg, 4, off_out, cap_out, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "32-bit") != nullptr && zeroed());
  // an empty defragmenter: stats and discard need no device
  uint64_t st[3] = {9, 9, 9}, n = 9;
  EXPECT(gpd_ip4_defrag_stats(d, st) == GPD_OK && st[0] == 0 && st[1] == 0 && st[2] == 0);
  EXPECT(gpd_ip4_defrag_stats(nullptr, st) == GPD_ERR_INVALID && gpd_ip4_defrag_stats(d, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_ip4_defrag_discard(d, 100, &n) == GPD_OK && n == 0);
  EXPECT(gpd_ip4_defrag_discard(nullptr, 100, &n) == GPD_ERR_INVALID && gpd_ip4_defrag_discard(d, 100, nullptr) == GPD_ERR_INVALID);
  gpd_ip4_defrag_destroy(d);
  gpd_ip4_defrag_destroy(nullptr);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
