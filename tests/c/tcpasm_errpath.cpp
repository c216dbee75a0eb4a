// tcpasm_errpath.cpp — the host part of the stateful assembler (include/gpd_tcpasm.h) on its
// no-device paths: every argument check of gpd_tcp_assembler_run, _create, _stats, _reset and
// _conns returns before the device is touched, and an object that holds no connection answers a
// run without segments with zeros.  A stand-alone program for a host sanitizer build, linked with
// gpd_tcpasm.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/tcpasm_errpath.cpp gopacket_amd/csrc/gpd_tcpasm.hip -o tcpasm_errpath
//
// The runtime functions of the context are stubbed here.  Prints "ok" and exits 0 when every
// path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_tcpasm.h"

static char g_err[256];
static int g_device_asked;

namespace gpd {
int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
int ctx_device(const gpd_ctx *) { return ++g_device_asked, 0; }
int ctx_num_cus(const gpd_ctx *) { return 1; }
void *ctx_scratch(gpd_ctx *, int, size_t) { return nullptr; }
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
  alignas(16) static unsigned char seg_bytes[8 * 32 + 16], group_bytes[8 * 16 + 16];
  alignas(16) static unsigned char rec_bytes[8 * 32 + 16], stream_bytes[8 * 48 + 16], out_bytes[256 + 16];
  alignas(16) static unsigned char seen_bytes[8 * 8 + 16], ts_bytes[4 * 8 + 16];
  auto *segs = reinterpret_cast<gpd_tcp_seg *>(seg_bytes);
  auto *groups = reinterpret_cast<gpd_tcp_group *>(group_bytes);
  auto *recs = reinterpret_cast<gpd_tcp_reasm *>(rec_bytes);
  auto *streams = reinterpret_cast<gpd_tcp_stream *>(stream_bytes);
  auto *seen = reinterpret_cast<uint64_t *>(seen_bytes);
  auto *ts = reinterpret_cast<uint64_t *>(ts_bytes);
  uint8_t *bytes = out_bytes;
  static uint8_t data[64];
  static uint32_t off[4], cap[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  const gpd_tcp_asm_opts opts{4, 0};
  const gpd_tcp_flush fl{0, 0, 0};

  // create / destroy / stats / reset / conns
  gpd_tcp_assembler *a = nullptr;
  EXPECT(gpd_tcp_assembler_create(nullptr, 16, &opts, &a) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_assembler_create(ctx, 16, &opts, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_assembler_create(ctx, 16, nullptr, &a) == GPD_OK && a != nullptr);
  gpd_tcp_assembler_destroy(nullptr);
  uint64_t st[4] = {7, 7, 7, 7};
  EXPECT(gpd_tcp_assembler_stats(nullptr, st) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_assembler_stats(a, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_assembler_stats(a, st) == GPD_OK && st[0] == 0 && st[1] == 0 && st[2] == 0 && st[3] == 0);
  EXPECT(gpd_tcp_assembler_reset(nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_assembler_reset(a, nullptr) == GPD_OK);  // nothing held, nothing allocated: no device call
  EXPECT(gpd_tcp_assembler_conns(nullptr, reinterpret_cast<gpd_tcp_conn_info *>(out_bytes), nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_assembler_conns(a, nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_assembler_conns(a, reinterpret_cast<gpd_tcp_conn_info *>(out_bytes + 4), nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);

  uint64_t out[8];
  auto mark = [&] {
    for (auto &v : out) v = 7;
  };
  auto untouched = [&] {
    for (auto v : out)
      if (v != 7) return false;
    return true;
  };
  auto zeroed = [&] {
    for (auto v : out)
      if (v != 0) return false;
    return true;
  };
#define RUN(a_, in_, segs_, count_, groups_, ng_, ts_, fl_, recs_, mr_, seen_, streams_, ms_, bytes_, mb_, out_) \
  gpd_tcp_assembler_run(a_, in_, segs_, count_, groups_, ng_, ts_, 5, fl_, recs_, mr_, seen_, streams_, ms_, bytes_, mb_, out_, nullptr)

  // null arguments: nothing written before the pointers are known good
  mark();
  EXPECT(RUN(nullptr, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(untouched());
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, nullptr) == GPD_ERR_INVALID);
  EXPECT(RUN(a, nullptr, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(zeroed());
  // the limits
  gpd_batch big = in;
  big.n = 0xFFFFFF01ull;
  EXPECT(RUN(a, &big, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  EXPECT(RUN(a, &in, segs, 0x80000000ull, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^31") != nullptr);
  EXPECT(RUN(a, &in, segs, 4, groups, 5, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "groups") != nullptr);
  // output arrays: null with a capacity, no records-only mode, outputs without records, misaligned
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, nullptr, 8, nullptr, nullptr, 0, nullptr, 0, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, nullptr, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, nullptr, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, nullptr, 0, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "records-only") != nullptr);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, nullptr, 0, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, nullptr, 0, nullptr, streams, 0, nullptr, 0, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, nullptr, 0, nullptr, nullptr, 0, bytes, 0, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, nullptr, 0, seen, nullptr, 0, nullptr, 0, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, reinterpret_cast<gpd_tcp_reasm *>(rec_bytes + 8), 8, seen, streams, 8,
             bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, reinterpret_cast<gpd_tcp_stream *>(stream_bytes + 4), 8,
             bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, out_bytes + 1, 255, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, ts, &fl, recs, 8, reinterpret_cast<uint64_t *>(seen_bytes + 4), streams, 8, bytes,
             256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, reinterpret_cast<gpd_tcp_seg *>(seg_bytes + 4), 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes,
             256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, reinterpret_cast<gpd_tcp_group *>(group_bytes + 8), 2, ts, &fl, recs, 8, seen, streams, 8,
             bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, groups, 2, reinterpret_cast<uint64_t *>(ts_bytes + 4), &fl, recs, 8, seen, streams, 8, bytes,
             256, out) == GPD_ERR_INVALID);
  // segments without their arrays, and the batch they point into
  EXPECT(RUN(a, &in, nullptr, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(RUN(a, &in, segs, 4, nullptr, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(RUN(a, &nodata, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch nooff = in;
  nooff.offset = nullptr;
  EXPECT(RUN(a, &nooff, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(RUN(a, &wide, segs, 4, groups, 2, ts, &fl, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "32-bit") != nullptr && zeroed());
  // no segments and no connection held: a flush of nothing, with or without a batch, sized or not
  const gpd_tcp_flush all{~0ull, 1, 1};
  mark();
  EXPECT(RUN(a, nullptr, nullptr, 0, nullptr, 0, nullptr, &all, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, out) == GPD_OK &&
         zeroed());
  mark();
  EXPECT(RUN(a, &in, segs, 0, groups, 0, ts, nullptr, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_OK && zeroed());
  mark();
  EXPECT(RUN(a, &in, segs, 4, groups, 0, ts, &all, recs, 8, seen, streams, 8, bytes, 256, out) == GPD_OK && zeroed());
  EXPECT(g_device_asked == 1);  // create asked once for the context's device; nothing else did
  gpd_tcp_assembler_destroy(a);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
