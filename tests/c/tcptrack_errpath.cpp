// tcptrack_errpath.cpp — the host part of the connection tracker (include/gpd_tcptrack.h) on its
// no-device paths: every argument check of gpd_tcp_tracker_create, _run, _states, _forget and
// _reset returns before the device is touched, and an empty batch is a no-op.  A stand-alone
// program for a host sanitizer build, linked with gpd_tcptrack.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/tcptrack_errpath.cpp gopacket_amd/csrc/gpd_tcptrack.hip -o tcptrack_errpath
//
// The runtime functions of the context and of the flow table are stubbed here.  Prints "ok" and
// exits 0 when every path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_tcptrack.h"

static char g_err[256];
static int g_table_device;
static int g_peer_launches;

namespace gpd {
int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
int ctx_device(const gpd_ctx *) { return 0; }
int ctx_num_cus(const gpd_ctx *) { return 1; }
uint64_t flow_capacity(const gpd_flowtable *) { return 64; }
int flow_device(const gpd_flowtable *) { return g_table_device; }
hipError_t launch_flow_peers(const gpd_flowtable *, const PeerArgs &, hipStream_t) { return ++g_peer_launches, hipSuccess; }
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
  alignas(16) static unsigned char ctx_bytes[64], table_bytes[64];  // never read
  gpd_ctx *ctx = reinterpret_cast<gpd_ctx *>(ctx_bytes);
  gpd_flowtable *ft = reinterpret_cast<gpd_flowtable *>(table_bytes);
  static uint8_t data[64], verdict[4];
  static uint32_t off[4], cap[4], status[4], hdr[4], fid[4], conn[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  gpd_result res{};
  res.status = status;
  res.hdr_off = hdr;

  gpd_tcp_tracker *t = nullptr;
  const gpd_tcp_track_opts opts{1, 0}, bad_opts{0, 7};
  EXPECT(gpd_tcp_tracker_create(nullptr, ft, &opts, &t) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_create(ctx, nullptr, &opts, &t) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_create(ctx, ft, &opts, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_create(ctx, ft, &bad_opts, &t) == GPD_ERR_INVALID && t == nullptr);
  EXPECT(std::strstr(g_err, "reserved") != nullptr);
  g_table_device = 3;
  EXPECT(gpd_tcp_tracker_create(ctx, ft, &opts, &t) == GPD_ERR_INVALID && t == nullptr);
  EXPECT(std::strstr(g_err, "device") != nullptr);
  g_table_device = 0;
  EXPECT(gpd_tcp_tracker_create(ctx, ft, nullptr, &t) == GPD_OK && t != nullptr);
  gpd_tcp_tracker_destroy(nullptr);

  uint64_t out[4];
  auto mark = [&] {
    for (auto &v : out) v = 7;
  };
  auto all = [&](uint64_t x) {
    for (auto v : out)
      if (v != x) return false;
    return true;
  };
  // null arguments: nothing written before the pointers are known good
  mark();
  EXPECT(gpd_tcp_tracker_run(nullptr, &in, &res, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID && all(7));
  EXPECT(gpd_tcp_tracker_run(t, nullptr, &res, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID && all(7));
  EXPECT(gpd_tcp_tracker_run(t, &in, nullptr, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID && all(7));
  EXPECT(gpd_tcp_tracker_run(t, &in, &res, fid, verdict, conn, nullptr, nullptr) == GPD_ERR_INVALID);
  // the limit
  gpd_batch big = in;
  big.n = 0xFFFFFF01ull;
  EXPECT(gpd_tcp_tracker_run(t, &big, &res, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID && all(0));
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  // an empty batch is a no-op, whatever its arrays
  gpd_batch empty{nullptr, 0, nullptr, nullptr, 0};
  mark();
  EXPECT(gpd_tcp_tracker_run(t, &empty, &res, nullptr, nullptr, nullptr, out, nullptr) == GPD_OK && all(0));
  // missing arrays
  EXPECT(gpd_tcp_tracker_run(t, &in, &res, nullptr, verdict, conn, out, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_run(t, &in, &res, fid, nullptr, conn, out, nullptr) == GPD_ERR_INVALID);
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(gpd_tcp_tracker_run(t, &nodata, &res, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID);
  gpd_batch nooff = in;
  nooff.offset = nullptr;
  EXPECT(gpd_tcp_tracker_run(t, &nooff, &res, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID);
  gpd_result nohdr = res;
  nohdr.hdr_off = nullptr;
  EXPECT(gpd_tcp_tracker_run(t, &in, &nohdr, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "hdr_off") != nullptr);
  gpd_result nostatus = res;
  nostatus.status = nullptr;
  EXPECT(gpd_tcp_tracker_run(t, &in, &nostatus, fid, verdict, conn, out, nullptr) == GPD_ERR_INVALID);
  // states / forget / reset
  EXPECT(gpd_tcp_tracker_states(nullptr, verdict, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_states(t, nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_forget(nullptr, fid, 4, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_forget(t, nullptr, 4, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_forget(t, nullptr, 0, nullptr) == GPD_OK);
  EXPECT(gpd_tcp_tracker_forget(t, fid, 4, nullptr) == GPD_OK);  // nothing carried yet: no device call
  EXPECT(gpd_tcp_tracker_reset(nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tcp_tracker_reset(t, nullptr) == GPD_OK);           // likewise
  EXPECT(g_peer_launches == 0);
  gpd_tcp_tracker_destroy(t);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
