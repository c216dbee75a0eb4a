// pcapngwrite_errpath.cpp — the host part of include/gpd_pcapngwrite.h: the three block builders
// (which need no device at all) with exact-size and one-short buffers and as sizing calls, and
// gpd_pcapng_write on its no-device paths: every argument check returns before the context or
// the device is touched.  A stand-alone program for a host sanitizer build, linked with
// gpd_pcapngwrite.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/pcapngwrite_errpath.cpp gopacket_amd/csrc/gpd_pcapngwrite.hip -o pcapngwrite_errpath
//
// The runtime functions the entry point calls after its checks are stubbed here; reaching one
// is a failure.  Every output buffer is a heap block of exactly the size under test, so that a
// byte written beyond it is the sanitizer's to report.  Prints "ok" and exits 0 when every path
// answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_pcapngwrite.h"

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

// One builder through its three calls: sizing, a buffer of exactly the size, a buffer one short
// (which must stay untouched).  Returns the block.
template <class F>
static std::vector<uint8_t> build(F call, uint64_t want_len) {
  uint64_t len = 7;
  EXPECT(call(nullptr, 0, &len) == GPD_OK);
  EXPECT(len == want_len && len % 4 == 0);
  std::vector<uint8_t> exact(len, 0xA5);
  uint64_t len2 = 7;
  EXPECT(call(exact.data(), len, &len2) == GPD_OK && len2 == len);
  if (len) {
    std::vector<uint8_t> shorter(len - 1, 0xA5);
    uint64_t len3 = 7;
    EXPECT(call(shorter.data(), len - 1, &len3) == GPD_ERR_INVALID && len3 == len);
    for (uint8_t b : shorter) EXPECT(b == 0xA5);
    EXPECT(std::strstr(g_err, "out_cap") != nullptr);
  }
  uint32_t head[2] = {0, 0}, tail = 0;
  if (len >= 12) {
    std::memcpy(head, exact.data(), 8);
    std::memcpy(&tail, exact.data() + len - 4, 4);
    EXPECT(head[1] == len && tail == len);
  }
  return exact;
}

int main() {
  static const uint8_t strs[] = "gopacketA testamd64linux";  // application, comment, hardware, OS
  gpd_pcapng_section_info si{};
  si.application = {0, 8, 0};
  si.comment = {8, 6, 0};
  si.hardware = {14, 5, 0};
  si.os = {19, 5, 0};
  auto sect = [&](uint8_t *o, uint64_t cap, uint64_t *len) {
    return gpd_pcapng_section_block(&si, strs, sizeof strs - 1, o, cap, len);
  };
  // 24 + (4 + 8) + (4 + 8) + (4 + 8) + (4 + 8) + 4 + 4
  std::vector<uint8_t> b = build(sect, 80);
  EXPECT(b[0] == 0x0A && b[1] == 0x0D && b[8] == 0x4D && b[24] == 4 && b[26] == 8 && std::memcmp(&b[28], "gopacket", 8) == 0);
  gpd_pcapng_section_info none{};
  auto sect0 = [&](uint8_t *o, uint64_t cap, uint64_t *len) {
    return gpd_pcapng_section_block(&none, nullptr, 0, o, cap, len);
  };
  build(sect0, 28);  // no option and no end-of-options entry
  uint64_t len = 7;
  gpd_pcapng_section_info be = si;
  be.big_endian = 1;
  EXPECT(gpd_pcapng_section_block(&be, strs, sizeof strs - 1, nullptr, 0, &len) == GPD_ERR_INVALID && len == 0);
  gpd_pcapng_section_info outside = si;
  outside.os = {20, 5, 0};  // one byte past strs
  EXPECT(gpd_pcapng_section_block(&outside, strs, sizeof strs - 1, nullptr, 0, &len) == GPD_ERR_INVALID);
  outside.os = {~0ull - 2, 5, 0};  // off + len wraps
  EXPECT(gpd_pcapng_section_block(&outside, strs, sizeof strs - 1, nullptr, 0, &len) == GPD_ERR_INVALID);
  outside.os = {0, 65536, 0};  // no 16-bit option length holds it
  EXPECT(gpd_pcapng_section_block(&outside, strs, sizeof strs - 1, nullptr, 0, &len) == GPD_ERR_INVALID);
  EXPECT(gpd_pcapng_section_block(nullptr, strs, 1, nullptr, 0, &len) == GPD_ERR_INVALID);
  EXPECT(gpd_pcapng_section_block(&si, strs, sizeof strs - 1, nullptr, 0, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_pcapng_section_block(&si, strs, sizeof strs - 1, nullptr, 5, &len) == GPD_ERR_INVALID);  // null out, a capacity
  si.os = {~0ull, 3, 0};  // three zero bytes
  b = build(sect, 80 - 4);
  EXPECT(b[60] == 3 && b[62] == 3 && b[64] == 0 && b[66] == 0 && b[67] == 0);
  si.os = {19, 5, 0};

  gpd_pcapng_iface ifc{};
  ifc.name = {0, 3, 0};     // "gop"
  ifc.filter = {8, 4, 0};   // "A te"
  ifc.ts_offset = 100;
  ifc.ts_resolution = 3;    // not looked at: if_tsresol is 9
  ifc.linktype = 1;
  ifc.snaplen = 96;
  auto intf = [&](uint8_t *o, uint64_t cap, uint64_t *len) {
    return gpd_pcapng_interface_block(&ifc, strs, sizeof strs - 1, o, cap, len);
  };
  // 16 + name (4 + 4) + filter (4 + 8: a zero byte and 4 bytes, padded) + tsoffset 12 + tsresol 8 + end 4 + 4
  b = build(intf, 64);
  EXPECT(b[24] == 11 && b[26] == 5 && b[28] == 0 && b[29] == 'A' && b[33] == 0);
  EXPECT(b[36] == 14 && b[38] == 8 && b[40] == 100 && b[48] == 9 && b[50] == 1 && b[52] == 9 && b[53] == 0);
  gpd_pcapng_iface bare{};
  auto intf0 = [&](uint8_t *o, uint64_t cap, uint64_t *len) {
    return gpd_pcapng_interface_block(&bare, nullptr, 0, o, cap, len);
  };
  build(intf0, 16 + 8 + 4 + 4);  // if_tsresol is always there
  gpd_pcapng_iface longf{};
  longf.filter = {~0ull, 65535, 0};  // one more than the option can say with its zero byte
  EXPECT(gpd_pcapng_interface_block(&longf, nullptr, 0, nullptr, 0, &len) == GPD_ERR_INVALID);
  longf.filter = {~0ull, 65534, 0};
  EXPECT(gpd_pcapng_interface_block(&longf, nullptr, 0, nullptr, 0, &len) == GPD_OK && len == 16 + 4 + 65536 + 8 + 4 + 4);

  gpd_pcapng_stats st{};
  st.last_update = 1519128000195312500ull;
  st.start_time = st.last_update - 100000000000ull;
  st.end_time = st.last_update;
  st.packets_received = 100;
  st.packets_dropped = 1;
  st.has_last_update = st.has_start_time = st.has_end_time = 1;
  auto stats = [&](uint8_t *o, uint64_t cap, uint64_t *len) { return gpd_pcapng_stats_block(1, 2, &st, o, cap, len); };
  b = build(stats, 24 + 4 * 12 + 4);
  uint32_t w[4];
  std::memcpy(w, &b[8], 16);
  EXPECT(w[0] == 1 && w[1] == (uint32_t)(st.last_update >> 32) && w[2] == (uint32_t)st.last_update && w[3] == (2u | 8u << 16));
  gpd_pcapng_stats st0{};
  st0.packets_received = st0.packets_dropped = GPD_PCAPNG_NO_VALUE64;
  st0.last_update = 5;  // without has_last_update: timestamp 0
  auto stats0 = [&](uint8_t *o, uint64_t cap, uint64_t *len) { return gpd_pcapng_stats_block(0, 1, &st0, o, cap, len); };
  b = build(stats0, 24);
  std::memcpy(w, &b[8], 12);
  EXPECT(w[0] == 0 && w[1] == 0 && w[2] == 0);
  EXPECT(gpd_pcapng_stats_block(2, 2, &st, nullptr, 0, &len) == GPD_ERR_PCAP && len == 0);
  EXPECT(std::strcmp(g_err, "Can't send statistics for non existent interface 2; have only 2 interfaces") == 0);
  EXPECT(gpd_pcapng_stats_block(-1, 2, &st, nullptr, 0, &len) == GPD_ERR_PCAP);
  EXPECT(std::strcmp(g_err, "Can't send statistics for non existent interface -1; have only 2 interfaces") == 0);
  EXPECT(gpd_pcapng_stats_block(0, 2, nullptr, nullptr, 0, &len) == GPD_ERR_INVALID);

  // gpd_pcapng_write: what it refuses without a device
  alignas(16) static unsigned char ctx_bytes[64];  // never read: the checks come first
  gpd_ctx *ctx = reinterpret_cast<gpd_ctx *>(ctx_bytes);
  alignas(16) static uint8_t out[256];
  static uint8_t data[64], prefix[32];
  static uint32_t off[4], cap[4];
  static uint64_t ts[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  uint64_t nw = 7, nb = 7, bad = 7;
  uint32_t why = 7;
#define WRITE(ctx_, in_, ts_, pre_, plen_, out_, cap_) \
  gpd_pcapng_write(ctx_, in_, ts_, nullptr, nullptr, 1, nullptr, pre_, plen_, out_, cap_, &nw, &nb, &bad, &why, nullptr)
  EXPECT(WRITE(nullptr, &in, ts, prefix, 8, out, sizeof out) == GPD_ERR_INVALID);
  EXPECT(WRITE(ctx, nullptr, ts, prefix, 8, out, sizeof out) == GPD_ERR_INVALID);
  EXPECT(nw == 7 && nb == 7 && bad == 7 && why == 7);  // nothing written before the pointers are known good
  EXPECT(gpd_pcapng_write(ctx, &in, ts, nullptr, nullptr, 1, nullptr, prefix, 8, out, sizeof out, &nw, &nb, &bad, nullptr,
                          nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_pcapng_write(ctx, &in, ts, nullptr, nullptr, 1, nullptr, prefix, 8, out, sizeof out, nullptr, &nb, &bad, &why,
                          nullptr) == GPD_ERR_INVALID);
  EXPECT(WRITE(ctx, &in, ts, prefix, 8, out + 4, 128) == GPD_ERR_INVALID);  // misaligned out
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  EXPECT(nw == 0 && nb == 0 && bad == ~0ull && why == GPD_PCAPNGW_BAD_NONE);
  EXPECT(WRITE(ctx, &in, ts, prefix, 8, nullptr, 128) == GPD_ERR_INVALID);  // null out with a capacity
  for (uint32_t plen : {1u, 2u, 3u, 6u, 30u}) EXPECT(WRITE(ctx, &in, ts, prefix, plen, out, sizeof out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "multiple of 4") != nullptr);
  EXPECT(WRITE(ctx, &in, ts, prefix, GPD_PCAPNGW_MAX_PREFIX + 4, out, sizeof out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "65536") != nullptr);
  EXPECT(WRITE(ctx, &in, ts, nullptr, 8, out, sizeof out) == GPD_ERR_INVALID);  // a length and no prefix
  EXPECT(WRITE(ctx, &in, nullptr, prefix, 8, out, sizeof out) == GPD_ERR_INVALID);  // ts_ns is required
  gpd_batch big = in;
  big.n = 0xFFFFFF01ull;
  EXPECT(WRITE(ctx, &big, ts, prefix, 8, out, sizeof out) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  gpd_batch nodata = in;
  nodata.data = nullptr;  // null `in` arrays with n > 0
  EXPECT(WRITE(ctx, &nodata, ts, prefix, 8, out, sizeof out) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(WRITE(ctx, &wide, ts, prefix, 8, out, sizeof out) == GPD_ERR_INVALID);
  EXPECT(g_reached == 0);  // no path above went past the checks
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
