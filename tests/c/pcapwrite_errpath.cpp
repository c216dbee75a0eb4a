// pcapwrite_errpath.cpp — include/gpd_pcapwrite.h on its no-device paths: gpd_pcap_file_header
// (which needs no device at all), and every argument check of gpd_pcap_write and
// gpd_batch_select, which return before the context or the device is touched.  The twin of
// pcapngwrite_errpath.cpp: a stand-alone program for a host sanitizer build, linked with
// gpd_pcapwrite.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/pcapwrite_errpath.cpp gopacket_amd/csrc/gpd_pcapwrite.hip -o pcapwrite_errpath
//
// The runtime functions the entry points call after their checks are stubbed here; reaching one
// is a failure.  The error texts are compared whole.  Prints "ok" and exits 0 when every path
// answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_pcapwrite.h"

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
#define EXPECT_ERR(call, text)                                      \
  do {                                                              \
    g_err[0] = 0;                                                   \
    EXPECT((call) == GPD_ERR_INVALID && std::strcmp(g_err, text) == 0); \
  } while (0)

int main() {
  // gpd_pcap_file_header: a heap block of exactly 24 bytes, so a 25th is the sanitizer's to report
  std::vector<uint8_t> fh(24, 0xA5);
  EXPECT(gpd_pcap_file_header(0, 65536, 1, fh.data()) == GPD_OK);
  const uint8_t want[24] = {0xD4, 0xC3, 0xB2, 0xA1, 2, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0};
  EXPECT(std::memcmp(fh.data(), want, 24) == 0);
  EXPECT(gpd_pcap_file_header(GPD_PCAPW_NANOS | GPD_PCAPW_FILE_HEADER, 7, 101, fh.data()) == GPD_OK);
  EXPECT(fh[0] == 0x4D && fh[1] == 0x3C && fh[2] == 0xB2 && fh[3] == 0xA1 && fh[16] == 7 && fh[20] == 101);
  EXPECT_ERR(gpd_pcap_file_header(0, 0, 1, nullptr), "gpd_pcap_file_header: null out");
  EXPECT_ERR(gpd_pcap_file_header(4, 0, 1, fh.data()), "gpd_pcap_file_header: unknown flags 0x4");

  alignas(16) static unsigned char ctx_bytes[64];  // never read: the checks come first
  gpd_ctx *ctx = reinterpret_cast<gpd_ctx *>(ctx_bytes);
  alignas(16) static uint8_t out[256];
  static uint8_t data[64];
  static uint32_t off[4], cap[4], o_off[4], o_len[4], o_idx[4];
  static uint64_t ts[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  gpd_batch big = in, nodata = in, nooff = in, nocap = in, wide = in, empty{nullptr, 0, nullptr, nullptr, 0};
  big.n = 0xFFFFFF01ull;
  nodata.data = nullptr;
  nooff.offset = nullptr;
  nocap.caplen = nullptr;
  wide.data_len = 0xFFFFFFF0ull;

  // gpd_pcap_write: what it refuses without a device
  uint64_t nw = 7, nb = 7, bad = 7;
#define WRITE(ctx_, in_, ts_, flags_, out_, cap_) \
  gpd_pcap_write(ctx_, in_, ts_, nullptr, nullptr, flags_, 65536, 1, out_, cap_, &nw, &nb, &bad, nullptr)
  EXPECT_ERR(WRITE(nullptr, &in, ts, 0, out, sizeof out), "gpd_pcap_write: null argument");
  EXPECT_ERR(WRITE(ctx, nullptr, ts, 0, out, sizeof out), "gpd_pcap_write: null argument");
  EXPECT_ERR(WRITE(ctx, &big, ts, 0, out, sizeof out), "gpd_pcap_write: batch of 4294967041 packets (max 2^32 - 256)");
  EXPECT_ERR(WRITE(ctx, &nodata, ts, 0, out, sizeof out), "gpd_pcap_write: batch data/offset/caplen must be non-NULL");
  EXPECT_ERR(WRITE(ctx, &nooff, ts, 0, out, sizeof out), "gpd_pcap_write: batch data/offset/caplen must be non-NULL");
  EXPECT_ERR(WRITE(ctx, &nocap, ts, 0, out, sizeof out), "gpd_pcap_write: batch data/offset/caplen must be non-NULL");
  EXPECT_ERR(WRITE(ctx, &wide, ts, 0, out, sizeof out), "gpd_pcap_write: data_len 4294967280 outside the 32-bit offset range");
  EXPECT(nw == 7 && nb == 7 && bad == 7);  // nothing written before the pointers are known good
  EXPECT_ERR(gpd_pcap_write(ctx, &in, ts, nullptr, nullptr, 0, 65536, 1, out, sizeof out, nullptr, &nb, &bad, nullptr),
             "gpd_pcap_write: null result pointer");
  EXPECT_ERR(gpd_pcap_write(ctx, &in, ts, nullptr, nullptr, 0, 65536, 1, out, sizeof out, &nw, nullptr, &bad, nullptr),
             "gpd_pcap_write: null result pointer");
  EXPECT_ERR(gpd_pcap_write(ctx, &in, ts, nullptr, nullptr, 0, 65536, 1, out, sizeof out, &nw, &nb, nullptr, nullptr),
             "gpd_pcap_write: null result pointer");
  EXPECT(nw == 7 && nb == 7 && bad == 7);
  EXPECT_ERR(WRITE(ctx, &in, ts, 4, out, sizeof out), "gpd_pcap_write: unknown flags 0x4");
  EXPECT(nw == 0 && nb == 0 && bad == ~0ull);  // the results are reset once they can be
  EXPECT_ERR(WRITE(ctx, &in, ts, 0x80000000u, out, sizeof out), "gpd_pcap_write: unknown flags 0x80000000");
  EXPECT_ERR(WRITE(ctx, &in, nullptr, 0, out, sizeof out),
             "gpd_pcap_write: ts_ns is required (a zero Timestamp's time.Now() is the caller's)");
  const char *aligned = "gpd_pcap_write: out must be a 16-byte aligned buffer of out_cap bytes";
  for (int k : {1, 4, 8, 15}) EXPECT_ERR(WRITE(ctx, &in, ts, 0, out + k, 128), aligned);  // misaligned out
  EXPECT_ERR(WRITE(ctx, &in, ts, GPD_PCAPW_FILE_HEADER, nullptr, 128), aligned);  // null out with a capacity
  EXPECT_ERR(WRITE(ctx, &big, nullptr, 4, out + 1, 128), "gpd_pcap_write: batch of 4294967041 packets (max 2^32 - 256)");

  // gpd_batch_select
  uint64_t k = 7;
  nb = 7;
#define SELECT(ctx_, in_, out_, cap_) \
  gpd_batch_select(ctx_, in_, nullptr, out_, cap_, o_off, o_len, o_idx, 4, &k, &nb, nullptr)
  EXPECT_ERR(SELECT(nullptr, &in, out, sizeof out), "gpd_batch_select: null argument");
  EXPECT_ERR(SELECT(ctx, nullptr, out, sizeof out), "gpd_batch_select: null argument");
  EXPECT_ERR(SELECT(ctx, &big, out, sizeof out), "gpd_batch_select: batch of 4294967041 packets (max 2^32 - 256)");
  EXPECT_ERR(SELECT(ctx, &nodata, out, sizeof out), "gpd_batch_select: batch data/offset/caplen must be non-NULL");
  EXPECT_ERR(SELECT(ctx, &wide, out, sizeof out), "gpd_batch_select: data_len 4294967280 outside the 32-bit offset range");
  EXPECT(k == 7 && nb == 7);
  EXPECT_ERR(gpd_batch_select(ctx, &in, nullptr, out, sizeof out, o_off, o_len, o_idx, 4, nullptr, &nb, nullptr),
             "gpd_batch_select: null result pointer");
  EXPECT_ERR(gpd_batch_select(ctx, &in, nullptr, out, sizeof out, o_off, o_len, o_idx, 4, &k, nullptr, nullptr),
             "gpd_batch_select: null result pointer");
  const char *aligned_sel = "gpd_batch_select: out_data must be a 16-byte aligned buffer of out_cap bytes";
  for (int j : {1, 4, 8, 15}) EXPECT_ERR(SELECT(ctx, &in, out + j, 128), aligned_sel);
  EXPECT(k == 0 && nb == 0);
  EXPECT_ERR(SELECT(ctx, &in, nullptr, 128), aligned_sel);  // null out_data with a capacity
  // n == 0: nothing to select, with a buffer, as a sizing call, and with no arrays at all
  k = nb = 7;
  EXPECT(SELECT(ctx, &empty, out, sizeof out) == GPD_OK && k == 0 && nb == 0);
  k = nb = 7;
  EXPECT(SELECT(ctx, &empty, nullptr, 0) == GPD_OK && k == 0 && nb == 0);
  k = nb = 7;
  EXPECT(gpd_batch_select(ctx, &empty, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &k, &nb, nullptr) == GPD_OK &&
         k == 0 && nb == 0);
  EXPECT_ERR(SELECT(ctx, &empty, out + 4, 64), aligned_sel);  // the buffer is checked before n
  for (size_t j = 0; j < sizeof out; ++j) EXPECT(out[j] == 0);  // no call wrote the output
  EXPECT(g_reached == 0);  // no path above went past the checks
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
