// dhcp_errpath.cpp — the host part of the DHCP decode (include/gpd_dhcp.h) on its no-device paths:
// every argument check of gpd_dhcp_decode returns before the context or the device is touched, and
// gpd_dhcp_decode_host needs no device at all.  A stand-alone program for a host sanitizer build,
// linked with gpd_dhcp.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/dhcp_errpath.cpp gopacket_amd/csrc/gpd_dhcp.hip -o dhcp_errpath
//
// The four runtime functions the entry point calls after its checks are stubbed here; reaching one
// is a failure.  Prints "ok" and exits 0 when every path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_dhcp.h"

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
  alignas(16) static unsigned char msg_bytes[4 * 48 + 16], opt_bytes[8 * 8 + 16];
  static uint8_t data[64];
  static uint32_t off[4], cap[4], st[4], ho[4];
  static uint64_t lw[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  gpd_result res{};
  res.status = st;
  res.layers = lw;
  res.hdr_off = ho;
  gpd_dhcp_out out{reinterpret_cast<gpd_dhcp_msg *>(msg_bytes), 4, reinterpret_cast<gpd_dhcp_opt *>(opt_bytes), 8};
  gpd_dhcp_counts c;
  std::memset(&c, 7, sizeof c);

  // ---- gpd_dhcp_decode: null arguments
  EXPECT(gpd_dhcp_decode(nullptr, &in, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dhcp_decode(ctx, nullptr, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dhcp_decode(ctx, &in, nullptr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dhcp_decode(ctx, &in, &res, nullptr, nullptr, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dhcp_decode(ctx, &in, &res, nullptr, &out, nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 0x0707070707070707ull);  // nothing written before the pointers are known good
  // the budget's range
  for (uint32_t bad : {0u, 65537u, 0xFFFFFFFFu}) {
    gpd_dhcp_config cfg{bad, 0};
    EXPECT(gpd_dhcp_decode(ctx, &in, &res, &cfg, &out, &c, nullptr) == GPD_ERR_INVALID);
    EXPECT(std::strstr(g_err, "max_options") != nullptr);
  }
  gpd_dhcp_config rsv{2048, 1};
  EXPECT(gpd_dhcp_decode(ctx, &in, &res, &rsv, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 0 && c.options == 0 && c.deferred == 0 && c.work == 0);
  // an empty batch: a no-op, with the smallest and the largest budget
  gpd_batch empty{nullptr, 0, nullptr, nullptr, 0};
  for (uint32_t ok : {1u, 65536u}) {
    gpd_dhcp_config cfg{ok, 0};
    std::memset(&c, 7, sizeof c);
    EXPECT(gpd_dhcp_decode(ctx, &empty, &res, &cfg, &out, &c, nullptr) == GPD_OK);
    EXPECT(c.msgs == 0 && c.options == 0 && c.deferred == 0);
  }
  // 2^32 - 256 packets, or more
  gpd_batch big = in;
  big.n = 0xFFFFFF00ull;
  EXPECT(gpd_dhcp_decode(ctx, &big, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  big.n = 0x100000000ull;
  EXPECT(gpd_dhcp_decode(ctx, &big, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  // output arrays: null with a capacity, misaligned
  gpd_dhcp_out o2 = out;
  o2.msgs = nullptr;
  EXPECT(gpd_dhcp_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  o2 = out;
  o2.opts = nullptr;
  EXPECT(gpd_dhcp_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  o2 = out;
  o2.msgs = reinterpret_cast<gpd_dhcp_msg *>(msg_bytes + 4);
  EXPECT(gpd_dhcp_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  o2 = out;
  o2.opts = reinterpret_cast<gpd_dhcp_opt *>(opt_bytes + 8);
  EXPECT(gpd_dhcp_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  // the batch and the results it needs
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(gpd_dhcp_decode(ctx, &nodata, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(gpd_dhcp_decode(ctx, &wide, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_result nohdr = res;
  nohdr.hdr_off = nullptr;
  EXPECT(gpd_dhcp_decode(ctx, &in, &nohdr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_result nost = res;
  nost.status = nullptr;
  EXPECT(gpd_dhcp_decode(ctx, &in, &nost, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "hdr_off") != nullptr);
  EXPECT(g_reached == 0);  // no path above went past the checks

  // ---- gpd_dhcp_decode_host: a DHCPv6 request with two options, from a heap block of exactly
  // its length
  static const uint8_t two[] = {3, 0x57, 0x19, 0x58, 0, 1, 0, 2, 'a', 'b', 0, 8, 0, 0};
  uint8_t *q = static_cast<uint8_t *>(std::malloc(sizeof two));
  std::memcpy(q, two, sizeof two);
  gpd_dhcp_msg m;
  auto *opts = static_cast<gpd_dhcp_opt *>(std::malloc(2 * sizeof(gpd_dhcp_opt)));
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 0, nullptr, opts, 2, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 0, &m, opts, 2, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dhcp_decode_host(6, nullptr, 5, 0, &m, opts, 2, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 0, &m, nullptr, 2, &c) == GPD_ERR_INVALID);
  for (uint32_t bad : {0u, 5u, 7u}) {
    EXPECT(gpd_dhcp_decode_host(bad, q, sizeof two, 0, &m, opts, 2, &c) == GPD_ERR_INVALID);
    EXPECT(std::strstr(g_err, "version") != nullptr);
  }
  // the sizing call, one short, exact
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 0, &m, nullptr, 0, &c) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 1 && c.options == 2 && c.deferred == 0 && c.work == 2);
  EXPECT(m.verdict == GPD_DHCP_OK && m.n_opts == 2 && m.version == 6 && m.op == 3 && m.xid == 0x571958 &&
         m.err_off == sizeof two && m.mflags == GPD_DHCP_CONTENTS);
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 0, &m, opts, 1, &c) == GPD_ERR_INVALID);
  EXPECT(c.options == 2);
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 0, &m, opts, 2, &c) == GPD_OK);
  EXPECT(opts[0].off == 4 && opts[0].code == 1 && opts[0].length == 2);
  EXPECT(opts[1].off == 10 && opts[1].code == 8 && opts[1].length == 0);
  // the budget: work 2 decodes, a budget of 1 defers (no entries, nothing stored)
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 2, &m, opts, 2, &c) == GPD_OK && m.verdict == GPD_DHCP_OK);
  EXPECT(gpd_dhcp_decode_host(6, q, sizeof two, 1, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_DEFERRED && c.deferred == 1 && c.options == 0 && m.n_opts == 0 && m.version == 6 &&
         m.op == 0 && m.xid == 0 && m.err_off == 0 && m.mflags == 0 && m.data_len == sizeof two);
  // an empty and a short message; an option cut inside its body keeps the one before it
  EXPECT(gpd_dhcp_decode_host(6, nullptr, 0, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_E_V6_TOO_SHORT && m.truncated == 1 && m.data_len == 0 && c.work == 0);
  EXPECT(gpd_dhcp_decode_host(4, nullptr, 0, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_E_V4_TOO_SHORT && m.truncated == 1 && m.version == 4 && m.err_arg == 0);
  EXPECT(gpd_dhcp_decode_host(4, q, sizeof two, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_E_V4_TOO_SHORT && m.err_arg == sizeof two && m.op == 0);
  EXPECT(gpd_dhcp_decode_host(6, q, 13, 0, &m, opts, 2, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_E_V6_OPT_NO_DATA && m.truncated == 0 && m.n_opts == 1 && m.err_off == 10 &&
         c.options == 1 && c.work == 2);
  std::free(q);
  // a DHCPv4 header whose hlen (below 228) passes its 240 bytes, and one option byte behind it
  uint8_t *b = static_cast<uint8_t *>(std::calloc(241, 1));
  b[0] = 2, b[2] = 227, b[236] = 0x63, b[237] = 0x82, b[238] = 0x53, b[239] = 0x63, b[240] = 0x35;
  EXPECT(gpd_dhcp_decode_host(4, b, 240, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_OK && m.mflags == GPD_DHCP_HW_PAST_DATA && m.hlen == 227 && m.op == 2 && c.work == 0);
  EXPECT(gpd_dhcp_decode_host(4, b, 241, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_E_V4_OPT_NO_DATA && m.err_off == 240 && m.mflags == GPD_DHCP_HW_PAST_DATA && c.work == 1);
  b[239] = 0x62;
  EXPECT(gpd_dhcp_decode_host(4, b, 241, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DHCP_E_V4_BAD_MAGIC && m.err_off == 236 && m.hlen == 227);
  // from 228 up 28 + HardwareLen wraps in uint8: the reference's panic, before the cookie is looked at
  for (uint32_t hl : {228u, 255u}) {
    b[2] = (uint8_t)hl;
    EXPECT(gpd_dhcp_decode_host(4, b, 241, 0, &m, nullptr, 0, &c) == GPD_OK);
    EXPECT(m.verdict == GPD_DHCP_E_V4_HW_PANIC && m.err_off == 28 && m.err_arg == hl - 228 && m.hlen == hl &&
           m.op == 2 && m.mflags == 0 && m.truncated == 0 && m.n_opts == 0 && c.work == 0);
  }
  std::free(b);
  std::free(opts);
  EXPECT(g_reached == 0);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
