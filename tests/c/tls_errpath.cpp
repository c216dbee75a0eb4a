// tls_errpath.cpp — the host part of the TLS decode (include/gpd_tls.h) on its no-device paths:
// every argument check of gpd_tls_decode and gpd_tls_decode_ranges returns before the context or
// the device is touched, and gpd_tls_decode_host needs no device at all.  A stand-alone program
// for a host sanitizer build, linked with gpd_tls.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/tls_errpath.cpp gopacket_amd/csrc/gpd_tls.hip -o tls_errpath
//
// The four runtime functions the entry points call after their checks are stubbed here; reaching
// one is a failure.  Prints "ok" and exits 0 when every path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_tls.h"

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
  alignas(16) static unsigned char msg_bytes[4 * 48 + 16], rec_bytes[8 * 16 + 16];
  static uint8_t data[64];
  static uint32_t off[4], cap[4], st[4], ho[4], rlen[4];
  static uint64_t lw[4], roff[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  gpd_result res{};
  res.status = st;
  res.layers = lw;
  res.hdr_off = ho;
  gpd_tls_out out{reinterpret_cast<gpd_tls_msg *>(msg_bytes), 4, reinterpret_cast<gpd_tls_rec *>(rec_bytes), 8};
  gpd_tls_ranges rg{data, sizeof data, roff, rlen, 4};
  gpd_tls_counts c;
  std::memset(&c, 7, sizeof c);

  // ---- gpd_tls_decode: null arguments
  EXPECT(gpd_tls_decode(nullptr, &in, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode(ctx, nullptr, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode(ctx, &in, nullptr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode(ctx, &in, &res, nullptr, nullptr, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode(ctx, &in, &res, nullptr, &out, nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 0x0707070707070707ull);  // nothing written before the pointers are known good
  // the budget's range
  for (uint32_t bad : {0u, 1048577u, 0xFFFFFFFFu}) {
    gpd_tls_config cfg{bad, 0};
    EXPECT(gpd_tls_decode(ctx, &in, &res, &cfg, &out, &c, nullptr) == GPD_ERR_INVALID);
    EXPECT(std::strstr(g_err, "max_records") != nullptr);
    EXPECT(gpd_tls_decode_ranges(ctx, &rg, &cfg, &out, &c, nullptr) == GPD_ERR_INVALID);
    EXPECT(std::strstr(g_err, "max_records") != nullptr);
  }
  gpd_tls_config rsv{1024, 1};
  EXPECT(gpd_tls_decode(ctx, &in, &res, &rsv, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_ranges(ctx, &rg, &rsv, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 0 && c.records == 0 && c.deferred == 0 && c.work == 0);
  // an empty batch and no ranges: a no-op, with the smallest and the largest budget
  gpd_batch empty{nullptr, 0, nullptr, nullptr, 0};
  gpd_tls_ranges none{nullptr, 0, nullptr, nullptr, 0};
  for (uint32_t ok : {1u, 1048576u}) {
    gpd_tls_config cfg{ok, 0};
    std::memset(&c, 7, sizeof c);
    EXPECT(gpd_tls_decode(ctx, &empty, &res, &cfg, &out, &c, nullptr) == GPD_OK);
    EXPECT(c.msgs == 0 && c.records == 0 && c.deferred == 0);
    std::memset(&c, 7, sizeof c);
    EXPECT(gpd_tls_decode_ranges(ctx, &none, &cfg, &out, &c, nullptr) == GPD_OK);
    EXPECT(c.msgs == 0 && c.records == 0 && c.deferred == 0);
  }
  // 2^32 - 256 packets or ranges, or more
  gpd_batch big = in;
  big.n = 0xFFFFFF00ull;
  EXPECT(gpd_tls_decode(ctx, &big, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  gpd_tls_ranges bigr = rg;
  bigr.n = 0x100000000ull;
  EXPECT(gpd_tls_decode_ranges(ctx, &bigr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  // output arrays: null with a capacity, misaligned
  gpd_tls_out o2 = out;
  o2.msgs = nullptr;
  EXPECT(gpd_tls_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_ranges(ctx, &rg, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  o2 = out;
  o2.recs = nullptr;
  EXPECT(gpd_tls_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_ranges(ctx, &rg, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  o2 = out;
  o2.msgs = reinterpret_cast<gpd_tls_msg *>(msg_bytes + 4);
  EXPECT(gpd_tls_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  o2 = out;
  o2.recs = reinterpret_cast<gpd_tls_rec *>(rec_bytes + 8);
  EXPECT(gpd_tls_decode_ranges(ctx, &rg, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  // the batch and the results it needs
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(gpd_tls_decode(ctx, &nodata, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(gpd_tls_decode(ctx, &wide, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_result nohdr = res;
  nohdr.hdr_off = nullptr;
  EXPECT(gpd_tls_decode(ctx, &in, &nohdr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_result nost = res;
  nost.status = nullptr;
  EXPECT(gpd_tls_decode(ctx, &in, &nost, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "hdr_off") != nullptr);
  // the ranges' own arrays
  EXPECT(gpd_tls_decode_ranges(nullptr, &rg, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_ranges(ctx, nullptr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_ranges(ctx, &rg, nullptr, nullptr, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_ranges(ctx, &rg, nullptr, &out, nullptr, nullptr) == GPD_ERR_INVALID);
  gpd_tls_ranges r2 = rg;
  r2.off = nullptr;
  EXPECT(gpd_tls_decode_ranges(ctx, &r2, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  r2 = rg;
  r2.len = nullptr;
  EXPECT(gpd_tls_decode_ranges(ctx, &r2, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  r2 = rg;
  r2.bytes = nullptr;
  EXPECT(gpd_tls_decode_ranges(ctx, &r2, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "off/len") != nullptr);
  EXPECT(g_reached == 0);  // no path above went past the checks

  // ---- gpd_tls_decode_host: a handshake record and a two-byte alert, from a heap block of
  // exactly their length
  static const uint8_t two[] = {22, 3, 3, 0, 3, 'a', 'b', 'c', 21, 3, 3, 0, 2, 2, 40};
  uint8_t *q = static_cast<uint8_t *>(std::malloc(sizeof two));
  std::memcpy(q, two, sizeof two);
  gpd_tls_msg m;
  auto *recs = static_cast<gpd_tls_rec *>(std::malloc(2 * sizeof(gpd_tls_rec)));
  EXPECT(gpd_tls_decode_host(q, sizeof two, 0, nullptr, recs, 2, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_host(q, sizeof two, 0, &m, recs, 2, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_host(nullptr, 5, 0, &m, recs, 2, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_tls_decode_host(q, sizeof two, 0, &m, nullptr, 2, &c) == GPD_ERR_INVALID);
  // the sizing call, one short, exact
  EXPECT(gpd_tls_decode_host(q, sizeof two, 0, &m, nullptr, 0, &c) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 1 && c.records == 2 && c.deferred == 0 && c.work == 2);
  EXPECT(m.verdict == GPD_TLS_OK && m.n_handshake == 1 && m.n_alert == 1 && m.contents_off == 8 && m.err_off == 15);
  EXPECT(gpd_tls_decode_host(q, sizeof two, 0, &m, recs, 1, &c) == GPD_ERR_INVALID);
  EXPECT(c.records == 2);
  EXPECT(gpd_tls_decode_host(q, sizeof two, 0, &m, recs, 2, &c) == GPD_OK);
  EXPECT(recs[0].off == 0 && recs[0].content_type == 22 && recs[0].version == 0x0303 && recs[0].length == 3);
  EXPECT(recs[1].off == 8 && recs[1].content_type == 21 && recs[1].a == 2 && recs[1].b == 40 && recs[1].flags == 0 &&
         recs[1].index_in_kind == 0);
  // the budget: work 2 decodes, a budget of 1 defers (no entries, nothing stored)
  EXPECT(gpd_tls_decode_host(q, sizeof two, 2, &m, recs, 2, &c) == GPD_OK && m.verdict == GPD_TLS_OK);
  EXPECT(gpd_tls_decode_host(q, sizeof two, 1, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_TLS_DEFERRED && c.deferred == 1 && c.records == 0 && m.n_handshake == 0 &&
         m.contents_off == 0 && m.err_off == 0 && m.data_len == sizeof two);
  // an empty and a short message; a record cut inside its body keeps the one before it
  EXPECT(gpd_tls_decode_host(nullptr, 0, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_TLS_E_TOO_SHORT && m.truncated == 1 && m.data_len == 0 && c.work == 1);
  EXPECT(gpd_tls_decode_host(q, 4, 0, &m, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_TLS_E_TOO_SHORT && m.data_len == 4 && m.err_off == 0);
  EXPECT(gpd_tls_decode_host(q, 14, 0, &m, recs, 2, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_TLS_E_LENGTH_MISMATCH && m.truncated == 1 && m.n_handshake == 1 && m.n_alert == 0 &&
         m.err_off == 8 && m.contents_off == 8 && c.records == 1);
  std::free(q);
  std::free(recs);
  EXPECT(g_reached == 0);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
