// dns_errpath.cpp — the host part of the DNS decode (include/gpd_dns.h) on its no-device paths:
// every argument check of gpd_dns_decode returns before the context or the device is touched,
// and gpd_dns_decode_host needs no device at all.  A stand-alone program for a host sanitizer
// build, linked with gpd_dns.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/dns_errpath.cpp gopacket_amd/csrc/gpd_dns.hip -o dns_errpath
//
// The four runtime functions the entry point calls after its checks are stubbed here; reaching
// one is a failure.  Prints "ok" and exits 0 when every path answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_dns.h"

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
  alignas(16) static unsigned char msg_bytes[4 * 48 + 16], ent_bytes[8 * 32];
  static uint8_t names[64];
  static uint8_t data[64];
  static uint32_t off[4], cap[4], st[4], ho[4];
  static uint64_t lw[4];
  gpd_batch in{data, sizeof data, off, cap, 4};
  gpd_result res{};
  res.status = st;
  res.layers = lw;
  res.hdr_off = ho;
  gpd_dns_out out{reinterpret_cast<gpd_dns_msg *>(msg_bytes), 4, reinterpret_cast<gpd_dns_entry *>(ent_bytes), 8, names, 64};
  gpd_dns_counts c;
  std::memset(&c, 7, sizeof c);

  // null arguments
  EXPECT(gpd_dns_decode(nullptr, &in, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode(ctx, nullptr, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode(ctx, &in, nullptr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode(ctx, &in, &res, nullptr, nullptr, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode(ctx, &in, &res, nullptr, &out, nullptr, nullptr) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 0x0707070707070707ull);  // nothing written before the pointers are known good
  // the budget's range
  for (uint32_t bad : {0u, 65536u, 0xFFFFFFFFu}) {
    gpd_dns_config cfg{bad, 0};
    EXPECT(gpd_dns_decode(ctx, &in, &res, &cfg, &out, &c, nullptr) == GPD_ERR_INVALID);
    EXPECT(std::strstr(g_err, "max_work") != nullptr);
  }
  gpd_dns_config rsv{4096, 1};
  EXPECT(gpd_dns_decode(ctx, &in, &res, &rsv, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 0 && c.entries == 0 && c.name_bytes == 0 && c.deferred == 0 && c.work == 0);
  // an empty batch: a no-op, with the smallest and the largest budget
  gpd_batch empty{nullptr, 0, nullptr, nullptr, 0};
  for (uint32_t ok : {1u, 65535u}) {
    gpd_dns_config cfg{ok, 0};
    std::memset(&c, 7, sizeof c);
    EXPECT(gpd_dns_decode(ctx, &empty, &res, &cfg, &out, &c, nullptr) == GPD_OK);
    EXPECT(c.msgs == 0 && c.entries == 0 && c.name_bytes == 0 && c.deferred == 0);
  }
  // a batch of 2^32 - 256 packets or more
  gpd_batch big = in;
  big.n = 0xFFFFFF00ull;
  EXPECT(gpd_dns_decode(ctx, &big, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "2^32") != nullptr);
  // output arrays: null with a capacity, misaligned
  gpd_dns_out o2 = out;
  o2.msgs = nullptr;
  EXPECT(gpd_dns_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  o2 = out;
  o2.entries = nullptr;
  EXPECT(gpd_dns_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  o2 = out;
  o2.names = nullptr;
  EXPECT(gpd_dns_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  o2 = out;
  o2.msgs = reinterpret_cast<gpd_dns_msg *>(msg_bytes + 4);
  EXPECT(gpd_dns_decode(ctx, &in, &res, nullptr, &o2, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "aligned") != nullptr);
  // the batch and the results it needs
  gpd_batch nodata = in;
  nodata.data = nullptr;
  EXPECT(gpd_dns_decode(ctx, &nodata, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_batch wide = in;
  wide.data_len = 0xFFFFFFF0ull;
  EXPECT(gpd_dns_decode(ctx, &wide, &res, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_result nohdr = res;
  nohdr.hdr_off = nullptr;
  EXPECT(gpd_dns_decode(ctx, &in, &nohdr, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  gpd_result nost = res;
  nost.status = nullptr;
  EXPECT(gpd_dns_decode(ctx, &in, &nost, nullptr, &out, &c, nullptr) == GPD_ERR_INVALID);
  EXPECT(std::strstr(g_err, "hdr_off") != nullptr);
  EXPECT(g_reached == 0);  // no path above went past the checks

  // gpd_dns_decode_host: a query of one question, from a heap block of exactly its length
  static const uint8_t query[] = {0x12, 0x34, 0x01, 0x00, 0, 1, 0, 0, 0, 0, 0, 0, 3, 'w', 'w', 'w', 2, 'g', 'o', 0, 0, 1, 0, 1};
  uint8_t *q = static_cast<uint8_t *>(std::malloc(sizeof query));
  std::memcpy(q, query, sizeof query);
  gpd_dns_msg m;
  auto *ents = static_cast<gpd_dns_entry *>(std::malloc(sizeof(gpd_dns_entry)));
  auto *nm = static_cast<uint8_t *>(std::malloc(6));
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, nullptr, ents, 1, nm, 6, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, &m, ents, 1, nm, 6, nullptr) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode_host(nullptr, 5, 0, &m, ents, 1, nm, 6, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, &m, nullptr, 1, nm, 6, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, &m, ents, 1, nullptr, 6, &c) == GPD_ERR_INVALID);
  // the sizing call, one short each, exact
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, &m, nullptr, 0, nullptr, 0, &c) == GPD_ERR_INVALID);
  EXPECT(c.msgs == 1 && c.entries == 1 && c.name_bytes == 6 && c.deferred == 0 && c.work == 11);
  EXPECT(m.verdict == GPD_DNS_OK && m.n_q == 1 && m.id == 0x1234);
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, &m, ents, 0, nm, 6, &c) == GPD_ERR_INVALID);
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, &m, ents, 1, nm, 5, &c) == GPD_ERR_INVALID);
  EXPECT(c.entries == 1 && c.name_bytes == 6);
  EXPECT(gpd_dns_decode_host(q, sizeof query, 0, &m, ents, 1, nm, 6, &c) == GPD_OK);
  EXPECT(std::memcmp(nm, "www.go", 6) == 0 && ents[0].name_len == 6 && ents[0].type == 1 && ents[0].klass == 1);
  // the budget: work 11 decodes, 10 defers (no entries, no names, nothing stored)
  EXPECT(gpd_dns_decode_host(q, sizeof query, 11, &m, ents, 1, nm, 6, &c) == GPD_OK && m.verdict == GPD_DNS_OK);
  EXPECT(gpd_dns_decode_host(q, sizeof query, 10, &m, nullptr, 0, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DNS_DEFERRED && c.deferred == 1 && c.entries == 0 && c.name_bytes == 0 && m.n_q == 0 &&
         m.qdcount == 1);
  // an empty and a short message
  EXPECT(gpd_dns_decode_host(nullptr, 0, 0, &m, nullptr, 0, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DNS_E_TOO_SHORT && m.truncated == 1 && m.data_len == 0);
  EXPECT(gpd_dns_decode_host(q, 11, 0, &m, nullptr, 0, nullptr, 0, &c) == GPD_OK);
  EXPECT(m.verdict == GPD_DNS_E_TOO_SHORT && m.id == 0 && m.data_len == 11);
  std::free(q);
  std::free(ents);
  std::free(nm);
  EXPECT(g_reached == 0);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
