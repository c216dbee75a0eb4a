// flow_expire_errpath.cpp — the host part of flow expiry (include/gpd_flow_expire.h) on its
// no-device paths: the null and range refusals of gpd_flow_remove, gpd_flow_expire and
// gpd_flow_load return before the table or the device is touched and set the error string, and
// the calls that have nothing to do (no ids; last_below == 0) are no-ops.  A stand-alone program
// for a host sanitizer build, linked with gpd_flow.hip alone:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         tests/c/flow_expire_errpath.cpp gopacket_amd/csrc/gpd_flow.hip -o flow_expire_errpath
//
// The runtime functions of the context are stubbed here, and the table is a block of poisoned
// bytes: a path that read it would be reported.  Prints "ok" and exits 0 when every path
// answers as the header says.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <sanitizer/asan_interface.h>

#include "../../gopacket_amd/csrc/gpd_internal.h"
#include "../../include/gpd_flow_expire.h"

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
int ctx_num_cus(const gpd_ctx *) { return 1; }
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

static bool said(const char *what) {
  const bool yes = std::strstr(g_err, what) != nullptr;
  g_err[0] = 0;
  return yes;
}

int main() {
  alignas(16) static unsigned char table_bytes[256];
  ASAN_POISON_MEMORY_REGION(table_bytes, sizeof table_bytes);  // never read
  gpd_flowtable *ft = reinterpret_cast<gpd_flowtable *>(table_bytes);
  static uint32_t ids[4];
  static uint8_t hold[4];
  uint64_t count = 7, out[2] = {7, 7};

  // gpd_flow_remove
  EXPECT(gpd_flow_remove(nullptr, ids, 4, nullptr) == GPD_ERR_INVALID && said("gpd_flow_remove: null"));
  EXPECT(gpd_flow_remove(ft, nullptr, 4, nullptr) == GPD_ERR_INVALID && said("gpd_flow_remove: null"));
  EXPECT(gpd_flow_remove(ft, nullptr, 0, nullptr) == GPD_OK);  // no ids: nothing to do
  EXPECT(gpd_flow_remove(ft, ids, 0, nullptr) == GPD_OK);

  // gpd_flow_expire
  EXPECT(gpd_flow_expire(nullptr, 5, hold, 0, ids, 4, &count, nullptr) == GPD_ERR_INVALID && count == 7);
  EXPECT(said("gpd_flow_expire: null"));
  EXPECT(gpd_flow_expire(ft, 5, hold, 0, ids, 4, nullptr, nullptr) == GPD_ERR_INVALID && said("gpd_flow_expire: null"));
  EXPECT(gpd_flow_expire(ft, 5, hold, 2u, ids, 4, &count, nullptr) == GPD_ERR_INVALID && count == 0);
  EXPECT(said("unknown flags 0x2"));
  count = 7;
  EXPECT(gpd_flow_expire(ft, 5, hold, GPD_FLOW_EXPIRE_PAIRS | 0x80000000u, ids, 4, &count, nullptr) == GPD_ERR_INVALID);
  EXPECT(said("unknown flags") && count == 0);
  count = 7;
  EXPECT(gpd_flow_expire(ft, 5, hold, 0, nullptr, 4, &count, nullptr) == GPD_ERR_INVALID && count == 0);
  EXPECT(said("null ids with max_ids 4"));
  // last_below == 0: nothing is before the first packet, with any other arguments
  count = 7;
  EXPECT(gpd_flow_expire(ft, 0, hold, GPD_FLOW_EXPIRE_PAIRS, ids, 4, &count, nullptr) == GPD_OK && count == 0);
  count = 7;
  EXPECT(gpd_flow_expire(ft, 0, nullptr, 0, nullptr, 0, &count, nullptr) == GPD_OK && count == 0);  // and as a sizing call
  EXPECT(g_err[0] == 0);

  // gpd_flow_load
  EXPECT(gpd_flow_load(nullptr, out, nullptr) == GPD_ERR_INVALID && said("gpd_flow_load: null"));
  EXPECT(gpd_flow_load(ft, nullptr, nullptr) == GPD_ERR_INVALID && said("gpd_flow_load: null"));
  EXPECT(out[0] == 7 && out[1] == 7);
  EXPECT(GPD_FLOW_EXPIRE_PAIRS == 1u);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
