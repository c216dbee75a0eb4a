// dhcp_walk_host.cpp — the DHCP walker (gopacket_amd/csrc/gpd_dhcp_walk.h) compiled for the host as
// a stand-alone program, built by tests/test_dhcp.py with AddressSanitizer and UBSan.
//
//   dhcp_walk_host FILE MAX_OPTIONS
//
// FILE: u32 count, then per message u32 version (4 or 6), u32 length and its bytes.  Every message
// is copied into a heap block of exactly its length (a read one byte past it is the sanitizer's),
// walked with the counting sink, then with the storing sink into an exactly-sized heap array, then
// again into an array one element short (the stores are bounded by the sink, and what was stored
// must be a prefix of the exact result).  One line per message: the message record and the option
// entries in hex, and the work.  tests/test_dhcp.py compares the lines with tests/dhcp_ref.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../gopacket_amd/csrc/gpd_dhcp_walk.h"

static void hex(const void *p, size_t n) {
  const uint8_t *b = static_cast<const uint8_t *>(p);
  for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
  if (n == 0) std::printf("-");
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const uint64_t max_options = std::strtoull(argv[2], nullptr, 10);
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t version = 0, len = 0;
    if (std::fread(&version, 4, 1, f) != 1 || std::fread(&len, 4, 1, f) != 1) return 2;
    uint8_t *data = static_cast<uint8_t *>(std::malloc(len ? len : 1));
    if (len && std::fread(data, 1, len, f) != len) return 2;
    if (len == 0) {  // an empty message: no byte of the block may be read
      std::free(data);
      data = nullptr;
    }
    gpd_dhcp_msg m0, m1, m2;
    std::memset(&m0, 0xEE, sizeof m0);  // the walk fills every byte, the reserved ones included
    std::memset(&m1, 0xEE, sizeof m1);
    std::memset(&m2, 0xEE, sizeof m2);
    gpd::DhcpWalk S;
    S.max_options = max_options;
    gpd::dhcp_walk(version, data, len, gpd::DhcpCountSink{}, S, m0);
    const uint32_t no = S.n_opts;
    auto *opts = static_cast<gpd_dhcp_opt *>(std::malloc(no ? no * sizeof(gpd_dhcp_opt) : 1));
    std::memset(opts, 0xEE, no * sizeof(gpd_dhcp_opt));
    gpd::DhcpWalk W;
    W.max_options = max_options;
    gpd::dhcp_walk(version, data, len, gpd::DhcpStoreSink{opts, no}, W, m1);
    if (std::memcmp(&m0, &m1, sizeof m0) != 0 || W.n_opts != no || W.work != S.work) {
      std::printf("message %u: the two sinks disagree\n", k);
      return 1;
    }
    const uint32_t so = no ? no - 1 : 0;  // one element short
    auto *opts2 = static_cast<gpd_dhcp_opt *>(std::malloc(so ? so * sizeof(gpd_dhcp_opt) : 1));
    gpd::DhcpWalk X;
    X.max_options = max_options;
    gpd::dhcp_walk(version, data, len, gpd::DhcpStoreSink{opts2, so}, X, m2);
    if (std::memcmp(&m0, &m2, sizeof m0) != 0 || X.n_opts != no ||
        std::memcmp(opts, opts2, so * sizeof(gpd_dhcp_opt)) != 0) {
      std::printf("message %u: the short buffer differs from the exact one\n", k);
      return 1;
    }
    hex(&m1, sizeof m1);
    std::printf(" ");
    hex(opts, no * sizeof(gpd_dhcp_opt));
    std::printf(" %llu\n", (unsigned long long)W.work);
    std::free(opts);
    std::free(opts2);
    std::free(data);
  }
  std::fclose(f);
  return 0;
}
