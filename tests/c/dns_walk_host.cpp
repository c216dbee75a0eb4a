// dns_walk_host.cpp — the DNS walker (gopacket_amd/csrc/gpd_dns_walk.h) compiled for the host as a
// stand-alone program, built by tests/test_dns.py with AddressSanitizer and UBSan.
//
//   dns_walk_host FILE MAX_WORK
//
// FILE: u32 count, then per message u32 length and its bytes.  Every message is copied into a
// heap block of exactly its length (a read past it is the sanitizer's), walked with the counting
// sink, then with the storing sink into exactly-sized heap arrays, then again into arrays one
// element short each (the stores are bounded by the sink, and what was stored must be a prefix of
// the exact result).  One line per message: the message record, the entries and the names in hex,
// and the work.  tests/test_dns.py compares the lines with tests/dns_ref.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_dns_walk.h"

static void hex(const void *p, size_t n) {
  const uint8_t *b = static_cast<const uint8_t *>(p);
  for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
  if (n == 0) std::printf("-");
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const uint64_t max_work = std::strtoull(argv[2], nullptr, 10);
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t len = 0;
    if (std::fread(&len, 4, 1, f) != 1) return 2;
    uint8_t *data = static_cast<uint8_t *>(std::malloc(len ? len : 1));
    if (len && std::fread(data, 1, len, f) != len) return 2;
    if (len == 0) {  // an empty message: no byte of the block may be read
      std::free(data);
      data = nullptr;
    }
    gpd_dns_msg m0{}, m1{}, m2{};
    gpd::DnsWalk S;
    S.max_work = max_work;
    gpd::dns_walk(data, len, gpd::DnsCountSink{}, S, m0);
    const uint32_t ne = S.n_entries, nb = S.name_bytes;
    auto *ents = static_cast<gpd_dns_entry *>(std::malloc(ne ? ne * sizeof(gpd_dns_entry) : 1));
    auto *names = static_cast<uint8_t *>(std::malloc(nb ? nb : 1));
    std::memset(ents, 0xEE, ne * sizeof(gpd_dns_entry));
    std::memset(names, 0xEE, nb);
    gpd::DnsWalk W;
    W.max_work = max_work;
    gpd::dns_walk(data, len, gpd::DnsStoreSink{ents, ne, names, nb, 0u}, W, m1);
    if (std::memcmp(&m0, &m1, sizeof m0) != 0 || W.n_entries != ne || W.name_bytes != nb || W.work != S.work) {
      std::printf("message %u: the two sinks disagree\n", k);
      return 1;
    }
    // one element short each
    const uint32_t se = ne ? ne - 1 : 0, sb = nb ? nb - 1 : 0;
    auto *ents2 = static_cast<gpd_dns_entry *>(std::malloc(se ? se * sizeof(gpd_dns_entry) : 1));
    auto *names2 = static_cast<uint8_t *>(std::malloc(sb ? sb : 1));
    gpd::DnsWalk X;
    X.max_work = max_work;
    gpd::dns_walk(data, len, gpd::DnsStoreSink{ents2, se, names2, sb, 0u}, X, m2);
    if (std::memcmp(&m0, &m2, sizeof m0) != 0 || X.n_entries != ne || X.name_bytes != nb ||
        std::memcmp(ents, ents2, se * sizeof(gpd_dns_entry)) != 0 || std::memcmp(names, names2, sb) != 0) {
      std::printf("message %u: the short buffers differ from the exact ones\n", k);
      return 1;
    }
    hex(&m1, sizeof m1);
    std::printf(" ");
    hex(ents, ne * sizeof(gpd_dns_entry));
    std::printf(" ");
    hex(names, nb);
    std::printf(" %llu\n", (unsigned long long)W.work);
    std::free(ents);
    std::free(names);
    std::free(ents2);
    std::free(names2);
    std::free(data);
  }
  std::fclose(f);
  return 0;
}
