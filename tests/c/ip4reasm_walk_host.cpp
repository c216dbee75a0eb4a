// ip4reasm_walk_host.cpp — ip4defrag's state machine for one key (gopacket_amd/csrc/gpd_ip4reasm_walk.h,
// the code lane 0 of a group's wave runs) on the host, for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -I include -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/c/ip4reasm_walk_host.cpp -o ip4reasm_walk_host
//   ip4reasm_walk_host groups.txt > outcomes.txt
//
// Input (text): "ngroups", then per group "nrec split" and nrec lines
// "src payload_len frag_offset length more t".  The first `split` records are one batch and the
// rest the next one, with the list carried between them as the device carries it: each batch
// gets node and piece arrays of exactly the carried nodes plus its records (the bound the device
// relies on), so an overrun is a sanitizer report.
// Output: per record "O what payload_len nfrags length flags npieces" and, for a datagram, its
// pieces "P src len pos"; per group "L nn highest current final last_seen".
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_ip4reasm_walk.h"

struct Rec {
  gpd::IprNode node;
  unsigned more;
  uint64_t t;
};

static void batch(gpd::IprList &L, std::vector<gpd::IprNode> &carried, const Rec *recs, unsigned n) {
  std::vector<gpd::IprNode> nodes(carried.size() + n);
  std::vector<gpd::IprPiece> pieces(carried.size() + n);
  for (size_t k = 0; k < carried.size(); ++k) nodes[k] = carried[k];
  uint32_t ppos = 0;
  for (unsigned i = 0; i < n; ++i) {
    gpd::IprBuilt B{};
    const uint32_t what = gpd::ipr_step(L, nodes.data(), recs[i].node, recs[i].more != 0, recs[i].t, pieces.data() + ppos, B);
    if (what == GPD_IP4_COMPLETE) {
      std::printf("O %u %u %u %u %u %u\n", what, B.payload_len, B.nfrags, B.length, B.flags, B.npieces);
      for (uint32_t p = 0; p < B.npieces; ++p)
        std::printf("P %u %u %u\n", pieces[ppos + p].src, pieces[ppos + p].len, pieces[ppos + p].pos);
      ppos += B.npieces;
    } else {
      std::printf("O %u 0 0 0 0 0\n", what);
    }
  }
  carried.assign(nodes.begin(), nodes.begin() + L.nn);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned ngroups;
  if (std::fscanf(f, "%u", &ngroups) != 1) return 2;
  for (unsigned g = 0; g < ngroups; ++g) {
    unsigned nrec, split;
    if (std::fscanf(f, "%u %u", &nrec, &split) != 2 || split > nrec) return 2;
    std::vector<Rec> recs(nrec);
    for (unsigned i = 0; i < nrec; ++i) {
      unsigned src, plen, fo, length, more;
      uint64_t t;
      if (std::fscanf(f, "%u %u %u %u %u %" SCNu64, &src, &plen, &fo, &length, &more, &t) != 6) return 2;
      recs[i] = Rec{gpd::IprNode{src, plen, (uint16_t)fo, (uint16_t)length, gpd::kIprBatch}, more, t};
    }
    gpd::IprList L;
    gpd::ipr_list_init(L);
    std::vector<gpd::IprNode> carried;
    batch(L, carried, recs.data(), split);
    batch(L, carried, recs.data() + split, nrec - split);
    std::printf("L %u %u %u %u %" PRIu64 "\n", L.nn, L.highest, L.current, L.final_received, L.last_seen);
  }
  std::fclose(f);
  return 0;
}
