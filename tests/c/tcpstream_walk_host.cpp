// tcpstream_walk_host.cpp — the assembler's sequential step (gopacket_amd/csrc/gpd_tcpstream_walk.h,
// the code lane 0 of a group's wave runs) on the host, for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -I include -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/c/tcpstream_walk_host.cpp -o tcpstream_walk_host
//   tcpstream_walk_host groups.txt > records.txt
//
// Input (text): "max_pages close_all ngroups", then per group "nseg open next_seq" and nseg lines
// "packet seq flags payload_off payload_len".  Every group gets page nodes and a record region of
// exactly its pages (the bound the device relies on), so an overrun is a sanitizer report.
// Output: per group its records "R packet src_off len skip stream_off call flags" and one line
// "S nrec ncalls nbytes completed open next_seq".
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_tcpstream_walk.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned max_pages, close_all, ngroups;
  if (std::fscanf(f, "%u %u %u", &max_pages, &close_all, &ngroups) != 3) return 2;
  for (unsigned g = 0; g < ngroups; ++g) {
    unsigned nseg, open, next_seq;
    if (std::fscanf(f, "%u %u %u", &nseg, &open, &next_seq) != 3) return 2;
    std::vector<gpd_tcp_seg> segs(nseg);
    std::vector<uint32_t> pbase(nseg + 1, 0);
    for (unsigned i = 0; i < nseg; ++i) {
      unsigned packet, seq, flags, off, len;
      if (std::fscanf(f, "%u %u %u %u %u", &packet, &seq, &flags, &off, &len) != 5) return 2;
      gpd_tcp_seg s{};
      s.packet = packet;
      s.seq = seq;
      s.flags = (uint16_t)flags;
      s.payload_off = off;
      s.payload_len = len;
      s.lookup_only = (uint8_t)(!(flags & GPD_TCP_SYN) && len == 0);
      segs[i] = s;
      pbase[i + 1] = pbase[i] + gpd::tsm_pages(len);
    }
    std::vector<gpd::TsmNode> nodes(pbase[nseg]);
    std::vector<gpd_tcp_reasm> recs(pbase[nseg]);
    gpd::TsmConn c;
    gpd::tsm_conn_init(c, open ? 1u : 0u, open ? next_seq : 0u);
    const gpd::TsmIo io{nodes.data(), recs.data(), pbase[nseg], max_pages};
    for (unsigned i = 0; i < nseg; ++i) gpd::tsm_step(c, io, segs[i], pbase[i]);
    gpd::tsm_finish(c, io, close_all != 0);
    if (c.nrec > pbase[nseg]) return 3;
    for (uint32_t r = 0; r < c.nrec; ++r)
      std::printf("R %u %u %u %d %" PRIu64 " %u %u\n", recs[r].packet, recs[r].src_off, recs[r].len, recs[r].skip,
                  recs[r].stream_off, recs[r].call, (unsigned)recs[r].flags);
    std::printf("S %u %u %u %u %u %u\n", c.nrec, c.ncalls, c.nbytes, c.completed, c.exists, c.exists ? c.next_seq : 0u);
  }
  std::fclose(f);
  return 0;
}
