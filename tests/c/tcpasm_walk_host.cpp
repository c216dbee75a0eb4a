// tcpasm_walk_host.cpp — the stateful assembler's state machine (gopacket_amd/csrc/gpd_tcpasm_walk.h,
// the code lane 0 of an item's wave runs) on the host, for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -I include -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/c/tcpasm_walk_host.cpp -o tcpasm_walk_host
//   tcpasm_walk_host conns.txt > records.txt
//
// Input (text): "max_pages nconn", then per connection "nruns" and per run
// "nseg T close_all flush_all" followed by nseg lines "packet seq flags payload_off payload_len ts".
// A connection's page list is carried from run to run as the device carries it: an array of
// exactly conn.pages TamCarried records in list order.  Every run gets a node region and record
// arrays of exactly carried pages + the run's pages (the bound the device relies on), so an
// overrun is a sanitizer report.
// Output: per run its records "R packet src_off len skip stream_off call flags seen" and one line
// "S nrec ncalls nbytes completed flags next_seq pages page_bytes last_seen".
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_tcpasm_walk.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned max_pages, nconn;
  if (std::fscanf(f, "%u %u", &max_pages, &nconn) != 2) return 2;
  for (unsigned k = 0; k < nconn; ++k) {
    unsigned nruns;
    if (std::fscanf(f, "%u", &nruns) != 1) return 2;
    gpd_tcp_conn_info info{};
    std::vector<gpd::TamCarried> carried;
    for (unsigned run = 0; run < nruns; ++run) {
      unsigned nseg, close_all, flush_all;
      uint64_t T;
      if (std::fscanf(f, "%u %" SCNu64 " %u %u", &nseg, &T, &close_all, &flush_all) != 4) return 2;
      std::vector<gpd_tcp_seg> segs(nseg);
      std::vector<uint64_t> ts(nseg);
      std::vector<uint32_t> pbase(nseg + 1, 0);
      uint32_t maxpkt = 0;
      for (unsigned i = 0; i < nseg; ++i) {
        unsigned packet, seq, flags, off, len;
        if (std::fscanf(f, "%u %u %u %u %u %" SCNu64, &packet, &seq, &flags, &off, &len, &ts[i]) != 6) return 2;
        gpd_tcp_seg s{};
        s.packet = packet;
        s.seq = seq;
        s.flags = (uint16_t)flags;
        s.payload_off = off;
        s.payload_len = len;
        s.lookup_only = (uint8_t)(!(flags & GPD_TCP_SYN) && len == 0);
        segs[i] = s;
        pbase[i + 1] = pbase[i] + gpd::tsm_pages(len);
        if (packet > maxpkt) maxpkt = packet;
      }
      std::vector<uint32_t> offset(nseg ? maxpkt + 1 : 0);
      for (size_t p = 0; p < offset.size(); ++p) offset[p] = (uint32_t)p * 4096u;
      const uint32_t cp = (uint32_t)carried.size();
      if (cp != info.pages) return 3;
      const uint32_t cap = cp + pbase[nseg];
      std::vector<gpd::TamNode> nodes(cap);
      std::vector<gpd_tcp_reasm> recs(cap);
      std::vector<uint64_t> seen(cap);
      std::vector<uint32_t> src(cap);
      for (uint32_t j = 0; j < cp; ++j) nodes[j] = gpd::tam_node_of(carried[j], j, cp);
      gpd::TamConn c;
      gpd::tam_conn_load(c, info);
      const gpd::TamIo io{nodes.data(), recs.data(), seen.data(), src.data(), cap, max_pages, offset.data(),
                          (uint32_t)offset.size()};
      for (unsigned i = 0; i < nseg; ++i) gpd::tam_step(c, io, segs[i], cp + pbase[i], ts[i]);
      const gpd_tcp_flush fl{T, close_all, flush_all};
      gpd::tam_flush(c, io, fl);
      if (c.nrec > cap) return 3;
      for (uint32_t r = 0; r < c.nrec; ++r)
        std::printf("R %u %u %u %d %" PRIu64 " %u %u %" PRIu64 "\n", recs[r].packet, recs[r].src_off, recs[r].len,
                    recs[r].skip, recs[r].stream_off, recs[r].call, (unsigned)recs[r].flags, seen[r]);
      info = gpd::tam_conn_info(c);
      std::printf("S %u %u %u %u %u %u %u %u %" PRIu64 "\n", c.nrec, c.ncalls, c.nbytes, c.completed, info.flags,
                  info.next_seq, info.pages, info.page_bytes, info.last_seen_ns);
      // the new carry: the remaining pages in list order, exactly info.pages of them
      std::vector<gpd::TamCarried> next(info.pages);
      uint32_t cur = c.exists ? c.first : gpd::kTsmNil, off = 0, bytes = 0;
      for (uint32_t j = 0; j < info.pages; ++j) {
        if (cur >= cap) return 4;
        const gpd::TamNode nd = nodes[cur];
        next[j] = gpd::TamCarried{nd.seq, nd.len, nd.end, off, nd.seen, 0};
        off += nd.len;
        bytes += nd.len;
        cur = nd.next;
      }
      if (cur != gpd::kTsmNil || bytes != info.page_bytes) return 4;
      carried.swap(next);
    }
  }
  std::fclose(f);
  return 0;
}
