// gpd_pcapng_internal.h — the pcapng reader's state, shared by gpd_pcapng.cpp and the runtime's
// gpd_decode_pcapng (not public ABI).  No HIP here: gpd_pcapng.cpp compiles alone with g++.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/gpd_pcapng.h"

namespace gpd {

struct NgPacket {
  uint64_t off;  // where the packet's bytes start in the buffer
  uint32_t caplen, wirelen, ifindex, linktype, ts_nsec;
  int64_t ts_sec;
};

}  // namespace gpd

// pcapgo.NgReader (ngread.go:42-58) over a buffer instead of a bufio.Reader.
struct gpd_pcapng_reader {
  const uint8_t *buf = nullptr;
  uint64_t len = 0;
  uint64_t pos = 0;      // the stream position (bufio's read pointer)
  uint64_t blk_pos = 0;  // header position of the block last read by read_block
  gpd_pcapng_opts opts{};
  gpd_pcapng_section_info section{};
  std::vector<gpd_pcapng_iface> ifaces;
  uint32_t linktype = 0;     // r.linkType
  uint32_t blk_type = 0;     // r.currentBlock.typ
  uint32_t blk_len = 0;      // r.currentBlock.length: what is left of the block, wrapping
  uint32_t opt_code = 0;     // r.currentOption.code
  gpd_pcapng_str opt_val{UINT64_MAX, 1024, 0};  // r.currentOption.value (make([]byte, 1024))
  bool first_found = false;  // r.firstSectionFound
  bool big_endian = false;   // r.bigEndian
  int stop = 0;              // GPD_PCAPNG_STOP_*: nonzero = the reader has stopped for good
  std::string err;           // its text

  // One ReadPacketData: 0 and *p set, or the stop (also kept in `stop`, text in `err`).
  int next_packet(gpd::NgPacket *p);
  int open();          // NewNgReader after the fields above are set
  int skip_section();  // SkipSection
  // gpd_decode_pcapng, after the device walk stopped at a state-changing block at `pos`: read
  // the section header, interface description and statistics blocks that follow, exactly as
  // next_packet's loop would on its way to the next packet, and stop in front of the first
  // block of another type.  0, or the stop.
  int absorb_state_blocks();
  // The text and return code of a stop, published to gpd_pcapng_last_error() and (in the
  // library) gpd_last_error_string(): GPD_OK for LIMIT / EOF, else GPD_ERR_PCAPNG.
  int result(int stop_code) const;
};
