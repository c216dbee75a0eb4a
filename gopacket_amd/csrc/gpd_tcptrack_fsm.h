// gpd_tcptrack_fsm.h — reassembly's TCPSimpleFSM (reassembly/tcpcheck.go:119-246) as one step
// function, and the algebra the connection tracker (gpd_tcptrack.hip, include/gpd_tcptrack.h)
// scans with.  Plain C++17 for the host and the device: the kernels, the host program
// tests/c/tcptrack_fsm_host.cpp and nothing else include it.
//
// The FSM's whole state is (state 0..5, t.dir): 12 elements.  CheckState reads, besides that
// state, only the packet's SYN, ACK, FIN and RST bits, its direction and the creation option
// SupportMissingEstablishment (:168-246), so a packet is a map of the 12 elements to themselves.
// A map is 12 nibbles in a uint64_t, nibble e = the element that element e goes to; maps compose
// associatively, and the state before packet k of a connection is the composition of packets
// 0..k-1 applied to the state the connection carried in.  The 32 maps per option (4 flag bits
// and the direction) are derived from `step` at compile time: there is no second table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GPD_FSM_HD __host__ __device__
#else
#define GPD_FSM_HD
#endif

namespace gpd {
namespace fsm {

// tcpcheck.go:131-138
enum : uint32_t { kClosed = 0, kSynSent = 1, kEstablished = 2, kCloseWait = 3, kLastAck = 4, kReset = 5 };
// a packet's code: its four flags and its direction (1 = server to client, TCPDirServerToClient)
enum : uint32_t { kSyn = 1, kAck = 2, kFin = 4, kRst = 8, kDir = 16, kCodes = 32 };

struct Step {
  uint32_t state, tdir, accept;
};

// CheckState(tcp, dir) on (state, t.dir): the state after, t.dir after, and its result.
GPD_FSM_HD constexpr Step step(uint32_t state, uint32_t tdir, uint32_t code, bool missing_establishment) {
  const bool syn = code & kSyn, ack = code & kAck, fin = code & kFin, rst = code & kRst;
  const uint32_t dir = (code >> 4) & 1u;
  if (state == kClosed && missing_establishment && !(syn && !ack)) {  // :168-182
    if (syn && ack) {
      state = kSynSent;
      tdir = dir ^ 1u;
    } else if (fin && !ack) {
      state = kEstablished;
    } else if (fin && ack) {
      state = kCloseWait;
      tdir = dir ^ 1u;
    } else {
      state = kEstablished;
    }
  }
  switch (state) {
    case kClosed:  // :186-191
      if (syn && !ack) return Step{kSynSent, dir, 1u};
      break;
    case kSynSent:  // :192-205
      if (rst) return Step{kReset, tdir, 1u};
      if (syn && ack && dir == (tdir ^ 1u)) return Step{kEstablished, tdir, 1u};
      if (syn && !ack && dir == tdir) return Step{state, tdir, 1u};
      break;
    case kEstablished:  // :207-219
      if (rst) return Step{kReset, tdir, 1u};
      if (fin) return Step{kCloseWait, dir, 1u};
      return Step{state, tdir, 1u};
    case kCloseWait:  // :221-233
      if (rst) return Step{kReset, tdir, 1u};
      if (fin && ack && dir == (tdir ^ 1u)) return Step{kLastAck, tdir, 1u};
      if (ack) return Step{state, tdir, 1u};
      break;
    case kLastAck:  // :234-243
      if (rst) return Step{kReset, tdir, 1u};
      if (ack && tdir == dir) return Step{kClosed, tdir, 1u};
      break;
    default:  // kReset: no case, :245
      break;
  }
  return Step{state, tdir, 0u};
}

// ---- elements and the carried byte ---------------------------------------------------------------
constexpr uint32_t kElems = 12;
GPD_FSM_HD constexpr uint32_t elem(uint32_t state, uint32_t tdir) { return state + 6u * tdir; }
// the carried byte of include/gpd_tcptrack.h: state in bits 0..2, t.dir in bit 3
GPD_FSM_HD constexpr uint32_t elem_of_byte(uint32_t b) { return (b & 7u) + 6u * ((b >> 3) & 1u); }
GPD_FSM_HD constexpr uint32_t byte_of_elem(uint32_t e) { return e < 6u ? e : (e - 6u) | 8u; }
// the verdict byte: accept, the packet's direction, the state after, t.dir after
GPD_FSM_HD constexpr uint32_t verdict(const Step &s, uint32_t code) {
  return s.accept | (((code >> 4) & 1u) << 1) | (s.state << 2) | (s.tdir << 5);
}

// ---- maps -----------------------------------------------------------------------------------------
using Map = uint64_t;
constexpr Map kIdentity = 0xBA9876543210ull;
GPD_FSM_HD constexpr uint32_t apply(Map m, uint32_t e) { return (uint32_t)(m >> (4u * e)) & 15u; }
// a, then b.  Twelve nibble extracts: the index of each is data, so a byte permute (v_perm_b32
// selects among 8 bytes with a selector of its own) would need the map as 12 bytes in three
// words, three permutes and two selects per four elements; the shifts are fewer instructions.
GPD_FSM_HD constexpr Map compose(Map a, Map b) {
  Map r = 0;
  for (uint32_t e = 0; e < kElems; ++e) r |= (Map)apply(b, apply(a, e)) << (4u * e);
  return r;
}
GPD_FSM_HD constexpr Map generator(uint32_t code, bool missing_establishment) {
  Map r = 0;
  for (uint32_t e = 0; e < kElems; ++e) {
    const Step s = step(e % 6u, e / 6u, code, missing_establishment);
    r |= (Map)elem(s.state, s.tdir) << (4u * e);
  }
  return r;
}
struct GenTable {
  Map g[2][kCodes];  // [SupportMissingEstablishment][code]
};
constexpr GenTable make_gen_table() {
  GenTable t{};
  for (uint32_t o = 0; o < 2u; ++o)
    for (uint32_t c = 0; c < kCodes; ++c) t.g[o][c] = generator(c, o != 0u);
  return t;
}

}  // namespace fsm
}  // namespace gpd
