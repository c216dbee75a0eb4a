// gpd_dhcp_walk.h — (*DHCPv4).DecodeFromBytes (layers/dhcpv4.go:126-179, option decode :558-578)
// and (*DHCPv6).DecodeFromBytes (layers/dhcpv6.go:89-124, option decode
// dhcpv6_options.go:610-621) as one walker over a message's bytes, plain C++17 shared by the device
// kernels (gpd_dhcp.hip), the host entry point gpd_dhcp_decode_host and the stand-alone test
// program (tests/c/dhcp_walk_host.cpp).
//
// Both decodes are a fixed header and a loop over a TLV list with one offset as its state; they
// differ in the header and in the option framing.  The tests come in the reference's order, and
// `work` (include/gpd_dhcp.h) is the number of option decodes begun.
//
// The walker is templated on a sink that is told every appended option; the sizing sink ignores
// them (the walk's count is the result), the storing sink puts them into an array whose capacity
// is the sizing walk's count.  No array lives in the walker: nothing here can make a kernel use
// scratch memory.  Every byte is read as a byte, at an offset below len.
#pragma once
#include <stdint.h>

#include "../../include/gpd_dhcp.h"

#if defined(__HIPCC__)
#define GPD_DHCP_HD __host__ __device__ __forceinline__
#else
#define GPD_DHCP_HD inline
#endif

namespace gpd {

// The sizing sink.
struct DhcpCountSink {
  GPD_DHCP_HD void opt(uint32_t, uint32_t, uint32_t, uint32_t) const {}
};

// The storing sink: option k of the message to opts[k], inside the capacity, as one 8-byte store
// (opts is 16-byte aligned, an entry 8 bytes).
struct DhcpStoreSink {
  gpd_dhcp_opt *opts;
  uint32_t cap;
  GPD_DHCP_HD void opt(uint32_t k, uint32_t off, uint32_t code, uint32_t length) const {
    if (k >= cap) return;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t v2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<v2 *>(opts + k) = v2{off, code | (length << 16)};
#else
    opts[k] = gpd_dhcp_opt{off, (uint16_t)code, (uint16_t)length};
#endif
  }
};

struct DhcpWalk {
  uint64_t work = 0, max_options = 0;  // max_options 0: unbounded
  uint32_t n_opts = 0;                 // appended
};

// The record of a message that is the host's: no entries, everything but data_len and version zero.
GPD_DHCP_HD void dhcp_deferred(uint32_t version, uint32_t len, DhcpWalk &W, gpd_dhcp_msg &m) {
  m = gpd_dhcp_msg{};
  m.data_len = len;
  m.version = (uint8_t)version;
  m.verdict = (uint8_t)GPD_DHCP_DEFERRED;
  W.n_opts = 0;
}

GPD_DHCP_HD uint32_t dhcp_be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }

// d.DecodeFromBytes(data[:len]) of a DHCPv4 (version 4) or a DHCPv6 (version 6).  m.packet,
// data_off and first_opt are left zero.
template <class Sink>
GPD_DHCP_HD void dhcp_walk(uint32_t version, const uint8_t *d, uint32_t len, const Sink &sink, DhcpWalk &W,
                           gpd_dhcp_msg &m) {
  m = gpd_dhcp_msg{};
  m.data_len = len;
  m.version = (uint8_t)version;
  uint32_t verdict = GPD_DHCP_OK, truncated = 0, mflags = 0, err_arg = 0;
  uint32_t off = 0;  // where the reference returned
  if (version == 4u) {
    if (len < 240u) {                                            // dhcpv4.go:127-130
      truncated = 1;
      verdict = GPD_DHCP_E_V4_TOO_SHORT;
      err_arg = len;
    } else {
      m.op = d[0];                                               // :132-138
      m.htype = d[1];
      m.hlen = d[2];
      m.hops = d[3];
      m.xid = (dhcp_be16(d + 4) << 16) | dhcp_be16(d + 6);
      m.secs = (uint16_t)dhcp_be16(d + 8);
      m.flags = (uint16_t)dhcp_be16(d + 10);
      // :143 data[28 : 28+d.HardwareLen]: the sum is uint8 arithmetic.  From 228 up it wraps below
      // 28 and the slice expression panics for every message; below that it can pass len, where
      // the reference slices by capacity
      if (m.hlen < 228u && 28u + m.hlen > len) mflags |= GPD_DHCP_HW_PAST_DATA;
      if (m.hlen >= 228u) {
        verdict = GPD_DHCP_E_V4_HW_PANIC;
        err_arg = m.hlen - 228u;
        off = 28u;
      } else if (((dhcp_be16(d + 236) << 16) | dhcp_be16(d + 238)) != 0x63825363u) {  // :146-148
        verdict = GPD_DHCP_E_V4_BAD_MAGIC;
        off = 236u;
      } else if (len == 240u) {                                  // :150-153: nil, Contents not set
        off = len;
      } else {
        off = 240u;
        bool done = true;
        while (off < len) {                                      // :159-174
          if (++W.work > W.max_options && W.max_options != 0) {
            dhcp_deferred(version, len, W, m);
            return;
          }
          const uint32_t type = d[off];                          // :563
          if (type == GPD_DHCP_V4_END) break;                    // :164-166
          uint32_t length = 0;
          if (type != GPD_DHCP_V4_PAD) {
            const uint32_t rem = len - off;
            if (rem < 2u) {                                      // :568-570
              verdict = GPD_DHCP_E_V4_OPT_NO_DATA;
              done = false;
              break;
            }
            length = d[off + 1u];
            if (length > rem - 2u) {                             // :572-574
              verdict = GPD_DHCP_E_V4_OPT_MALFORMED;
              done = false;
              break;
            }
          }
          sink.opt(W.n_opts, off, type, length);                 // :167
          ++W.n_opts;
          off += type == GPD_DHCP_V4_PAD ? 1u : length + 2u;     // :169-173
        }
        if (done) {                                              // :176
          mflags |= GPD_DHCP_CONTENTS;
          off = len;
        }
      }
    }
  } else {
    if (len < 4u) {                                              // dhcpv6.go:90-93
      truncated = 1;
      verdict = GPD_DHCP_E_V6_TOO_SHORT;
      err_arg = len;
    } else {
      mflags |= GPD_DHCP_CONTENTS;                               // :94
      m.op = d[0];                                               // :96
      const bool relay = m.op == GPD_DHCP_V6_RELAY_FORWARD || m.op == GPD_DHCP_V6_RELAY_REPLY;
      if (relay && len < 34u) {                                  // :100-103
        truncated = 1;
        verdict = GPD_DHCP_E_V6_RELAY_SHORT;
        err_arg = len;
      } else {
        if (relay) {                                             // :104-107
          mflags |= GPD_DHCP_RELAY;
          m.hops = d[1];
          off = 34u;
        } else {                                                 // :109-110
          m.xid = ((uint32_t)d[1] << 16) | dhcp_be16(d + 2);
          off = 4u;
        }
        while (off < len) {                                      // :114-121
          if (++W.work > W.max_options && W.max_options != 0) {
            dhcp_deferred(version, len, W, m);
            return;
          }
          const uint32_t rem = len - off;
          if (rem < 4u) {                                        // dhcpv6_options.go:611-613
            verdict = GPD_DHCP_E_V6_OPT_NO_DATA;
            break;
          }
          const uint32_t code = dhcp_be16(d + off), length = dhcp_be16(d + off + 2u);
          if (rem < 4u + length) {                               // :616-618: the test in int, the
            verdict = GPD_DHCP_E_V6_OPT_SIZE;                    // text's argument in uint16
            err_arg = (4u + length) & 0xFFFFu;
            break;
          }
          sink.opt(W.n_opts, off, code, length);                 // dhcpv6.go:119
          ++W.n_opts;
          off += 4u + length;                                    // :120
        }
      }
    }
  }
  m.n_opts = W.n_opts;
  m.err_off = off;  // GPD_DHCP_OK: len
  m.err_arg = err_arg;
  m.verdict = (uint8_t)verdict;
  m.truncated = (uint8_t)truncated;
  m.mflags = (uint8_t)mflags;
}

}  // namespace gpd
