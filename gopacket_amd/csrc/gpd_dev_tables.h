// gpd_dev_tables.h — the dispatch tables as the kernels read them from the image staged in LDS
// (layouts: gpd_internal.h): the generic decoder's Tab<PAGES> (sparse hashes in LDS, or two-level
// pages in global memory) and the fast decoders' fixed-layout bucket lookups.
#pragma once
#include "gpd_dev_common.h"

namespace gpd {

enum Dec : uint32_t {
  D_ETH, D_DOT1Q, D_IP4, D_IP6, D_IP6EXT, D_TCP, D_UDP, D_VXLAN, D_PAYLOAD, D_FRAG, D_ICMP4,
  D_LLC, D_NONE = 15
};

struct TE {        // a dispatch-table result
  uint32_t lt;     // LayerType (0: none / unknown)
  uint32_t ent;    // its type-LUT entry: decoder id (15 = not registered) | layer code << 4
};

template <bool PAGES>
struct Tab {
  const uint16_t *pages;
  uint32_t eth_base, tcp_base, udp_base, eth_bits, tcp_bits, udp_bits, eth_mult, tcp_mult, udp_mult;

  // type LUT (registered set applied by the host)
  __device__ __forceinline__ uint32_t lut(uint32_t t) const { return t < 128 ? g_lds[t] : 0xFFu; }
  __device__ __forceinline__ TE proto(uint32_t p) const {  // enums_generated.go:151-153
    const uint32_t v = lds_u32(4 * (kHashLutWords + (p & 0xFFu)));
    return TE{v & 0xFFFFu, v >> 16};
  }
  // Raw slot of `key` in a two-way bucketed hash: LayerType << 8 | LUT entry in the low 16
  // bits (0x00FF on a miss: LayerType 0, not registered).  One ds_read_b64, no loop.
  __device__ __forceinline__ uint32_t bucket(uint32_t base, uint32_t mult, uint32_t bits,
                                             uint32_t key) const {
    const uint32_t b = __builtin_amdgcn_ubfe(key * mult, 16 - bits, bits);
    const uint2 v = *reinterpret_cast<const uint2 *>(g_lds + 4 * base + 8 * b);
    return (v.x >> 16) == key ? v.x : ((v.y >> 16) == key ? v.y : 0xFFu);
  }
  __device__ __forceinline__ TE hash(uint32_t base, uint32_t mult, uint32_t bits, uint32_t key) const {
    const uint32_t r = bucket(base, mult, bits, key);
    return TE{(r >> 8) & 0xFFu, r & 0xFFu};
  }
  __device__ __forceinline__ TE page(uint32_t dir, uint32_t key) const {
    const uint32_t pg = pages[dir + (key >> 8)];
    const uint32_t lt = pages[kTabPages + pg * 256u + (key & 0xFFu)];
    return TE{lt, lut(lt)};
  }
  __device__ __forceinline__ TE eth(uint32_t et) const {  // enums_generated.go:77-79
    return PAGES ? page(kTabEthDir, et) : hash(eth_base, eth_mult, eth_bits, et);
  }
  __device__ __forceinline__ TE tcp(uint32_t port) const {  // ports.go:54-60 (raw)
    return PAGES ? page(kTabTcpDir, port) : hash(tcp_base, tcp_mult, tcp_bits, port);
  }
  __device__ __forceinline__ TE udp(uint32_t port) const {  // ports.go:97-103 (raw)
    return PAGES ? page(kTabUdpDir, port) : hash(udp_base, udp_mult, udp_bits, port);
  }
};
template <bool PAGES>
__device__ __forceinline__ Tab<PAGES> make_tab(const KParams &P) {
  return Tab<PAGES>{P.pages,    P.eth_base, P.tcp_base, P.udp_base, P.eth_bits,
                    P.tcp_bits, P.udp_bits, P.eth_mult, P.tcp_mult, P.udp_mult};
}

// TCP/UDP NextLayerType: dst port table, else src port table; 0 => Payload
// (tcp.go:308-314, udp.go:105-110).  Both lookups are issued together.
__device__ __forceinline__ TE ports_next(TE d, TE s, uint32_t payload_ent) {
  d = d.lt ? d : TE{(uint32_t)GPD_LT_PAYLOAD, payload_ent};
  s = s.lt ? s : TE{(uint32_t)GPD_LT_PAYLOAD, payload_ent};
  return d.lt != GPD_LT_PAYLOAD ? d : s;
}

// Lookup in a fixed-layout bucket hash (gpd_internal.h kFix*): raw slot, 0x00FF on a miss.
__device__ __forceinline__ uint32_t fix_bucket_at(uint32_t base, uint32_t mult, uint32_t key) {
  const uint32_t b = __builtin_amdgcn_ubfe(__umul24(key, mult), 16 - kFixBits, kFixBits);
  const uint2 v = *reinterpret_cast<const uint2 *>(g_lds + 8 * (base / 2 + b));
  return (v.x >> 16) == key ? v.x : ((v.y >> 16) == key ? v.y : 0xFFu);
}
template <uint32_t BASE>
__device__ __forceinline__ uint32_t fix_bucket(uint32_t mult, uint32_t key) {
  return fix_bucket_at(BASE, mult, key);
}

// TCP/UDP NextLayerType on raw slots (tcp.go:308-314, udp.go:105-110): the dst-port entry
// unless it is 0 or Payload, else the src-port entry (0 => Payload).
__device__ __forceinline__ uint32_t ports_next_raw(uint32_t rd, uint32_t rs, uint32_t pl_raw) {
  const uint32_t s = (rs & 0xFF00u) ? rs : pl_raw;
  return (rd & 0xFD00u) ? rd : s;
}

// Is this one of the EtherTypes the default tables map to Dot1Q?  Only a guess that lets the
// network header be fetched early; the table lookup still decides, and a packet whose
// lookups disagree with a guess goes to the generic decoder.
__device__ __forceinline__ uint32_t tag_type(uint32_t et) {
  return (et == 0x8100u || et == 0x88A8u) ? 1u : 0u;
}

}  // namespace gpd
