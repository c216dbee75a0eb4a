// gpd_locate.h — where an application-layer message lies in its packet: the step the DNS and TLS
// hand-offs share (gpd_dns.hip, gpd_tls.hip).  For every candidate the generic decoder runs over
// the packet again; the message is the Payload of the last decoded layer's object.
#pragma once
#include <hip/hip_runtime.h>

#include "gpd_dev_generic.h"

namespace gpd {

// The last decoded layer's object: codes 1..4 are objects 0..3, the four IPv6 extension codes
// share object 4, codes 9..15 are objects 5..11 (gpd.h).
__device__ __forceinline__ uint32_t obj_of_code(uint32_t code) {
  return code <= 4u ? code - 1u : code <= 8u ? (uint32_t)GPD_OBJ_IPV6_EXT : code - 4u;
}

// Called by every lane of a grid of 256-lane workgroups with image_words * 4 bytes of dynamic
// LDS.  For candidate j < cnt, packet idx[j]: d_off[j], d_len[j] are its message inside the
// captured bytes, forced[j] is 1 when the packet's header offsets word or layer count is
// saturated (the message is the host's).
template <bool PAGES>
__device__ __forceinline__ void locate_payloads(const KParams &P, uint32_t cnt, const uint32_t *idx, uint32_t *d_off,
                                                uint32_t *d_len, uint32_t *forced) {
  if (cnt <= blockIdx.x * 256u) return;
  for (uint32_t k = threadIdx.x; k < P.image_words; k += 256) reinterpret_cast<uint32_t *>(g_lds)[k] = P.image[k];
  __syncthreads();
  const Tab<PAGES> T = make_tab<PAGES>(P);
  const uint32_t dlen = (uint32_t)P.data_len;
  const uint32_t options = (P.options & ~kDiagMask) | GPD_OPT_NO_CHECKSUMS | GPD_OPT_NO_FLOW_HASH;
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const uint32_t i = idx[j];
    const uint32_t off = min(P.offset[i], dlen), len = min(P.caplen[i], dlen - off);
    gpd_ext_rec e;
    decode_packet<true>(GlbSrc{P.data, off}, len, T, P.first, options, &e);
    // decoded's last element: the highest nonzero nibble of the 32 codes
    const uint64_t w = e.layer_codes[1] ? e.layer_codes[1] : e.layer_codes[0];
    const uint32_t code = w ? (uint32_t)(w >> ((63u - (uint32_t)__builtin_clzll(w)) & ~3u)) & 15u : 0u;
    const uint32_t obj = code ? obj_of_code(code) : (uint32_t)GPD_NOBJ;
    uint32_t p_off = 0, p_len = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)GPD_NOBJ; ++k)
      if (k == obj) {
        p_off = e.obj[k].payload_off;
        p_len = e.obj[k].payload_len;
      }
    if (p_off > len) p_off = len;  // (never: a Payload lies inside the packet)
    if (p_len > len - p_off) p_len = len - p_off;
    const uint32_t st = P.rec ? P.rec[i].status : P.status[i];
    const bool tp = code == GPD_C_TCP || code == GPD_C_UDP;
    const bool sat = GPD_STATUS_SATURATED(st) || (tp && GPD_HDR_TP(P.hdr_off[i]) == GPD_HDR_NONE);
    d_off[j] = p_off;
    d_len[j] = p_len;
    forced[j] = sat ? 1u : 0u;
  }
}

}  // namespace gpd
