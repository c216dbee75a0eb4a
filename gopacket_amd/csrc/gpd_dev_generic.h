// gpd_dev_generic.h — the generic decoder: decode_packet, the DecodingLayerParser loop for one
// packet over any byte source, and the fallback lists through which the fast kernels hand it the
// packets their straight-line decode leaves (fb_append while streaming, decode_fallback_list at
// the end of the wave).
#pragma once
#include "gpd_dev_tables.h"

namespace gpd {

#define GPD_FAIL(code, x0, x1) \
  do { err = (code); a0 = (x0); a1 = (x1); goto fail; } while (0)

template <bool EXT, bool PAGES, class S>
__device__ __forceinline__ Out decode_packet(const S &s, uint32_t caplen, const Tab<PAGES> &T,
                                             uint32_t first, uint32_t options, gpd_ext_rec *ext,
                                             gpd_detail *det = nullptr) {
  uint32_t truncated = 0, err = 0, a0 = 0, a1 = 0;
  uint32_t ncount = 0;
  // decoded[0..11] in `codes` (the core word), [12..15] in hcodes, [16..31] in ecodes1
  uint64_t codes = 0, ecodes1 = 0;
  uint32_t hcodes = 0;
  uint32_t stop = 0, klass = GPD_ST_OK;
  // final state of the objects the fused outputs read: where their addresses / ports were read
  // (ip4_off, ip6_off, tcp_poff, udp_off) and their Contents+Payload (ip4_hl, tcp_off/tcp_tot,
  // udp_off/udp_tot) — the last successful decode of each kind, or what a failing call of that
  // kind assigned after it (the fail block)
  uint32_t ip4_off = 0, ip4_hl = 0, ip6_off = 0;
  uint32_t tcp_off = 0, tcp_tot = 0, tcp_poff = 0, udp_off = 0, udp_tot = 0;
  uint32_t err_dec = GPD_NOBJ_NONE, err_wrote = 0;
  uint32_t last_net = 0, last_tp = 0, tp_net = 0;  // net: 1 v4, 2 v6; tp: 1 TCP, 2 UDP
  uint32_t obj_valid = 0;
  gpd_layer_rec rec[EXT ? GPD_NOBJ : 1];

  uint32_t typ = first;
  uint32_t ent = T.lut(typ);
  uint32_t dec = ent & 15u;
  uint32_t off = 0, len = caplen;
  if (dec == D_NONE) {
    stop = typ;  // layers_decoder.go:12-17
  } else {
    for (;;) {
      uint32_t c_off = off, c_len, p_off, p_len, next;
      switch (dec) {
        case D_ETH: {  // ethernet.go:41-62
          if (len < 14) GPD_FAIL(GPD_E_ETH_TOO_SMALL, 0, 0);
          uint32_t w[1];
          load_words(s, off + 12, w);
          uint32_t et = ((w[0] & 0xFFu) << 8) | ((w[0] >> 8) & 0xFFu);
          c_len = 14; p_off = off + 14; p_len = len - 14;
          if (et < 0x0600u) {
            if (p_len < et) truncated = 1;
            else p_len = et;
            et = 0;  // EthernetTypeLLC
          }
          next = T.eth(et).lt;
          break;
        }
        case D_DOT1Q: {  // dot1q.go:29-40
          if (len < 4) { truncated = 1; GPD_FAIL(GPD_E_DOT1Q_TOO_SHORT, len, 0); }
          uint32_t w[1];
          load_words(s, off, w);
          c_len = 4; p_off = off + 4; p_len = len - 4;
          next = T.eth(be16_at(w, 2)).lt;
          break;
        }
        case D_IP4: {  // ip4.go:188-286
          if (len < 20) { truncated = 1; GPD_FAIL(GPD_E_IP4_TOO_SHORT, len, 0); }
          uint32_t w[3];
          load_words(s, off, w);  // bytes 0..11 (version/IHL .. protocol)
          uint32_t ihl = byte_at(w, 0) & 0x0Fu;
          uint32_t length = be16_at(w, 2);
          uint32_t ff = be16_at(w, 6);
          uint32_t proto = byte_at(w, 9);
          if (length == 0) length = len & 0xFFFFu;  // uint16(len(data))
          if (length < 20) GPD_FAIL(GPD_E_IP4_LENGTH_LT20, length, 0);
          if (ihl < 5) GPD_FAIL(GPD_E_IP4_IHL_LT5, ihl, 0);
          if (ihl * 4 > length) GPD_FAIL(GPD_E_IP4_IHL_GT_LENGTH, ihl, length);
          uint32_t dlen = len;
          if (len > length) {
            dlen = length;
          } else if (len < length) {
            truncated = 1;
            if (ihl * 4 > len) GPD_FAIL(GPD_E_IP4_HDR_TRUNC, 0, 0);
          }
          c_len = ihl * 4; p_off = off + c_len; p_len = dlen - c_len;
          for (uint32_t q = 20; q < c_len;) {  // options, ip4.go:240-273
            uint32_t rem = c_len - q;
            uint32_t t = s.u8(off + q);
            if (t == 0) break;
            if (t == 1) { q += 1; continue; }
            if (rem < 2) { truncated = 1; GPD_FAIL(GPD_E_IP4_OPT_LT2, rem, 0); }
            uint32_t ol = s.u8(off + q + 1);
            if (rem < ol) { truncated = 1; GPD_FAIL(GPD_E_IP4_OPT_EXCEEDS, t, ol); }
            if (ol <= 2) GPD_FAIL(GPD_E_IP4_OPT_LE2, t, ol);
            q += ol;
          }
          next = ((ff >> 13) & 1u) || (ff & 0x1FFFu) ? (uint32_t)GPD_LT_FRAGMENT : T.proto(proto).lt;
          break;
        }
        case D_IP6: {  // ip6.go:221-291
          if (len < 40) { truncated = 1; GPD_FAIL(GPD_E_IP6_TOO_SHORT, len, 0); }
          uint32_t w[2];
          load_words(s, off + 4, w);  // bytes 4..11: payload length, next header
          uint32_t length = be16_at(w, 0);
          uint32_t nh = byte_at(w, 2);
          c_len = 40; p_off = off + 40; p_len = len - 40;
          uint32_t use_nh = nh;
          if (nh == 0) {  // hop-by-hop parsed inside IPv6
            uint32_t hlen = p_len, hoff = p_off;
            if (hlen < 2) { truncated = 1; GPD_FAIL(GPD_E_IP6EXT_LT2, hlen, 0); }
            uint32_t hnh = s.u8(hoff), actual = s.u8(hoff + 1) * 8u + 8u;
            if (hlen < actual) GPD_FAIL(GPD_E_IP6EXT_LT_SPEC, hlen, actual);
            bool found = false;
            uint32_t jd = 0, jl = 0;
            for (uint32_t q = 2; q < actual;) {  // ip6.go:516-524 over data[offset:]
              uint32_t rem = hlen - q;
              if (rem < 2) { truncated = 1; GPD_FAIL(GPD_E_IP6_TLV_LT2, 0, 0); }
              uint32_t t = s.u8(hoff + q), act = 1;
              if (t != 0) {
                uint32_t ol = s.u8(hoff + q + 1);
                act = ol + 2;
                if (rem < act) { truncated = 1; GPD_FAIL(GPD_E_IP6_TLV_TRUNC, 0, 0); }
                if (t == 0xC2u && !found) { found = true; jd = q + 2; jl = ol; }
              }
              q += act;
            }
            uint32_t jumbo_len = 0;
            bool jumbo = false;
            if (found) {  // getIPv6HopByHopJumboLength, ip6.go:54-76
              if (jl != 4) GPD_FAIL(GPD_E_IP6_JUMBO_TLV_LEN, 0, 0);
              jumbo_len = (s.u8(hoff + jd) << 24) | (s.u8(hoff + jd + 1) << 16) |
                          (s.u8(hoff + jd + 2) << 8) | s.u8(hoff + jd + 3);
              if (jumbo_len <= 65535u) GPD_FAIL(GPD_E_IP6_JUMBO_TOO_SMALL, 0, 0);
              jumbo = true;
            }
            use_nh = hnh;
            if (jumbo && length == 0) {
              if (jumbo_len > p_len) truncated = 1;
              else p_len = jumbo_len;  // payload still starts at the HBH header (ip6.go:255)
              next = T.proto(use_nh).lt;
              break;
            } else if (jumbo) {
              GPD_FAIL(GPD_E_IP6_JUMBO_AND_LEN, 0, 0);
            } else if (length == 0) {
              GPD_FAIL(GPD_E_IP6_LEN0_NO_JUMBO, 0, 0);
            }
            p_off += actual;
            p_len -= actual;
          }
          if (length == 0) GPD_FAIL(GPD_E_IP6_LEN0_NOT_HBH, nh, 0);
          if (length > p_len) truncated = 1;
          else p_len = length;
          next = T.proto(use_nh).lt;
          break;
        }
        case D_IP6EXT: {  // ip6.go:418-432,443-461
          if (len < 2) { truncated = 1; GPD_FAIL(GPD_E_IP6EXT_LT2, len, 0); }
          uint32_t w[1];
          load_words(s, off, w);
          uint32_t actual = byte_at(w, 1) * 8u + 8u;
          if (len < actual) GPD_FAIL(GPD_E_IP6EXT_LT_SPEC, len, actual);
          c_len = actual; p_off = off + actual; p_len = len - actual;
          next = T.proto(byte_at(w, 0)).lt;
          break;
        }
        case D_TCP: {  // tcp.go:229-314
          if (len < 20) { truncated = 1; GPD_FAIL(GPD_E_TCP_TOO_SHORT, len, 0); }
          uint32_t w[4];
          load_words(s, off, w);  // bytes 0..15: ports .. flags
          const TE ld = T.tcp(be16_at(w, 2)), ls = T.tcp(be16_at(w, 0));
          uint32_t doff = byte_at(w, 12) >> 4;
          if (doff < 5) GPD_FAIL(GPD_E_TCP_DOFF_LT5, doff, 0);
          uint32_t ds = doff * 4;
          if (ds > len) { truncated = 1; GPD_FAIL(GPD_E_TCP_DOFF_GT_LEN, 0, 0); }
          c_len = ds; p_off = off + ds; p_len = len - ds;
          for (uint32_t q = 20; q < ds;) {  // OPTIONS, tcp.go:274-300
            uint32_t rem = ds - q;
            uint32_t k = s.u8(off + q), ol = 1;
            if (k == 0) break;
            if (k != 1) {
              if (rem < 2) { truncated = 1; GPD_FAIL(GPD_E_TCP_OPT_LT2_REM, rem, 0); }
              ol = s.u8(off + q + 1);
              if (ol < 2) GPD_FAIL(GPD_E_TCP_OPT_LEN_LT2, ol, 0);
              if (ol > rem) { truncated = 1; GPD_FAIL(GPD_E_TCP_OPT_EXCEEDS, ol, rem); }
            }
            q += ol;
          }
          next = ports_next(ld, ls, 0).lt;
          break;
        }
        case D_UDP: {  // udp.go:30-56,105-110
          if (len < 8) { truncated = 1; GPD_FAIL(GPD_E_UDP_TOO_SHORT, len, 0); }
          uint32_t w[2];
          load_words(s, off, w);
          const TE ld = T.udp(be16_at(w, 2)), ls = T.udp(be16_at(w, 0));
          uint32_t length = be16_at(w, 4);
          c_len = 8; p_off = off + 8;
          if (length >= 8) {
            uint32_t hlen = length;
            if (hlen > len) { truncated = 1; hlen = len; }
            p_len = hlen - 8;
          } else if (length == 0) {
            p_len = len - 8;
          } else {
            GPD_FAIL(GPD_E_UDP_LEN_TOO_SMALL, length, 0);
          }
          next = ports_next(ld, ls, 0).lt;
          break;
        }
        case D_VXLAN: {  // vxlan.go:53-78
          if (len < 8) GPD_FAIL(GPD_E_VXLAN_TOO_SMALL, 0, 0);
          c_len = 8; p_off = off + 8; p_len = len - 8;
          next = GPD_LT_ETHERNET;
          break;
        }
        case D_ICMP4: {  // icmp4.go:220-231; NextLayerType :261-263
          if (len < 8) { truncated = 1; GPD_FAIL(GPD_E_ICMP4_TOO_SMALL, 0, 0); }
          c_len = 8; p_off = off + 8; p_len = len - 8;
          next = GPD_LT_PAYLOAD;
          break;
        }
        case D_LLC: {  // llc.go:31-52; NextLayerType :61-69
          if (len < 3) GPD_FAIL(GPD_E_LLC_TOO_SMALL, 0, 0);
          const uint32_t dsap = s.u8(off) & 0xFEu, ssap = s.u8(off + 1) & 0xFEu;
          const uint32_t ctl = s.u8(off + 2);
          c_len = 3;
          if (!(ctl & 1u) || (ctl & 3u) == 1u) {  // two-byte control field
            if (len < 4) GPD_FAIL(GPD_E_LLC_TOO_SMALL, 0, 0);
            c_len = 4;
          }
          p_off = off + c_len; p_len = len - c_len;
          next = (dsap == 0xAAu && ssap == 0xAAu) ? (uint32_t)GPD_LT_SNAP
               : (dsap == 0x42u && ssap == 0x42u) ? (uint32_t)GPD_LT_STP : (uint32_t)GPD_LT_ZERO;
          break;
        }
        default: {  // Payload / Fragment: all of it; LayerPayload nil; next Zero
          c_len = len; p_off = off + len; p_len = 0;
          next = GPD_LT_ZERO;
          break;
        }
      }
      // *decoded = append(*decoded, typ)
      {
        const uint64_t code = ent >> 4;
        if (ncount < GPD_CORE_MAX_LAYERS) codes |= code << (16 + 4 * ncount);
        else if (ncount < 16) hcodes |= (uint32_t)code << (4 * (ncount - GPD_CORE_MAX_LAYERS));
        else if (ncount < 32) ecodes1 |= code << (4 * (ncount - 16));
        ncount++;
      }
      obj_valid |= 1u << dec;  // Dec order == enum gpd_obj order
      if (EXT) {
#pragma unroll
        for (int k = 0; k < GPD_NOBJ; k++)
          if ((uint32_t)k == dec) rec[k] = gpd_layer_rec{c_off, c_len, p_off, p_len};
      }
      if (dec == D_IP4) { ip4_off = c_off; ip4_hl = c_len; last_net = 1; }
      else if (dec == D_IP6) { ip6_off = c_off; last_net = 2; }
      else if (dec == D_TCP) { tcp_off = tcp_poff = c_off; tcp_tot = c_len + p_len; last_tp = 1; tp_net = last_net; }
      else if (dec == D_UDP) { udp_off = c_off; udp_tot = c_len + p_len; last_tp = 2; tp_net = last_net; }
      typ = next;
      off = p_off;
      len = p_len;
      if (len == 0) break;  // layers_decoder.go:71-73
      ent = T.lut(typ);
      dec = ent & 15u;
      if (dec == D_NONE) { stop = typ; break; }
    }
  }
  goto done;
fail:
  klass = GPD_ST_DECODE_ERROR;
  {
    // What the failing DecodeFromBytes assigned to its reused object before returning
    // (gpd.h gpd_ext_rec.err_wrote): header fields from `off` (1), and BaseLayer too (2).
    uint32_t ec_len = 0, ep_off = 0, ep_len = 0;
    if (dec == D_IP4 && err != GPD_E_IP4_TOO_SHORT) {  // ip4.go:195-210, 235-236
      err_wrote = 2;
      ec_len = len; ep_off = off + len;                // Contents = data, Payload nil
      if (err >= GPD_E_IP4_OPT_LT2) {                  // options: the header split stands
        uint32_t w[1];
        load_words(s, off, w);
        uint32_t length = be16_at(w, 2);
        if (length == 0) length = len & 0xFFFFu;
        ec_len = (byte_at(w, 0) & 0x0Fu) * 4u;
        ep_off = off + ec_len;
        ep_len = min(len, length) - ec_len;
      }
    } else if (dec == D_IP6 && err != GPD_E_IP6_TOO_SHORT) {  // ip6.go:226-235
      err_wrote = 2;
      ec_len = 40; ep_off = off + 40; ep_len = len - 40;
    } else if (dec == D_TCP && err != GPD_E_TCP_TOO_SHORT) {  // tcp.go:234-268
      err_wrote = err == GPD_E_TCP_DOFF_LT5 ? 1u : 2u;
      ec_len = len; ep_off = off + len;                // doff overrun: Contents = data
      if (err >= GPD_E_TCP_OPT_LT2_REM) {              // options: the header split stands
        ec_len = (s.u8(off + 12) >> 4) * 4u;
        ep_off = off + ec_len;
        ep_len = len - ec_len;
      }
    } else if (dec == D_UDP && err == GPD_E_UDP_LEN_TOO_SMALL) {  // udp.go:35-41
      err_wrote = 2;
      ec_len = 8; ep_off = off + 8;                    // Contents = data[:8], Payload nil
    } else if (dec == D_LLC && len >= 3) {             // llc.go:35-39
      err_wrote = 1;
    }
    err_dec = dec;
    if (err_wrote && ((obj_valid >> dec) & 1u)) {  // only kinds in decoded feed the outputs
      if (dec == D_IP4) { ip4_off = off; ip4_hl = ec_len; }
      else if (dec == D_IP6) ip6_off = off;
      else if (dec == D_TCP) {
        tcp_poff = off;
        if (err_wrote == 2) { tcp_off = off; tcp_tot = ec_len + ep_len; }
      } else if (dec == D_UDP) { udp_off = off; udp_tot = 8; }
    }
    if (EXT && err_wrote == 2) {
#pragma unroll
      for (int k = 0; k < GPD_NOBJ; k++)
        if ((uint32_t)k == dec) rec[k] = gpd_layer_rec{off, ec_len, ep_off, ep_len};
    }
  }
done:
  if (klass != GPD_ST_DECODE_ERROR && stop != 0)
    klass = (options & GPD_OPT_IGNORE_UNSUPPORTED) ? GPD_ST_OK : GPD_ST_UNSUPPORTED;

  uint32_t st = klass | (truncated << 2);
  st |= (ncount > 31 ? 1u : 0u) << 3;
  st |= (ncount > 31 ? 31u : ncount) << 4;
  if (klass == GPD_ST_DECODE_ERROR) st |= err << 9;

  uint64_t nhash = 0, thash = 0;
  uint32_t cs = 0;
  st |= (last_net << 20) | (last_tp ? (last_tp == 1 ? 4u : 5u) << 24 : 0u);  // endpoint types
  uint32_t v4[2] = {0, 0};  // ip4 src/dst words, shared by the net hash and the pseudo-header
  if (last_net == 1 || (last_tp && tp_net == 1)) load_words(s, ip4_off + 12, v4);
  if (!(options & GPD_OPT_NO_FLOW_HASH)) {
    if (last_net == 1) {  // ip4.NetworkFlow(), ip4.go:63-65
      nhash = flow_fast(fnv_start<4>(v4[0]), fnv_start<4>(v4[1]), 1u);
      st |= 1u << 16;
    } else if (last_net == 2) {  // ip6.NetworkFlow(), ip6.go:49-51
      uint32_t w[8];
      load_words(s, ip6_off + 8, w);
      const H64 hs = fnv_more(fnv_more(fnv_more(fnv_start<4>(w[0]), w[1]), w[2]), w[3]);
      const H64 hd = fnv_more(fnv_more(fnv_more(fnv_start<4>(w[4]), w[5]), w[6]), w[7]);
      nhash = flow_fast(hs, hd, 2u);
      st |= 1u << 16;
    }
    if (last_tp) {  // tcp/udp.TransportFlow(), tcp.go:331-333, udp.go:123-125
      uint32_t w[1];
      load_words(s, last_tp == 1 ? tcp_poff : udp_off, w);
      uint32_t ept = last_tp == 1 ? 4u : 5u;
      thash = flow_fast(fnv_start<2>(w[0]), fnv_start<2>(w[0] >> 16), ept);
      st |= 1u << 17;
    }
  }
  if (!(options & GPD_OPT_NO_CHECKSUMS)) {
    // checksum(ip4.Contents), ip4.go:158-179; an odd-length Contents (a failed Length/IHL
    // check keeps all of data) makes `checksum` index past the end: a panic, no value
    if ((obj_valid & (1u << D_IP4)) && !(ip4_hl & 1u)) {
      uint32_t h[5];
      load_words(s, ip4_off, h);
      h[2] &= 0x0000FFFFu;  // bytes 10-11 read as zero
      uint32_t E = 0, O = 0;
#pragma unroll
      for (int k = 0; k < 5; k++) {
        E = __builtin_amdgcn_udot4(h[k], 0x00010001u, E, false);
        O = __builtin_amdgcn_udot4(h[k], 0x01000100u, O, false);
      }
      uint32_t sum = (E << 8) + O;
      if (ip4_hl > 20) sum += be16_sum(s, ip4_off + 20, ip4_hl - 20);
      cs |= fold_not(sum);
      st |= 1u << 18;
    }
    if (last_tp && tp_net) {  // tcp.ComputeChecksum(), tcp.go:193-195 / tcpip.go:75-88
      uint32_t ps;
      if (tp_net == 1) {
        ps = (__builtin_amdgcn_udot4(v4[0], 0x00010001u, 0, false) +
              __builtin_amdgcn_udot4(v4[1], 0x00010001u, 0, false)) * 256u +
             __builtin_amdgcn_udot4(v4[0], 0x01000100u, 0, false) +
             __builtin_amdgcn_udot4(v4[1], 0x01000100u, 0, false);
      } else {
        ps = be16_sum(s, ip6_off + 8, 32);
      }
      uint32_t toff = last_tp == 1 ? tcp_off : udp_off;
      uint32_t tot = last_tp == 1 ? tcp_tot : udp_tot;
      ps += last_tp == 1 ? 6u : 17u;
      ps += tot & 0xFFFFu;
      ps += tot >> 16;
      cs |= (uint32_t)fold_not(ps + be16_sum(s, toff, tot)) << 16;
      st |= 1u << 19;
    }
  }
  Out o;
  o.status = st;
  o.layers = codes | (stop & 0xFFFFu);
  o.net_hash = nhash;
  o.tp_hash = thash;
  o.csum = cs;
  o.hoff = hdr_word(last_net != 0, last_net == 1 ? ip4_off : ip6_off, last_tp != 0,
                    last_tp == 1 ? tcp_poff : udp_off);
  // decoded[0..15] as the ext / detail records hold them (the core word's 12 codes + hcodes)
  const uint64_t ecodes0 = (codes >> 16) | ((uint64_t)hcodes << 48);
  if (det && (klass == GPD_ST_DECODE_ERROR || ncount > GPD_CORE_MAX_LAYERS)) {  // gpd.h gpd_detail
    gpd_detail d;
    d.layer_codes[0] = ecodes0;
    d.layer_codes[1] = ecodes1;
    d.err_arg0 = klass == GPD_ST_DECODE_ERROR ? a0 : 0;
    d.err_arg1 = klass == GPD_ST_DECODE_ERROR ? a1 : 0;
    *det = d;
  }
  if (EXT) {
    gpd_ext_rec e;
    e.layer_codes[0] = ecodes0;
    e.layer_codes[1] = ecodes1;
    e.err_arg0 = klass == GPD_ST_DECODE_ERROR ? a0 : 0;
    e.err_arg1 = klass == GPD_ST_DECODE_ERROR ? a1 : 0;
    e.obj_valid = (uint16_t)obj_valid;
    e.err_obj = (uint8_t)err_dec;  // Dec order == enum gpd_obj order
    e.err_wrote = (uint8_t)err_wrote;
    e.err_off = klass == GPD_ST_DECODE_ERROR ? off : 0;
#pragma unroll
    for (int k = 0; k < GPD_NOBJ; k++)
      e.obj[k] = ((obj_valid >> k) & 1u) || ((uint32_t)k == err_dec && err_wrote == 2)
                     ? rec[k] : gpd_layer_rec{0, 0, 0, 0};
    *ext = e;
  }
  return o;
}
#undef GPD_FAIL

// A tile's leftovers (the lanes with fb set: packet i at offset off) appended to the wave's
// region of the fallback list, which starts at fb_start and holds fb_c entries so far; returns
// the new count.  (ro_kernel and sp_kernel; rs_kernel keeps its copy inline.)
__device__ __forceinline__ uint32_t fb_append(const KParams &P, uint32_t fb_start, uint32_t fb_c, uint32_t i,
                                              uint32_t off, uint32_t fb) {
  const uint64_t m = __ballot(fb != 0);
  if (m) {
    if (fb) P.fb_list[fb_start + fb_c + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                           __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = ((uint64_t)off << 32) | i;
    fb_c += (uint32_t)__popcll(m);
  }
  return fb_c;
}

// The end of a fast wave: its fallback list — the generic DecodingLayerParser loop
// (decode_packet), one lane per listed packet, its bytes read from global memory — here, at the
// end of the wave, overlapped with the other waves' streaming.  (A second kernel over the lists
// cost a launch boundary, ~5 us per launch, even when every list is empty.)  The live state of
// the streaming loop is dead by now, so the generic decoder's registers do not raise the
// kernel's.  Each round first stages every listed packet's first K bytes in the lane's slot of
// the (now idle) window buffer `buf` with independent 16-byte loads, so the decoder's dependent
// header reads hit LDS (HybSrc); bytes past the slot (long segments) still come from global
// memory.
template <uint32_t K, bool CS = true, bool HASH = true>
__device__ __forceinline__ void decode_fallback_list(const KParams &P, uint32_t buf, uint32_t fb_start, uint32_t fb_c,
                                                     uint32_t lane, uint32_t dlen, uint32_t options) {
#if GPD_EXP & 8
  return;  // (A/B diagnostic build, tools/mix_diag.sh: the generic decodes skipped, wrong results)
#endif
#if GPD_EXP & 64
  options |= GPD_OPT_NO_FLOW_HASH;  // (A/B diagnostic: the generic decodes' hashes skipped)
#endif
#if GPD_EXP & 128
  options |= GPD_OPT_NO_CHECKSUMS;  // (A/B diagnostic: the generic decodes' checksums skipped)
#endif
  const uint32_t tot = fb_c;
  if (tot) {
    __threadfence_block();  // the entries other lanes of this wave stored
    const Tab<false> T = make_tab<false>(P);
    const uint32_t slot = buf + K * lane;
    // readable bound of the batch contract (gpd.h gpd_batch: round_up(data_len, 16)): every
    // 16-byte chunk below it is whole, so no staging load reaches past it
    const uint64_t rlim = ((uint64_t)dlen + 15u) & ~15ull;
    // round j's descriptors and first K bytes; the next round's are fetched before this round
    // decodes (registers are free at the wave's end), so their three dependent global loads
    // (list entry, descriptor, bytes) overlap the decode instead of preceding it
    struct Fetch {
      uint32_t fi, off, len;
      v4u32 c[K / 16u];
    };
    auto fetch = [&](uint32_t j, Fetch &f) {
      const bool live = j < tot;
      const uint64_t e = live ? P.fb_list[fb_start + j] : 0ull;
      f.fi = (uint32_t)e;
      f.off = (uint32_t)(e >> 32);  // (clamped to dlen when listed)
      f.len = live ? min(P.caplen[f.fi], dlen - f.off) : 0u;
      const uint64_t gb = (uint64_t)f.off & ~15ull;
#pragma unroll
      for (uint32_t k = 0; k < K / 16u; k++)
        f.c[k] = (live && gb + 16u * k < rlim) ? *reinterpret_cast<const v4u32 *>(P.data + gb + 16u * k)
                                                : v4u32{0u, 0u, 0u, 0u};
    };
    Fetch cur;
    fetch(lane, cur);
    for (uint32_t j = lane; j - lane < tot; j += 64u) {
      const bool live = j < tot;
#pragma unroll
      for (uint32_t k = 0; k < K / 16u; k++) *reinterpret_cast<v4u32 *>(g_lds + slot + 16u * k) = cur.c[k];
      Fetch nxt;
      if (j + 64u - lane < tot) fetch(j + 64u, nxt);  // (wave-uniform)
      const uint32_t fi = cur.fi, off = cur.off, len = cur.len;
      const uint64_t gb = (uint64_t)off & ~15ull;
      // a round whose packets all lie inside their slots reads LDS only (no per-read bound)
      const bool all_in = __all(!live || (off & 15u) + len <= K);
#if GPD_EXP & 32
      if (live) {  // (A/B diagnostic: fetch, stage and store only)
        Out o{cur.c[0].x + (uint32_t)all_in, 0, 0, 0, 0, 0};
        store_out(P, fi, o);
      }
      cur = nxt;
      continue;
#endif
      if (live) {
        gpd_detail *det = P.detail ? P.detail + fi : nullptr;
        if (all_in)
          store_out(P, fi, decode_packet<false>(LdsSrc<false>{slot, off & 15u}, len, T, P.first, options, nullptr, det));
        else
          store_out(P, fi, decode_packet<false>(HybSrc<K>{P.data, off, gb, slot}, len, T, P.first, options, nullptr, det));
      }
      cur = nxt;
    }
  }
}

}  // namespace gpd
