// gpd_dev_fast.h — the straight-line decoder the fast kernels (rs_kernel, ro_kernel, sp_kernel)
// share: fast_decode, the header-once staging around it (hdr_parse, seg_pass) and the window
// commit / chunk prefix-sum helpers of their streaming loops.
#pragma once
#include "gpd_dev_tables.h"

namespace gpd {

// Straight-line decode of the stacks that carry nearly all traffic:
//   Ethernet [Dot1Q]{0,2} (IPv4 with IHL 5 | IPv6 without hop-by-hop) (TCP | UDP | ICMPv4)
//     [Payload | VXLAN + the same stack once more]
// for a packet in an LDS window, with Ethernet as the first layer.  Header offsets are
// runtime values and every header is read straight from LDS at its own byte address
// (gfx950 DS instructions take unaligned addresses), so one code path serves every tag
// count and both VXLAN passes.  The parse only records where the objects the fused outputs
// read ended up (the last IPv4 header, the last network layer, the last transport); the
// checksums and hashes are computed once at the end from LDS.  A lane whose packet leaves
// the envelope (IPv4 options, fragments, hop-by-hop, any decode error, unusual table
// mappings...) returns false having written nothing, and the packet goes to the generic
// decoder, so the results are those of decode_packet in every case.
//
// Instruction economy (the kernel is VALU-issue bound once the bytes are in LDS):
//  * checksums are summed in the little-endian domain with v_dot2_u32_u16 (one op per
//    4 bytes, no byte shuffles) and converted once at the end (fold_le_not);
//  * FNV-1a multiplies use the 2^40 + 0x1b3 split, with the first byte from the basis in
//    closed form;
//  * table lookups are one ds_read_b64 of a two-way bucket and two compares.

// LDS reads at any byte address
struct __attribute__((packed, aligned(1))) U128 {
  uint32_t x, y, z, w;
};
__device__ __forceinline__ U128 ld128(uint32_t a) { return *reinterpret_cast<const U128 *>(g_lds + a); }

// big-endian 16-bit value of bytes (0,1) / (2,3) of a little-endian word
__device__ __forceinline__ uint32_t be_lo(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0C0C0001u); }
__device__ __forceinline__ uint32_t be_hi(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0C0C0203u); }

struct FastCtx {        // wave-uniform facts about the registered set and the options
  uint32_t mult;        // the fixed-layout hash multiplier
  uint32_t pl_raw;      // Payload as a raw slot: LayerType 2 << 8 | its LUT entry
  uint32_t unsup;       // status class of a nonzero stop type (IgnoreUnsupported -> OK)
  uint32_t fr_ent;      // Fragment's LUT entry (decoder id D_FRAG when registered, else 15)
};
// ... read from the staged image (after the barrier that follows stage_image)
__device__ __forceinline__ FastCtx fast_ctx(const KParams &P, uint32_t options) {
  return FastCtx{P.eth_mult, ((uint32_t)GPD_LT_PAYLOAD << 8) | (reinterpret_cast<const uint8_t *>(g_lds)[GPD_LT_PAYLOAD]),
                 (options & GPD_OPT_IGNORE_UNSUPPORTED) ? GPD_ST_OK : GPD_ST_UNSUPPORTED,
                 reinterpret_cast<const uint8_t *>(g_lds)[GPD_LT_FRAGMENT]};
}

// The 64 bytes from a network header on (it and the first 16 bytes after it need <= 56),
// as four ds_read_b128 at the header's own byte address.  Misaligned, each costs ~3.6x an
// aligned one on gfx950, but aligned dword reads of the same bytes are slower still when
// packets sit at power-of-two strides (bank conflicts: tools/micro/lds_align.hip).
__device__ __forceinline__ void load64(uint32_t (&W)[16], uint32_t a) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const U128 q = ld128(a + 16 * k);
    W[4 * k] = q.x; W[4 * k + 1] = q.y; W[4 * k + 2] = q.z; W[4 * k + 3] = q.w;
  }
}

// A long transport segment left to the wave-cooperative sum (COOP): its partial LE-domain
// sum (pseudo-header, head and tail chunks) and the aligned 16-byte chunks [a, b) of the
// window between them, whose sum is a difference of the window's chunk prefix sums.
struct Seg {
  uint32_t part, a, b;
};

// P[c] = LE-domain sum of the window's 16-byte chunks below c, for c in [0, STAGE/16],
// written to LDS at pfx.  Lane l sums chunks [K l, K l + K), K = STAGE/1024; bytes past the
// window's end only reach entries beyond it.
template <int STAGE>
__device__ __forceinline__ void window_prefix(uint32_t buf, uint32_t pfx, uint32_t lane) {
  constexpr int K = STAGE / 1024;
  uint32_t c[K];
#pragma unroll
  for (int j = 0; j < K; j++) {
    const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + buf + 16u * K * lane + 16u * j);
    c[j] = dot2(q.w, 0x00010001u, dot2(q.z, 0x00010001u,
                dot2(q.y, 0x00010001u, dot2(q.x, 0x00010001u, 0u))));
  }
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const uint32_t v = c[j];
    c[j] = run;  // exclusive within the block
    run += v;
  }
  const uint32_t incl = wave_incl_scan(run), base = incl - run;
  uint4 *d = reinterpret_cast<uint4 *>(g_lds + pfx + 4u * K * lane);
#pragma unroll
  for (int j = 0; j < K / 4; j++)
    d[j] = uint4{base + c[4 * j], base + c[4 * j + 1], base + c[4 * j + 2], base + c[4 * j + 3]};
  if (lane == 63u) *reinterpret_cast<uint32_t *>(g_lds + pfx + 4u * K * 64u) = incl;
}

// TCP options the walk (tcp.go:274-300) accepts without reading them byte by byte: none, or
// exactly NOP, NOP, Timestamps (kind 8, length 10) — what established connections carry.  w:
// the first four option bytes (TCP header bytes 20..23) as a little-endian word.
__device__ __forceinline__ bool tcp_opts_quick(uint32_t hl, uint32_t w) {
  return hl == 20u || (hl == 32u && w == 0x0A080101u);
}

// Header-once decode (rs_kernel HO, windows of long frames): a tile of 64 such packets spans
// several windows, and a straight-line decode per window would run with the few lanes whose
// packets that window holds.  Instead, in the window that holds a packet, seg_pass keeps
// the bytes the decode reads in the lane's registers and sums the transport segment the
// decode will checksum; after the tile's last window fast_decode<HO> runs once for all 64
// lanes from those registers.
struct Hdr {
  uint32_t e1, e2, e3;  // frame bytes 12..23: EtherType and up to two tags (ld128(p + 8).y/z/w)
  uint32_t W[16];       // the 64 bytes from the network header on
  uint32_t pos;         // tp_off | tp_len << 16 of the segment summed (0xFFFFFFFF: none)
  uint32_t sum;         // its LE-domain byte sum, pseudo-header not included
  uint32_t ok;          // its TCP options parse (tcp.go:274-300); 2: a VXLAN payload follows
};

// The LE-domain sum s + bytes [S, S + len) of the window, read as its first 16-byte chunk, the
// whole chunks after it and the ragged tail (TCP.ComputeChecksum's loop, tcpip.go:52-88).
__device__ __forceinline__ uint32_t seg_sum_chunks(uint32_t S, uint32_t len, uint32_t s) {
  const U128 c0 = ld128(S), ct = ld128(S + (len & ~15u));
  const uint32_t w0 = len >= 16u ? 0x00010001u : 0u;  // first whole chunk
  s = dot2(c0.x, w0, s);
  s = dot2(c0.y, w0, s);
  s = dot2(c0.z, w0, s);
  s = dot2(c0.w, w0, s);
  const uint32_t r8 = (len & 15u) * 8u;  // ragged tail: an odd last byte is its half's low byte
  uint64_t lo = ((uint64_t)ct.y << 32) | ct.x, hi = ((uint64_t)ct.w << 32) | ct.z;
  lo = r8 >= 64u ? lo : (r8 ? (lo << (64u - r8)) >> (64u - r8) : 0ull);
  hi = r8 > 64u ? (hi << (128u - r8)) >> (128u - r8) : 0ull;
  s = dot2((uint32_t)lo, 0x00010001u, s);
  s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
  s = dot2((uint32_t)hi, 0x00010001u, s);
  s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
  const uint32_t xt = len & ~15u;
  for (uint32_t x = 16; x < xt; x += 16u) {
    const U128 q = ld128(S + x);
    s = dot2(q.x, 0x00010001u, s);
    s = dot2(q.y, 0x00010001u, s);
    s = dot2(q.z, 0x00010001u, s);
    s = dot2(q.w, 0x00010001u, s);
  }
  return s;
}

// hdr_parse: the first round trip of fast_decode (the Ethernet and network header bytes) kept
// in h, and the transport segment that fast_decode's guesses lead to (IPv4 IHL 5 / IPv6 by the
// version nibble, TCP / UDP by the protocol number, UDP Length): h.pos and (l4, seg); false
// when there is none.  Reads the packet's first 128 bytes at most (a TCP options walk).
// fast_decode<HO> confirms the guesses with the dispatch tables and uses the segment's sum only
// when its own transport segment is exactly h.pos (else the packet takes the generic decoder).
// With VXLAN registered (vxreg), a UDP segment whose ports lead to it is flagged (h.ok = 2) for
// the full decode in the window that holds it: its inner headers are not staged.
__device__ __forceinline__ bool hdr_parse(uint32_t p, uint32_t len, Hdr &h, const FastCtx &F, bool vxreg,
                                          uint32_t &l4_out, uint32_t &seg_out) {
  h.pos = 0xFFFFFFFFu;
  h.sum = 0;
  h.ok = 0;
  if (len < 15u) return false;
  const U128 e = ld128(p + 8);
  h.e1 = e.y;
  h.e2 = e.z;
  h.e3 = e.w;
  const uint32_t et0 = be_lo(e.y), et1 = be_lo(e.z);
  const uint32_t t1 = tag_type(et0), t2 = t1 & tag_type(et1);
  const uint32_t l3 = 14 + 4 * (t1 + t2);
  load64(h.W, p + l3);  // one trip after the tags are known (no speculative untagged read)
  if (et0 < 0x0600u) return false;
  if (len < l3 + 20u) return false;
  const uint32_t *W = h.W;
  const uint32_t ver = (W[0] >> 4) & 15u;
  const bool v4 = ver == 4u;
  const uint32_t dl = len - l3;
  const uint32_t length = v4 ? be_hi(W[0]) : be_lo(W[1]);
  uint32_t plen;
  if (v4) {
    if ((W[0] & 0x0Fu) != 5u || length < 20u) return false;
    plen = (dl > length ? length : dl) - 20u;
  } else {
    if (ver != 6u || dl < 40u) return false;
    plen = (length > dl - 40u) ? dl - 40u : length;
  }
  const uint32_t proto = v4 ? ((W[2] >> 8) & 0xFFu) : ((W[1] >> 16) & 0xFFu);
  const uint32_t g = proto == 6u ? 1u : (proto == 17u ? 2u : 0u);
  if (!g) return false;
  const uint32_t ty = v4 ? W[6] : W[11], tw = v4 ? W[8] : W[13];
  const uint32_t l4 = l3 + (v4 ? 20u : 40u);
  const uint32_t ulen = be_lo(ty);
  const uint32_t seg = (g == 2u && ulen >= 8u && ulen <= plen) ? ulen : plen;
  if (vxreg && g == 2u) {  // ports -> VXLAN (udp.go:108-110 NextLayerType by port)
    const uint32_t tx = v4 ? W[5] : W[10];
    const uint32_t rd = fix_bucket_at(kFixUdpBase, F.mult, be_hi(tx));
    const uint32_t rs = fix_bucket_at(kFixUdpBase, F.mult, be_lo(tx));
    if ((ports_next_raw(rd, rs, F.pl_raw) & 15u) == D_VXLAN) {
      h.ok = 2;
      return false;
    }
  }
  if (g == 1u) {  // the options walk of fast_decode, on the guess
    const uint32_t hl = ((tw >> 4) & 15u) * 4u;
    uint32_t ok = (plen >= 20u && hl >= 20u && hl <= plen) ? 1u : 0u;
    for (uint32_t q = 20; ok && !tcp_opts_quick(hl, v4 ? W[10] : W[15]) && q < hl;) {
      const uint32_t k = g_lds[p + l4 + q];
      if (k == 0) break;
      uint32_t ol = 1;
      if (k != 1) {
        if (hl - q < 2) { ok = 0; break; }
        ol = g_lds[p + l4 + q + 1];
        if (ol < 2 || ol > hl - q) { ok = 0; break; }
      }
      q += ol;
    }
    h.ok = ok;
  }
  h.pos = l4 | (seg << 16);
  l4_out = l4;
  seg_out = seg;
  return true;
}

// seg_pass (the per-window header-once step): hdr_parse, and the transport segment it guessed
// summed from this window: its head and tail here, the whole chunks between left to the
// window's chunk prefix sums (sg) when it is long and even-aligned.
template <bool COOP>
__device__ __forceinline__ void seg_pass(uint32_t p, uint32_t len, uint32_t buf, Hdr &h, Seg &sg,
                                         const FastCtx &F, bool vxreg) {
  uint32_t l4, seg;
  if (!hdr_parse(p, len, h, F, vxreg, l4, seg)) return;
  const uint32_t S = p + l4;
  if (COOP && seg >= 64u && !(S & 1u)) {
    // head [S, A) and tail [B, E) from their aligned chunks; [A, B) from the prefix sums
    const uint32_t E = S + seg, A = (S + 15u) & ~15u, B = E & ~15u;
    uint32_t s = 0;
    if (A > S) {
      const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + A - 16u);
      const uint32_t h8 = (S & 15u) * 8u;
      uint64_t lo = ((uint64_t)q.y << 32) | q.x, hi = ((uint64_t)q.w << 32) | q.z;
      lo = h8 >= 64u ? 0ull : (lo >> h8) << h8;
      hi = h8 > 64u ? (hi >> (h8 - 64u)) << (h8 - 64u) : hi;
      s = dot2((uint32_t)lo, 0x00010001u, s);
      s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
      s = dot2((uint32_t)hi, 0x00010001u, s);
      s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
    }
    if (E > B) {
      const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + B);
      const uint32_t r8 = (E & 15u) * 8u;
      uint64_t lo = ((uint64_t)q.y << 32) | q.x, hi = ((uint64_t)q.w << 32) | q.z;
      lo = r8 >= 64u ? lo : (lo << (64u - r8)) >> (64u - r8);
      hi = r8 > 64u ? (hi << (128u - r8)) >> (128u - r8) : 0ull;
      s = dot2((uint32_t)lo, 0x00010001u, s);
      s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
      s = dot2((uint32_t)hi, 0x00010001u, s);
      s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
    }
    sg = Seg{s, (A - buf) >> 4, (B - buf) >> 4};  // the caller adds P[b] - P[a] into h.sum
    return;
  }
  h.sum = seg_sum_chunks(S, seg, 0u);
}

// p: LDS address of the packet's first byte; len: its length.  CS / HASH: the fused
// checksums / flow hashes are requested (GPD_OPT_NO_CHECKSUMS / _NO_FLOW_HASH clear).
// Two dependent LDS round trips per pass (three for tagged frames): (1) the Ethernet header
// and the 64 bytes after it; (2) every table lookup — EtherType, protocol, ports, each on
// a guess read from the bytes (IPv4/IPv6 by the version nibble, TCP/UDP by the protocol
// number).  The lookups then confirm the guesses; a packet they contradict goes to the
// generic decoder.  Hashes and the IPv4 header checksum are computed from registers as
// each layer is accepted, so VXLAN's second pass overwrites them exactly as the reused
// layer objects are overwritten (A11); the transport checksum reads its segment's edge
// chunks once more after the parse.
// COOP: a long even-aligned segment's whole middle chunks are left to window_prefix (sg).
// HO: the header-once decode — no window is read: the header bytes and the segment sum come
// from seg_pass (*h), one pass (a VXLAN payload takes the generic decoder).
template <bool CS, bool HASH, bool COOP, bool HO = false, bool AL = false>
__device__ __forceinline__ bool fast_decode(uint32_t p, uint32_t len, const FastCtx &F, Out &o,
                                            uint32_t buf, Seg &sg, const Hdr *h = nullptr) {
  uint64_t codes = 0, nh = 0, th = 0;
  uint32_t nc = 0, trunc = 0, stop = 0;
  uint32_t net = 0, tp = 0, ip4 = 0, ipcs = 0;
  uint32_t tp_off = 0, tp_len = 0, tp_pl = 0;  // the last transport; its proto + length terms
  uint32_t tp_kind = 0, ps4 = 0, ps6 = 0;      // its network object kind; each kind's addresses
  uint32_t net_off = 0;                        // the last network header
  uint32_t b = 0, lim = len;                   // this pass's Ethernet offset; end of its data
  // AL (unshifted 8 KiB windows, frames of ~65..160 B): a VXLAN frame's inner Ethernet bytes
  // 8..23 come from the outer pass's registers when it is IPv4 (IHL 5) / UDP / VXLAN — one
  // misaligned LDS read fewer per pass (VXLAN -1.8 %; in the other kernels the longer live
  // range costs 1-5 %, measured A/B on one box)
  constexpr bool reg_e = !HO && AL;
  uint32_t ie1 = 0, ie2 = 0, ie3 = 0, have_ie = 0;
  auto put = [&](uint32_t code) { codes |= (uint64_t)code << (16 + 4 * nc); nc++; };
  for (int pass = 0; pass < (HO ? 1 : 2); pass++) {
    // ---- round trip 1: Ethernet header (ethernet.go:41-62) and the bytes after it
    if (lim < b + 15u) return false;  // too small, or an empty payload: generic path
    U128 e;  // bytes 8..23: EtherType and up to two tags
    uint32_t W[16];
    if (HO) {
      e.x = 0;
      e.y = h->e1;
      e.z = h->e2;
      e.w = h->e3;
#pragma unroll
      for (int k = 0; k < 16; k++) W[k] = h->W[k];
    } else if (reg_e && have_ie) {
      e.x = 0;
      e.y = ie1;
      e.z = ie2;
      e.w = ie3;
      load64(W, p + b + 14);
    } else {
      e = ld128(p + b + 8);
      load64(W, p + b + 14);
    }
    const uint32_t et0 = be_lo(e.y), et1 = be_lo(e.z), et2 = be_lo(e.w);
    if (et0 < 0x0600u) {  // 802.3 length framing
      // header-once tile decode only (the per-window kernels leave it to the generic decoder):
      // Ethernet's payload is Length bytes (ethernet.go:53-58), then LLC (llc.go:31-52) from the
      // staged bytes 14..16, then its next layer (llc.go:61-69) — which must stop the decode
      if (!HO || b != 0u) return false;
      const uint32_t re = fix_bucket<kFixEthBase>(F.mult, 0u);  // EthernetTypeLLC
      if ((re & 15u) != D_LLC) return false;
      uint32_t pl = lim - 14u;
      if (pl < et0) trunc = 1;
      else pl = et0;
      if (pl < 3u) return false;  // "LLC header too small": the generic decoder
      const uint32_t dsap = (e.y >> 16) & 0xFEu, ssap = (e.y >> 24) & 0xFEu, ctl = e.z & 0xFFu;
      uint32_t cl = 3;
      if (!(ctl & 1u) || (ctl & 3u) == 1u) {  // two-byte control field
        if (pl < 4u) return false;
        cl = 4;
      }
      put(GPD_C_ETHERNET);
      put((re >> 4) & 15u);
      if (pl == cl) break;  // layers_decoder.go:71-73
      const uint32_t nt = (dsap == 0xAAu && ssap == 0xAAu) ? (uint32_t)GPD_LT_SNAP
                        : (dsap == 0x42u && ssap == 0x42u) ? (uint32_t)GPD_LT_STP : (uint32_t)GPD_LT_ZERO;
      if ((reinterpret_cast<const uint8_t *>(g_lds)[nt] & 15u) != D_NONE) return false;
      stop = nt;
      break;
    }
    const uint32_t t1 = tag_type(et0), t2 = t1 & tag_type(et1);
    const uint32_t l3 = b + 14 + 4 * (t1 + t2);
    if (t1 && !HO) load64(W, p + l3);  // tagged: the network header is further in
    // ---- guesses from the bytes
    const uint32_t ver = (W[0] >> 4) & 15u;
    const bool v4 = ver == 4u;
    const uint32_t proto = v4 ? ((W[2] >> 8) & 0xFFu) : ((W[1] >> 16) & 0xFFu);
    const uint32_t g = proto == 6u ? 1u : (proto == 17u ? 2u : 0u);  // TCP / UDP
    const uint32_t tx = v4 ? W[5] : W[10], ty = v4 ? W[6] : W[11], tw = v4 ? W[8] : W[13];
    const uint32_t l4 = l3 + (v4 ? 20u : 40u);
    const uint32_t dl = lim - l3;
    const uint32_t length = v4 ? be_hi(W[0]) : be_lo(W[1]);  // IPv4 total / IPv6 payload
    uint32_t plen;                                             // the network payload
    if (v4) plen = (dl > length ? length : dl) - 20u;
    else plen = (length > dl - 40u) ? dl - 40u : length;
    const uint32_t ulen = be_lo(ty);
    const uint32_t seg = (g == 2u && ulen >= 8u && ulen <= plen) ? ulen : plen;
    // ---- round trip 2: all lookups
    const uint32_t r0 = fix_bucket<kFixEthBase>(F.mult, et0);
    uint32_t r1 = 0, r2 = 0;
    if (t1) {
      r1 = fix_bucket<kFixEthBase>(F.mult, et1);
      r2 = fix_bucket<kFixEthBase>(F.mult, et2);
    }
    // the network layer's next: the protocol table, or Fragment when an IPv4 header has MF or a
    // fragment offset (ip4.go:281-286) — LayerType | LUT entry << 16 either way
    const uint32_t pv = (v4 && (be_hi(W[1]) & 0x3FFFu)) ? (uint32_t)GPD_LT_FRAGMENT | (F.fr_ent << 16)
                                                      : lds_u32(4 * (kHashLutWords + proto));
    const uint32_t pbase = g == 1u ? kFixTcpBase : kFixUdpBase;
    const uint32_t rd = fix_bucket_at(pbase, F.mult, be_hi(tx));
    const uint32_t rs = fix_bucket_at(pbase, F.mult, be_lo(tx));
    // ---- Ethernet / Dot1Q (dot1q.go:29-50), confirming the tag guesses
    put(GPD_C_ETHERNET);
    if (((r0 & 15u) == D_DOT1Q) != (t1 != 0)) return false;
    uint32_t r = r0;
    if (t1) {
      if (lim <= b + 18u) return false;
      put(GPD_C_DOT1Q);
      if (((r1 & 15u) == D_DOT1Q) != (t2 != 0)) return false;
      r = r1;
      if (t2) {
        if (lim <= b + 22u || (r2 & 15u) == D_DOT1Q) return false;
        put(GPD_C_DOT1Q);
        r = r2;
      }
    }
    const uint32_t dec = r & 15u;
    if (dec == D_NONE) { stop = (r >> 8) & 0xFFu; break; }
    uint32_t ps;  // pseudo-header address words of this network layer (LE domain)
    if (dec == D_IP4) {  // ip4.go:188-286, IHL 5 only
      // IHL != 5 (options), Length 0 (TSO rule) or < 20 (error): generic path
      if (!v4 || dl < 20u || (W[0] & 0x0Fu) != 5u || length < 20u) return false;
      if (dl < length) trunc = 1;
      ps = dot2(W[4], 0x00010001u, dot2(W[3], 0x00010001u, 0u));
      if (CS) {  // checksum(ip4.Contents), ip4.go:158-179 (bytes 10-11 left out)
        ipcs = fold_le_not(dot2(W[2], 0x00000001u, dot2(W[1], 0x00010001u,
                           dot2(W[0], 0x00010001u, ps))));
        ip4 = 1;
      }
      if (HASH) nh = flow_fast(fnv_start<4>(W[3]), fnv_start<4>(W[4]), 1u);  // ip4.go:63-65
      ps4 = ps;
      net = 1;
      net_off = l3;
      put(GPD_C_IPV4);
      lim = l3 + 20u + plen;  // Length trims the payload (and Ethernet padding)
    } else if (dec == D_IP6) {  // ip6.go:221-278 without hop-by-hop
      if (ver != 6u || dl < 40u || proto == 0u || length == 0u) return false;
      if (length > dl - 40u) trunc = 1;
      ps = 0;
#pragma unroll
      for (int k = 2; k < 10; k++) ps = dot2(W[k], 0x00010001u, ps);  // tcpip.go:37-48
      if (HASH) {  // ip6.go:49-51
        const H64 hs = fnv_more(fnv_more(fnv_more(fnv_start<4>(W[2]), W[3]), W[4]), W[5]);
        const H64 hd = fnv_more(fnv_more(fnv_more(fnv_start<4>(W[6]), W[7]), W[8]), W[9]);
        nh = flow_fast(hs, hd, 2u);
      }
      ps6 = ps;
      net = 2;
      net_off = l3;
      put(GPD_C_IPV6);
      lim = l3 + 40u + plen;
    } else {
      return false;
    }
    if (plen == 0) break;
    // ---- transport, confirming the protocol guess
    const uint32_t d4 = (pv >> 16) & 15u;
    if (d4 == D_NONE) { stop = pv & 0xFFFFu; break; }
    // ICMPv4 (icmp4.go:220-231, next layer Payload :261-263) and gopacket.Fragment (base.go:108-117:
    // all of the rest, nothing after) share one exit: a separate Fragment exit made the compiler
    // add ~110 register moves to the loop (tools/isa_count.py)
    if (d4 == D_ICMP4 || d4 == D_FRAG) {
      const bool ic = d4 == D_ICMP4;
      if (ic && plen < 8u) return false;  // "ICMP layer less then 8 bytes": generic path
      put(ic ? GPD_C_ICMPV4 : GPD_C_FRAGMENT);
      if (!ic || plen == 8u) break;
      if ((F.pl_raw & 15u) == D_PAYLOAD) put(GPD_C_PAYLOAD);
      else stop = GPD_LT_PAYLOAD;
      break;
    }
    if (!((d4 == D_TCP && g == 1u) || (d4 == D_UDP && g == 2u))) return false;
    uint32_t hl;
    if (g == 1u) {  // tcp.go:229-314
      hl = ((tw >> 4) & 15u) * 4u;
      if (plen < 20u || hl < 20u || hl > plen) return false;
      if (HO && !h->ok) return false;
      // OPTIONS, tcp.go:274-300 (errors -> generic path)
      for (uint32_t q = 20; !HO && !tcp_opts_quick(hl, v4 ? W[10] : W[15]) && q < hl;) {
        const uint32_t k = g_lds[p + l4 + q];
        if (k == 0) break;
        uint32_t ol = 1;
        if (k != 1) {
          if (hl - q < 2) return false;
          ol = g_lds[p + l4 + q + 1];
          if (ol < 2 || ol > hl - q) return false;
        }
        q += ol;
      }
      put(GPD_C_TCP);
    } else {  // UDP, udp.go:30-56 (Length 0: the rest; 1..7: error)
      if (plen < 8u || (ulen != 0u && ulen < 8u)) return false;
      if (ulen > plen) trunc = 1;
      hl = 8;
      lim = l4 + seg;
      put(GPD_C_UDP);
    }
    tp = g;
    if (HASH) th = flow_fast(fnv_start<2>(tx), fnv_start<2>(tx >> 16), g == 1u ? 4u : 5u);
    // pseudo-header protocol and length as LE-domain words (seg < 2^16 in a window); the
    // addresses are added at the end from the network object of this kind as the call
    // leaves it (SetNetworkLayerForChecksum(&ip4) reads the reused object: for VXLAN whose
    // inner pass stops before a transport, the inner header's addresses)
    tp_pl = (g == 1u ? 0x0600u : 0x1100u) + __builtin_amdgcn_perm(0u, seg, 0x0C0C0001u);
    tp_kind = net;
    tp_off = l4;
    tp_len = seg;
    const uint32_t pl4 = seg - hl;
    if (pl4 == 0) break;
    const uint32_t next = ports_next_raw(rd, rs, F.pl_raw), nd = next & 15u;
    if (nd == D_NONE) { stop = (next >> 8) & 0xFFu; break; }
    if (nd == D_PAYLOAD) { put(GPD_C_PAYLOAD); break; }  // Payload consumes the rest
    if (HO || nd != D_VXLAN || pass == 1 || pl4 < 8u) return false;
    put(GPD_C_VXLAN);  // vxlan.go:53-78; its payload is an Ethernet frame (A11: two passes)
    b = l4 + hl + 8;
    if (pl4 == 8u) break;
    if (reg_e) {  // IPv4 (IHL 5) / UDP / VXLAN: the inner bytes 8..23 are W[11..14]
      have_ie = (v4 && g == 2u) ? 1u : 0u;
      ie1 = W[12];
      ie2 = W[13];
      ie3 = W[14];
    }
  }

  // ---- outputs, composed exactly as decode_packet does
  const uint32_t tp_ps = tp_pl + (tp_kind == 1u ? ps4 : ps6);
  uint32_t st = (stop ? F.unsup : GPD_ST_OK) | (trunc << 2) | (nc << 4);
  uint32_t cs = 0;
  st |= (net << 20) | (tp ? (tp == 1 ? 4u : 5u) << 24 : 0u);  // endpoint types (gpd.h)
  if (HASH) st |= (net ? 1u << 16 : 0u) | (tp ? 1u << 17 : 0u);
  sg.b = 0;
  if (HO) {
    if (CS) {  // the segment seg_pass summed must be this transport's
      if (tp && h->pos != (tp_off | (tp_len << 16))) return false;
      cs = (ip4 ? ipcs : 0u) | (tp ? fold_le_not(tp_ps + h->sum) << 16 : 0u);
      st |= (ip4 ? 1u << 18 : 0u) | (tp ? 1u << 19 : 0u);
    }
  } else if (COOP && CS && tp && tp_len >= 64u && !((p + tp_off) & 1u)) {
    // head [S, A) and tail [B, E) from their aligned chunks; [A, B) from the prefix sums
    const uint32_t S = p + tp_off, E = S + tp_len, A = (S + 15u) & ~15u, B = E & ~15u;
    uint32_t s = tp_ps;
    if (A > S) {  // keep bytes from S & 15 on
      const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + A - 16u);
      const uint32_t h8 = (S & 15u) * 8u;
      uint64_t lo = ((uint64_t)q.y << 32) | q.x, hi = ((uint64_t)q.w << 32) | q.z;
      lo = h8 >= 64u ? 0ull : (lo >> h8) << h8;
      hi = h8 > 64u ? (hi >> (h8 - 64u)) << (h8 - 64u) : hi;
      s = dot2((uint32_t)lo, 0x00010001u, s);
      s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
      s = dot2((uint32_t)hi, 0x00010001u, s);
      s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
    }
    if (E > B) {  // keep bytes below E & 15
      const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + B);
      const uint32_t r8 = (E & 15u) * 8u;
      uint64_t lo = ((uint64_t)q.y << 32) | q.x, hi = ((uint64_t)q.w << 32) | q.z;
      lo = r8 >= 64u ? lo : (lo << (64u - r8)) >> (64u - r8);
      hi = r8 > 64u ? (hi << (128u - r8)) >> (128u - r8) : 0ull;
      s = dot2((uint32_t)lo, 0x00010001u, s);
      s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
      s = dot2((uint32_t)hi, 0x00010001u, s);
      s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
    }
    sg = Seg{s, (A - buf) >> 4, (B - buf) >> 4};
    o.status = st | (ip4 ? 1u << 18 : 0u) | (1u << 19);
    o.layers = codes | (stop & 0xFFFFu);
    o.net_hash = HASH ? nh : 0;
    o.tp_hash = HASH ? th : 0;
    o.csum = ip4 ? ipcs : 0u;  // the transport half is added by the caller
    o.hoff = hdr_word(net != 0, net_off, tp != 0, tp_off);
    return true;
  } else if (AL && CS && tp && !((p + tp_off) & 1u)) {
    // AL (unshifted 8 KiB windows, VXLAN-sized frames): the same sum from aligned 16-byte
    // chunks, head [S, A) and tail [B, E) masked and the whole chunks between as they are — an
    // aligned DS read costs ~1/3.6 of a misaligned one (VXLAN -3.4 %; with shifted copies of
    // small frames the header reads are aligned already and the masking cost pcap64 +1 %,
    // measured A/B on one box)
    const uint32_t S = p + tp_off, E = S + tp_len, A = (S + 15u) & ~15u, B = E & ~15u;
    uint32_t s = tp_ps;
    if (A > S) {
      const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + A - 16u);
      const uint32_t h8 = (S & 15u) * 8u;
      const uint32_t e8 = E < A ? (A - E) * 8u : 0u;  // a segment ending inside its head chunk
      uint64_t lo = ((uint64_t)q.y << 32) | q.x, hi = ((uint64_t)q.w << 32) | q.z;
      lo = h8 >= 64u ? 0ull : (lo >> h8) << h8;
      hi = h8 > 64u ? (hi >> (h8 - 64u)) << (h8 - 64u) : hi;
      if (e8) {  // drop the e8 top bits of (hi, lo)
        hi = e8 >= 64u ? 0ull : (hi << e8) >> e8;
        lo = e8 > 64u ? (lo << (e8 - 64u)) >> (e8 - 64u) : lo;
      }
      s = dot2((uint32_t)lo, 0x00010001u, s);
      s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
      s = dot2((uint32_t)hi, 0x00010001u, s);
      s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
    }
    for (uint32_t x = A; x < B; x += 16u) {
      const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + x);
      s = dot2(q.x, 0x00010001u, s);
      s = dot2(q.y, 0x00010001u, s);
      s = dot2(q.z, 0x00010001u, s);
      s = dot2(q.w, 0x00010001u, s);
    }
    if (E > B && B >= A) {
      const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + B);
      const uint32_t r8 = (E & 15u) * 8u;
      uint64_t lo = ((uint64_t)q.y << 32) | q.x, hi = ((uint64_t)q.w << 32) | q.z;
      lo = r8 >= 64u ? lo : (lo << (64u - r8)) >> (64u - r8);
      hi = r8 > 64u ? (hi << (128u - r8)) >> (128u - r8) : 0ull;
      s = dot2((uint32_t)lo, 0x00010001u, s);
      s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
      s = dot2((uint32_t)hi, 0x00010001u, s);
      s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
    }
    cs = (ip4 ? ipcs : 0u) | (fold_le_not(s) << 16);
    st |= (ip4 ? 1u << 18 : 0u) | (1u << 19);
  } else if (CS) {
    // TCP.ComputeChecksum(), tcp.go:193-195 / tcpip.go:52-88 over the last transport.  Its
    // first and ragged-last 16-byte chunks are read here, once, after the parse (holding
    // them through the parse would cost 16 VGPRs, a wave per SIMD).
    const U128 c0 = ld128(p + tp_off), ct = ld128(p + tp_off + (tp_len & ~15u));
    uint32_t s = tp_ps;
    const uint32_t w0 = tp_len >= 16u ? 0x00010001u : 0u;  // first whole chunk
    s = dot2(c0.x, w0, s);
    s = dot2(c0.y, w0, s);
    s = dot2(c0.z, w0, s);
    s = dot2(c0.w, w0, s);
    // ragged tail: the first tp_len % 16 bytes of ct (an odd last byte is the low byte of
    // its half)
    const uint32_t r8 = (tp_len & 15u) * 8u;
    uint64_t lo = ((uint64_t)ct.y << 32) | ct.x, hi = ((uint64_t)ct.w << 32) | ct.z;
    lo = r8 >= 64u ? lo : (r8 ? (lo << (64u - r8)) >> (64u - r8) : 0ull);
    hi = r8 > 64u ? (hi << (128u - r8)) >> (128u - r8) : 0ull;
    s = dot2((uint32_t)lo, 0x00010001u, s);
    s = dot2((uint32_t)(lo >> 32), 0x00010001u, s);
    s = dot2((uint32_t)hi, 0x00010001u, s);
    s = dot2((uint32_t)(hi >> 32), 0x00010001u, s);
    const uint32_t xt = tp_len & ~15u;
    for (uint32_t x = 16; x < xt; x += 16u) {  // whole chunks after the first (long segments)
      const U128 q = ld128(p + tp_off + x);
      s = dot2(q.x, 0x00010001u, s);
      s = dot2(q.y, 0x00010001u, s);
      s = dot2(q.z, 0x00010001u, s);
      s = dot2(q.w, 0x00010001u, s);
    }
    cs = (ip4 ? ipcs : 0u) | (tp ? fold_le_not(s) << 16 : 0u);
    st |= (ip4 ? 1u << 18 : 0u) | (tp ? 1u << 19 : 0u);
  }
  o.status = st;
  o.layers = codes | (stop & 0xFFFFu);
  o.net_hash = HASH ? nh : 0;
  o.tp_hash = HASH ? th : 0;
  o.csum = cs;
  o.hoff = hdr_word(net != 0, net_off, tp != 0, tp_off);
  return true;
}

// Copy a register-staged window into LDS shifted up by s = 16 - 4Q - r bytes (0 < s < 16),
// with aligned ds_write_b128 only: LDS chunk m holds bytes [16m - s, 16m - s + 16) of the
// window, i.e. bytes [16 - s, 32 - s) of (chunk m-1 | chunk m).  Chunk m-1 of lane l is lane
// l-1's chunk (DPP wave_shr:1), lane 0 takes lane 63's of the previous 1-KiB row; one extra
// chunk past the window's end takes the last row's tail.
template <int Q, int NC, bool SUMS, typename V>
__device__ __forceinline__ void commit_shifted(const V (&wv)[NC], uint32_t buf, uint32_t lane, uint32_t r,
                                               uint32_t (&cs)[NC]) {
  uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;  // lane 63's chunk of the previous row
#pragma unroll
  for (int j = 0; j <= NC; j++) {
    uint32_t D[8];
    if (j < NC) {
      D[4] = wv[j].x; D[5] = wv[j].y; D[6] = wv[j].z; D[7] = wv[j].w;
    } else {
      D[4] = D[5] = D[6] = D[7] = 0u;
    }
    D[0] = (uint32_t)__builtin_amdgcn_update_dpp((int)b0, (int)D[4], 0x138, 0xF, 0xF, false);
    D[1] = (uint32_t)__builtin_amdgcn_update_dpp((int)b1, (int)D[5], 0x138, 0xF, 0xF, false);
    D[2] = (uint32_t)__builtin_amdgcn_update_dpp((int)b2, (int)D[6], 0x138, 0xF, 0xF, false);
    D[3] = (uint32_t)__builtin_amdgcn_update_dpp((int)b3, (int)D[7], 0x138, 0xF, 0xF, false);
    V out;
    out.x = __builtin_amdgcn_alignbyte(D[Q + 1], D[Q], r);
    out.y = __builtin_amdgcn_alignbyte(D[Q + 2], D[Q + 1], r);
    out.z = __builtin_amdgcn_alignbyte(D[Q + 3], D[Q + 2], r);
    out.w = __builtin_amdgcn_alignbyte(D[Q + 4], D[Q + 3], r);
    if (j < NC || lane == 0u) *reinterpret_cast<V *>(g_lds + buf + 1024u * j + 16u * lane) = out;
    if (SUMS && j < NC)
      cs[j] = dot2(out.w, 0x00010001u, dot2(out.z, 0x00010001u, dot2(out.y, 0x00010001u, dot2(out.x, 0x00010001u, 0u))));
    if (j < NC) {
      b0 = (uint32_t)__builtin_amdgcn_readlane((int)D[4], 63);
      b1 = (uint32_t)__builtin_amdgcn_readlane((int)D[5], 63);
      b2 = (uint32_t)__builtin_amdgcn_readlane((int)D[6], 63);
      b3 = (uint32_t)__builtin_amdgcn_readlane((int)D[7], 63);
    }
  }
}

// P[c] (see window_prefix) from the LE-domain sums of the chunks as committed: LDS chunk
// 64 j + l is row j of lane l, so each row is one wave prefix scan on top of the rows below.
template <int NC>
__device__ __forceinline__ void rows_prefix(const uint32_t (&cs)[NC], uint32_t pfx, uint32_t lane) {
  uint32_t base = 0;
#pragma unroll
  for (int j = 0; j < NC; j++) {
    const uint32_t incl = wave_incl_scan(cs[j]);
    *reinterpret_cast<uint32_t *>(g_lds + pfx + 4u * (64u * j + lane)) = base + incl - cs[j];
    base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
  if (lane == 0u) *reinterpret_cast<uint32_t *>(g_lds + pfx + 4u * 64u * NC) = base;
}

// LE-domain sum s + bytes [lo, hi) of the aligned 16-byte LDS chunk at a (0 <= lo <= hi <= 16).
__device__ __forceinline__ uint32_t chunk_part(uint32_t a, uint32_t lo, uint32_t hi, uint32_t s) {
  const uint4 q = *reinterpret_cast<const uint4 *>(g_lds + a);
  const uint32_t l8 = lo * 8u, h8 = hi * 8u;
  const uint64_t keep_lo = (l8 >= 64u ? 0ull : ~0ull << l8) & (h8 >= 64u ? ~0ull : (1ull << h8) - 1ull);
  const uint64_t keep_hi = (l8 >= 64u ? ~0ull << (l8 - 64u) : ~0ull) &
                           (h8 <= 64u ? 0ull : (h8 >= 128u ? ~0ull : (1ull << (h8 - 64u)) - 1ull));
  const uint64_t x = ((((uint64_t)q.y << 32) | q.x) & keep_lo), y = ((((uint64_t)q.w << 32) | q.z) & keep_hi);
  s = dot2((uint32_t)x, 0x00010001u, s);
  s = dot2((uint32_t)(x >> 32), 0x00010001u, s);
  s = dot2((uint32_t)y, 0x00010001u, s);
  return dot2((uint32_t)(y >> 32), 0x00010001u, s);
}

// A lane's view of the tile descriptors (rs_kernel, ro_kernel): plain register loads, issued two
// tiles ahead, and the clamp to the batch buffer where they are used.  The members are references
// to the kernel's own locals, as a lambda's captures would be: with copies, or as free functions,
// the kernels' register allocation moves (tools/isa_diff.py).
struct TileDesc {
  const KParams &P;
  const uint32_t &lane, &n, &ntiles, &dlen;
  __device__ __forceinline__ void load(uint32_t u, uint32_t &o, uint32_t &c) const {  // descriptors of tile u
    const uint32_t i = u * 64u + lane;
    o = c = 0;
    if (u < ntiles && i < n) {
      o = __builtin_nontemporal_load(P.offset + i);
      c = __builtin_nontemporal_load(P.caplen + i);
    }
  }
  __device__ __forceinline__ uint32_t read(uint32_t u, uint32_t o_raw, uint32_t c_raw, uint32_t &off,
                                           uint32_t &end) const {
    const uint32_t v = u * 64u + lane < n ? 1u : 0u;
    const uint32_t o = v ? min(o_raw, dlen) : 0u;
    const uint32_t l = v ? min(c_raw, dlen - o) : 0u;
    off = o;  // a packet reaching past data_len is clamped to the buffer
    end = o + l;
    return v;
  }
};

}  // namespace gpd
