// gpd_dev_common.h — what every decode kernel's translation unit shares (device code, all
// header-inline): the option / diagnostic bits, the LDS arena, the byte sources the decoders read
// packets through, the wave reductions, checksum folds and FNV hashes, the result record and its
// store, and the window planning and LDS-DMA primitives.
//
// One wavefront lane per packet; a wave owns tiles of 64 consecutive packet indices.  The decode
// loop, the IPv4 header checksum, the TCP/UDP pseudo-header checksum and both flow FastHashes are
// fused, so packet bytes leave HBM exactly once.  Semantics follow the reference (paths relative
// to google/gopacket):
//   loop ............ layers_decoder.go:60-79, parser.go:302-316
//   Ethernet ........ layers/ethernet.go:41-62,110-112
//   Dot1Q ........... layers/dot1q.go:29-50
//   IPv4 ............ layers/ip4.go:188-286
//   IPv6 (+HBH) ..... layers/ip6.go:54-76,221-291,327-346,418-432,509-526
//   ExtSkipper ...... layers/ip6.go:443-461
//   TCP ............. layers/tcp.go:229-314
//   UDP ............. layers/udp.go:30-110
//   VXLAN ........... layers/vxlan.go:48-78
//   Payload/Fragment  base.go:55-63,108-117
//   checksums ....... layers/ip4.go:158-179, layers/tcpip.go:26-88, layers/tcp.go:193-195
//   FastHash ........ flows.go:60-83,167-174
// DESIGN.md §Semantics defines every output word.
#pragma once
#include <hip/hip_runtime.h>

#include "gpd_internal.h"

namespace gpd {

// The two diagnostic bits (bench --ablate nodecode / nowait) exist only in the diagnostic
// library (libgpd_diag.so, built with -DGPD_DIAG): there the runtime accepts them; in the
// shipped libgpd.so they are refused by gpd_ctx_set_options / gpd_ctx_create and every branch
// that reads them compiles away (kDiagBuild false => both constants 0).
#ifdef GPD_DIAG
constexpr bool kDiagBuild = true;
#else
constexpr bool kDiagBuild = false;
#endif
constexpr uint32_t kDiagSkipDecodeBit = 1u << 31, kDiagNoWaitBit = 1u << 30;
constexpr uint32_t kDiagSkipDecode = kDiagBuild ? kDiagSkipDecodeBit : 0u;  // stream only, no decode
constexpr uint32_t kDiagNoWait = kDiagBuild ? kDiagNoWaitBit : 0u;          // skip the per-tile DMA wait
constexpr uint32_t kDiagNtLoad = 1u << 29;      // A/B: window LDS-DMA with the nt cache policy
constexpr uint32_t kDiagNtStore = 1u << 28;     // A/B: result stores with the nt cache policy
constexpr uint32_t kShiftWindows = 1u << 27;    // internal: register-staged windows copied shifted
constexpr uint32_t kRegPrefix = 1u << 26;       // internal: 8 KiB windows of long frames (IMIX)
constexpr uint32_t kHeaderOnce = 1u << 25;      // internal: 8 KiB windows decoded once per tile (seg_pass)
constexpr uint32_t kRounds = 1u << 24;          // internal: header-once over 8 KiB rounds (ro_kernel)
constexpr uint32_t kDiagMask = kDiagSkipDecodeBit | kDiagNoWaitBit | kDiagNtLoad | kDiagNtStore | kShiftWindows |
                               kRegPrefix | kHeaderOnce | kRounds;
// A/B builds only (GPD_EXTRA_CFLAGS=-DGPD_EXP=..., tools/ab_exp.sh): a fast-path variant under
// test reads kExp inside an `#if GPD_EXP` block; the shipped library has none.
#ifndef GPD_EXP
#define GPD_EXP 0
#endif
[[maybe_unused]] constexpr uint32_t kExp = GPD_EXP;

// The LDS arena: the dispatch-table image first (LUT, ipproto, hashes), then the kernel's windows.
// Every kernel stages the image with its own copy of the same three-line loop: through a shared
// helper (thread count as an argument or a template parameter, P by reference or its fields by
// value) the compiler flips the loop's compare and branch, and the kernels are kept
// instruction-identical until a GPU measurement says otherwise (tools/isa_diff.py).
extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));

#ifdef GPD_PHASE_TIMING
// Diagnostic build only (libgpd_phase.so): per-phase shader-clock totals of the fast kernel's
// loop, summed over waves into g_phase (defined beside rs_kernel, the kernel that carries the
// marks); read back with gpd_diag_phase().
#define PH_DECL uint64_t ph_t = __builtin_amdgcn_s_memtime(), ph_acc[6] = {0, 0, 0, 0, 0, 0};
#define PH_MARK(k)                                      \
  do {                                                  \
    const uint64_t ph_n = __builtin_amdgcn_s_memtime(); \
    ph_acc[k] += ph_n - ph_t;                           \
    ph_t = ph_n;                                        \
  } while (0)
#define PH_FLUSH                                                              \
  do {                                                                        \
    if (lane == 0)                                                            \
      for (int k = 0; k < 6; k++) atomicAdd(&g_phase[k], (unsigned long long)ph_acc[k]); \
  } while (0)
#else
#define PH_DECL
#define PH_MARK(k) do {} while (0)
#define PH_FLUSH do {} while (0)
#endif

__device__ __forceinline__ uint32_t lds_u32(uint32_t a) {
  return *reinterpret_cast<const uint32_t *>(g_lds + a);
}

// ---------------------------------------------------------------- byte sources
// Logical window byte x -> physical LDS byte (slot rotation inside 256-byte blocks): 16-byte
// slot g of a rotated window is stored at slot (g & ~15) | ((g + (g >> 4)) & 15), so lanes walking
// packets at a power-of-two stride (64 B, 128 B...) spread over the LDS banks instead of piling
// on two.
__device__ __forceinline__ uint32_t swz_slot(uint32_t g) { return (g & ~15u) | ((g + (g >> 4)) & 15u); }

// SWZ: the window's 16-byte slots are rotated (decode_kernel's LDS-DMA windows); otherwise linear.
template <bool SWZ>
struct LdsSrc {
  uint32_t buf;  // LDS byte address of the window
  uint32_t pos;  // logical offset of the packet's first byte in the window
  __device__ __forceinline__ uint32_t abs(uint32_t rel) const { return pos + rel; }
  __device__ __forceinline__ uint32_t phys(uint32_t x) const {
    return SWZ ? buf + (swz_slot(x >> 4) << 4) + (x & 15u) : buf + x;
  }
  __device__ __forceinline__ uint32_t dw(uint32_t x) const { return lds_u32(phys(x)); }  // x 4-aligned
  __device__ __forceinline__ uint32_t u8(uint32_t rel) const { return g_lds[phys(pos + rel)]; }
  __device__ __forceinline__ uint4 q(uint32_t x) const {  // x 16-aligned
    return *reinterpret_cast<const uint4 *>(g_lds + phys(x));
  }
};

// Global memory: byte offsets into the batch buffer (16-aligned base pointer).
struct GlbSrc {
  const uint8_t *data;
  uint64_t pos;  // offset of the packet's first byte
  __device__ __forceinline__ uint64_t abs(uint32_t rel) const { return pos + rel; }
  __device__ __forceinline__ uint32_t dw(uint64_t a) const {
    return *reinterpret_cast<const uint32_t *>(data + a);
  }
  __device__ __forceinline__ uint32_t u8(uint32_t rel) const { return data[pos + rel]; }
  __device__ __forceinline__ uint4 q(uint64_t a) const {
    return *reinterpret_cast<const uint4 *>(data + a);
  }
};

// A fallback packet whose first K bytes (from its 16-aligned global start) a lane staged in
// its own LDS slot: reads below that bound come from LDS, the rest (long segments' checksums)
// from global memory.  The generic decoder's chain of dependent header reads then costs LDS
// latency instead of HBM latency (rs_kernel's end-of-wave fallback lists).
template <uint32_t K>
struct HybSrc {
  const uint8_t *data;
  uint64_t pos;    // global offset of the packet's first byte
  uint64_t gbase;  // pos & ~15: global offset of slot byte 0
  uint32_t slot;   // LDS address of the lane's slot
  __device__ __forceinline__ uint64_t abs(uint32_t rel) const { return pos + rel; }
  __device__ __forceinline__ uint32_t dw(uint64_t a) const {
    return a - gbase < K ? lds_u32(slot + (uint32_t)(a - gbase)) : *reinterpret_cast<const uint32_t *>(data + a);
  }
  __device__ __forceinline__ uint32_t u8(uint32_t rel) const {
    const uint64_t a = pos + rel;
    return a - gbase < K ? (uint32_t)g_lds[slot + (uint32_t)(a - gbase)] : (uint32_t)data[a];
  }
  __device__ __forceinline__ uint4 q(uint64_t a) const {
    return a - gbase < K ? *reinterpret_cast<const uint4 *>(g_lds + slot + (uint32_t)(a - gbase))
                         : *reinterpret_cast<const uint4 *>(data + a);
  }
};

// N little-endian words holding packet bytes [rel, rel+4N) (unaligned start).
template <int N, class S>
__device__ __forceinline__ void load_words(const S &s, uint32_t rel, uint32_t (&w)[N]) {
  auto A = s.abs(rel);
  auto Al = A & ~decltype(A)(3);
  uint32_t sh = (uint32_t)(A & 3);
  uint32_t a[N + 1];
#pragma unroll
  for (int k = 0; k <= N; k++) a[k] = s.dw(Al + 4 * k);
#pragma unroll
  for (int k = 0; k < N; k++) w[k] = __builtin_amdgcn_alignbyte(a[k + 1], a[k], sh);
}

template <int N>
__device__ __forceinline__ uint32_t byte_at(const uint32_t (&w)[N], int o) {
  return (w[o >> 2] >> (8 * (o & 3))) & 0xFFu;
}
template <int N>
__device__ __forceinline__ uint32_t be16_at(const uint32_t (&w)[N], int o) {
  return (byte_at(w, o) << 8) | byte_at(w, o + 1);
}

// ---------------------------------------------------------------- checksums / hashes
// Exact (mod 2^32) sum of the big-endian 16-bit words of packet bytes [rel, rel+len)
// as tcpipChecksum accumulates them (tcpip.go:57-65; an odd last byte counts <<8):
// S = 256*E + O with E/O the byte sums at even/odd positions of the range, taken
// with v_dot4_u32_u8 against 0/1 byte weights that also carry the edge masks.
template <class S>
__device__ __forceinline__ uint32_t be16_sum(const S &s, uint32_t rel, uint32_t len) {
  auto A = s.abs(rel);
  const auto end = A + len;
  const uint32_t ew = (A & 1) ? 0x01000100u : 0x00010001u;
  const uint32_t ow = ew ^ 0x01010101u;
  uint32_t E = 0, O = 0;
  for (auto C = A & ~decltype(A)(15); C < end; C += 16) {
    const uint4 v = s.q(C);
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
    const uint32_t lo = A > C ? (uint32_t)(A - C) : 0u;
    const uint32_t hi = end - C < 16 ? (uint32_t)(end - C) : 16u;
    const uint32_t m16 = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t bm = (((m16 >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u;
      E = __builtin_amdgcn_udot4(x[j], ew & bm, E, false);
      O = __builtin_amdgcn_udot4(x[j], ow & bm, O, false);
    }
  }
  return (E << 8) + O;
}

__device__ __forceinline__ uint16_t fold_not(uint32_t csum) {
  while (csum > 0xFFFFu) csum = (csum >> 16) + (csum & 0xFFFFu);
  return (uint16_t)~csum;
}

constexpr uint64_t kFnvBasis = 14695981039346656037ULL;  // flows.go:69
constexpr uint64_t kFnvPrime = 1099511628211ULL;         // flows.go:70

// FNV-1a (flows.go:60-67) with fnvPrime = 2^40 + 0x1b3: h * prime = h * 0x1b3 + (h << 40), the
// 64-bit state as two words (one 32x32->64 multiply per byte).
struct H64 {
  uint32_t lo, hi;
};
__device__ __forceinline__ H64 fnv_mulp(H64 h) {
  const uint64_t p = (uint64_t)h.lo * 0x1b3u;
  return H64{(uint32_t)p, h.hi * 0x1b3u + (uint32_t)(p >> 32) + (h.lo << 8)};
}
constexpr uint64_t kFnvC0 = (kFnvBasis & ~0xFFull) * kFnvPrime;  // (basis with byte 0 cleared) * prime
// fnvHash of the NB low bytes of w (byte 0 first), from the basis
template <int NB>
__device__ __forceinline__ H64 fnv_start(uint32_t w) {
  static_assert(NB == 2 || NB == 4, "fnv_start<2|4>");
  // byte 0 in closed form: (basis ^ b) * prime = C0 + c * 0x1b3 + (c << 40), c = b ^ 0x25
  const uint32_t c = (w & 0xFFu) ^ (uint32_t)(kFnvBasis & 0xFFu);
  const uint64_t r = (uint64_t)c * 0x1b3u + kFnvC0;
  H64 x{(uint32_t)r, (uint32_t)(r >> 32) + (c << 8)};
#pragma unroll
  for (int j = 1; j < NB; j++) {
    x.lo ^= (w >> (8 * j)) & 0xFFu;
    x = fnv_mulp(x);
  }
  return x;
}
__device__ __forceinline__ H64 fnv_more(H64 x, uint32_t w) {  // four more bytes
#pragma unroll
  for (int j = 0; j < 4; j++) {
    x.lo ^= (w >> (8 * j)) & 0xFFu;
    x = fnv_mulp(x);
  }
  return x;
}
// Flow.FastHash, flows.go:167-174
__device__ __forceinline__ uint64_t flow_fast(H64 s, H64 d, uint32_t ept) {
  const uint64_t sum = (((uint64_t)s.hi << 32) | s.lo) + (((uint64_t)d.hi << 32) | d.lo);
  const H64 x = fnv_mulp(H64{(uint32_t)sum ^ ept, (uint32_t)(sum >> 32)});
  return ((uint64_t)x.hi << 32) | x.lo;
}

// ---------------------------------------------------------------- one packet
struct Out {
  uint32_t status;
  uint64_t layers;
  uint64_t net_hash, tp_hash;
  uint32_t csum;
  uint32_t hoff;  // gpd.h header offsets word
};

__device__ __forceinline__ uint32_t hdr_word(bool net, uint32_t net_off, bool tp, uint32_t tp_off) {
  return (net ? min(net_off, 0xFFFFu) : 0xFFFFu) | ((tp ? min(tp_off, 0xFFFFu) : 0xFFFFu) << 16);
}

// v_dot2_u32_u16: acc + the two 16-bit halves of x weighted by those of w (the fast decoders sum
// checksums in the little-endian domain with it: one op per 4 bytes, no byte shuffles).
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t dot2(uint32_t x, uint32_t w, uint32_t acc) {
  return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, x), __builtin_bit_cast(u16x2, w), acc,
                                false);
}

// ~fold(S) (tcpip.go:66-69) from the little-endian-domain sum S' of the same 16-bit words:
// the one's-complement sum of byte-swapped words is the byte-swapped sum (RFC 1071 §2(B)),
// exactly — an all-zero input gives 0 in both domains, anything else a value in
// [1, 0xFFFF] congruent mod 0xFFFF — as long as neither sum wraps 2^32.  That holds for every
// segment the fast decoders sum: its length comes from a 16-bit IP length (a jumbogram's
// hop-by-hop header sends it to the generic decoder), so it has at most 65,535 bytes = 32,768
// words of at most 0xFFFF each, 0x7FFF8000, and the pseudo-header adds at most 18 words
// (32 address bytes, protocol, length): below 2^31 + 2^21 in either byte order — ro_kernel feeds
// such 64-KiB segments, the windowed kernels at most a window.  Two folds bring any u32 to
// <= 0xFFFF (tests/csum_cases.py folds(): the sums whose second fold carries in one domain only).
__device__ __forceinline__ uint32_t fold_le_not(uint32_t s) {
  s = (s >> 16) + (s & 0xFFFFu);
  s = (s >> 16) + (s & 0xFFFFu);
  return __builtin_amdgcn_perm(0u, ~s, 0x0C0C0001u);  // byte-swap the low half, high half 0
}

// ---------------------------------------------------------------- wave helpers
// Inclusive prefix sum over the 64 lanes: row shifts 1/2/4/8, then row broadcasts 15 / 31.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return v;
}

// max / min / sum over the wave (all 64 lanes take part)
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}

// ---------------------------------------------------------------- result store
__device__ __forceinline__ void store_out(const KParams &P, uint32_t i, const Out &o) {
  if (P.rec) {  // one 32-B gpd_record: {status, csum, layers} and {net_hash, tp_hash}
    v4u32 *r = reinterpret_cast<v4u32 *>(P.rec + i);
    const v4u32 a = {o.status, o.csum, (uint32_t)o.layers, (uint32_t)(o.layers >> 32)};
    const v4u32 b = {(uint32_t)o.net_hash, (uint32_t)(o.net_hash >> 32), (uint32_t)o.tp_hash,
                     (uint32_t)(o.tp_hash >> 32)};
    __builtin_nontemporal_store(a, r);
    __builtin_nontemporal_store(b, r + 1);
    if (P.hdr_off) __builtin_nontemporal_store(o.hoff, P.hdr_off + i);
    return;
  }
  if (P.options & kDiagNtStore) {
    __builtin_nontemporal_store(o.status, P.status + i);
    __builtin_nontemporal_store(o.layers, P.layers + i);
    if (P.net_hash) __builtin_nontemporal_store(o.net_hash, P.net_hash + i);
    if (P.tp_hash) __builtin_nontemporal_store(o.tp_hash, P.tp_hash + i);
    if (P.csum) __builtin_nontemporal_store(o.csum, P.csum + i);
    if (P.hdr_off) __builtin_nontemporal_store(o.hoff, P.hdr_off + i);
    return;
  }
  P.status[i] = o.status;
  P.layers[i] = o.layers;
  if (P.net_hash) P.net_hash[i] = o.net_hash;
  if (P.tp_hash) P.tp_hash[i] = o.tp_hash;
  if (P.csum) P.csum[i] = o.csum;
  if (P.hdr_off) P.hdr_off[i] = o.hoff;
}

// ---------------------------------------------------------------- windows and LDS-DMA
// A window of the batch buffer: bytes [base, base + nbytes) (base 16-aligned).
struct Window {
  uint32_t base, nbytes;
  uint32_t shift;  // rs_kernel: LDS byte of global byte x is buf + shift + (x - base)
};

// A window starts at the first pending packet (rounded down to 16) and covers every pending
// packet lying wholly inside [base, base + STAGE).  Packets normally sit in lane order, so
// the last covered lane's end is the extent; a full wave maximum only runs when some lane
// proves otherwise.
template <int STAGE>
__device__ __forceinline__ Window plan_window(bool pending, uint32_t off, uint32_t end, uint32_t l3m = 14u) {
  Window w{0, 0, 0};
  const uint64_t m = __ballot(pending);
  if (m == 0) return w;
  const uint32_t first = __builtin_amdgcn_readlane(off, (int)__builtin_ctzll(m));
  w.base = first & ~15u;
  // the shift that puts the first packet's byte l3m (mod 16: where the wave's last network
  // header sat, 14 for an untagged frame) on a 16-byte LDS boundary: misaligned DS reads
  // cost ~3.6x aligned ones (tools/micro/lds_align)
  w.shift = (32u - ((first & 15u) + l3m)) & 15u;
  const bool in = pending && off >= w.base && end - w.base <= (uint32_t)STAGE;
  const uint32_t x = in ? end - w.base : 0u;
  const uint64_t mi = __ballot(in);  // nonzero: the first pending lane is in
  uint32_t need = __builtin_amdgcn_readlane(x, 63 - (int)__builtin_clzll(mi));  // last lane in
  if (__any(x > need)) need = __builtin_amdgcn_readfirstlane(wave_max(x));
  w.nbytes = (need + 15u) & ~15u;
  return w;
}

// 16-byte LDS-DMA (global_load_lds_dwordx4): lane l's 16 bytes from gbase + voff land at LDS
// lds + 16 l.  Issued from inline asm so the compiler's waitcnt pass does not see it:
// otherwise it cannot tell the in-flight DMA into the other window from this window's
// ds_reads and drains it (vmcnt(0)) before the first one, serialising the prefetch.  Every
// wait on these loads is therefore explicit (a counted s_waitcnt vmcnt before a window is
// read; loads, stores and LDS-DMA retire in issue order, MI355X_MICROARCH.md).
__device__ __forceinline__ void glds16(const uint8_t *gbase, uint32_t voff, uint32_t lds,
                                       bool nt = false) {
  uint32_t keep;
  if (nt) {
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2 nt\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(gbase), "s"(lds)
        : "memory");
    return;
  }
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(gbase), "s"(lds)
      : "memory");
}

// 4-byte LDS-DMA (global_load_lds_dword): lane l's word from gbase + voff lands at LDS lds + 4 l.
__device__ __forceinline__ void glds4(const void *gbase, uint32_t voff, uint32_t lds) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(gbase), "s"(lds)
      : "memory");
}

}  // namespace gpd
