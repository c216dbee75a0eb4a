// gpd_kernels.hip — MI355X (gfx950) batched DecodingLayerParser kernels: the entry point
// (launch_decode), the generic decoder's kernel and the IPv4 fragment hand-off.
//
// The decode kernels are one translation unit per family over shared device headers:
//   gpd_dev_common.h   option bits, LDS arena, byte sources, wave reductions, folds, FNV, results
//   gpd_dev_tables.h   the dispatch tables as read from LDS
//   gpd_dev_generic.h  decode_packet (the DecodingLayerParser loop) and the fallback lists
//   gpd_dev_fast.h     fast_decode (the straight-line decoder) and the fast loops' helpers
//   gpd_launch.h       host side: launch geometry, the launch, CS / HASH dispatch
//   gpd_kernels.hip    decode_kernel: the generic decoder for every packet (extended records,
//                      other first layers, PAGES tables), over double-buffered LDS-DMA windows
//   gpd_rs.hip         rs_kernel: the fast path, windows staged through registers
//   gpd_ro.hip         ro_kernel: the fast path for long frames, header-once over 8 KiB rounds
//   gpd_sp.hip         sp_kernel: the fast path for small frames, loader / decoder split
// A batch takes one of the fast kernels when fast_eligible (below) holds — the straight-line
// decoder per packet, the generic one for the packets it leaves — and decode_kernel otherwise.
#include <hip/hip_runtime.h>

#include "gpd_compact.h"
#include "gpd_dev_generic.h"
#include "gpd_launch.h"

namespace gpd {

// Per-lane source offsets of a window: wave instruction c writes physical slots
// [64c, 64c+64); lane l's source is the logical slot that lands on slot 64c + l — for the
// rotated layout (gpd_dev_common.h swz_slot) that depends on c mod 4 only (four per-lane
// constants).
struct DmaLanes {
  uint32_t voff[4];
  __device__ __forceinline__ explicit DmaLanes(uint32_t lane) {
#pragma unroll
    for (int j = 0; j < 4; j++) voff[j] = 16u * ((lane & 48u) + ((lane - (lane >> 4) - 4u * j) & 15u));
  }
};

__device__ __forceinline__ void issue_window(const uint8_t *data, const Window &w, uint32_t buf,
                                             const DmaLanes &L, bool nt = false) {
  for (uint32_t c4 = 0; c4 < w.nbytes; c4 += 4096u) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t c = c4 + 1024u * j;
      if (c >= w.nbytes) break;
      if (c + 1024u <= w.nbytes || c + L.voff[j] < w.nbytes)
        glds16(data + w.base + c, L.voff[j], buf + c, nt);
    }
  }
}

// ---------------------------------------------------------------- kernel
constexpr int kGenWaves = 4;  // waves per workgroup
// LDS bytes per wave: two windows and two descriptor slots.
__host__ __device__ constexpr uint32_t wave_lds_bytes(int stage) { return 2u * stage + 1024u; }
static_assert(kGenWaves * wave_lds_bytes(4096) == 36864 && kGenWaves * wave_lds_bytes(8192) == 69632,
              "the workgroup LDS bytes gpd_launch.h pins launch_geom with");

// The generic decoder (decode_packet) for every packet.  Each wave owns 64-packet tiles t,
// t + W, ... (grid stride).  A tile's bytes are staged through LDS windows of STAGE bytes (a tile
// of large packets takes several; a packet larger than a window is decoded straight from global
// memory: same code, other byte source), and the window is the pipeline unit: per wave, LDS
// holds two window buffers, their 16-byte slots rotated against bank conflicts, and two
// descriptor slots (the 64 offsets and caplens of a tile), all filled by LDS-DMA, so the loop
// has no compiler-visible global loads and every wait is an explicit, counted one.  Iteration k:
//   wait for window k -> plan and issue window k+1 (the rest of this tile, or the next
//   tile's first window, whose descriptors arrived two tiles ago; then the descriptors two
//   tiles further on) -> decode window k's packets from LDS -> when window k ended its
//   tile, store the tile's 64 results.
template <int STAGE, bool EXT, bool PAGES>
__global__ __launch_bounds__(64 * kGenWaves, 1) void decode_kernel(KParams P) {
  constexpr int WAVES = kGenWaves;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // stage the dispatch-table image into LDS (inline in every kernel: gpd_dev_common.h g_lds)
  for (uint32_t k = threadIdx.x; k < P.image_words; k += 64 * WAVES)
    reinterpret_cast<uint32_t *>(g_lds)[k] = P.image[k];
  __syncthreads();
  const Tab<PAGES> T = make_tab<PAGES>(P);
  const uint32_t img = (P.image_words * 4u + 15u) & ~15u;
  const uint32_t bufs = img + wave * wave_lds_bytes(STAGE);
  const uint32_t dslots = bufs + 2u * STAGE;  // two slots of 64 offsets + 64 caplens
  const uint32_t n = P.n_dev ? min((uint32_t)P.n, *P.n_dev) : (uint32_t)P.n;  // <= kMaxLaunchPackets
  const uint32_t ntiles = (n + 63u) >> 6;
  const uint32_t nwaves = gridDim.x * WAVES;
  const uint32_t dlen = (uint32_t)P.data_len;
  const uint32_t fits = (uint32_t)STAGE - 15u;  // a packet of <= fits bytes always fits a window
  const uint32_t options = P.options & ~kDiagMask;
  const bool nt = P.options & kDiagNtLoad;
  const uint32_t nst = EXT ? 0u : P.nstores;  // result stores per tile (EXT: drain fully)
  const DmaLanes L(lane);

  uint32_t tp = blockIdx.x * WAVES + wave;  // the planner's tile
  if (tp >= ntiles) return;
  auto desc_issue = [&](uint32_t u, uint32_t slot) -> uint32_t {  // descriptors of tile u
    if (u >= ntiles) return 0u;
    if (u * 64u + lane < n) {
      glds4(P.offset + u * 64u, 4u * lane, dslots + slot * 512u);
      glds4(P.caplen + u * 64u, 4u * lane, dslots + slot * 512u + 256u);
    }
    return 2u;  // VMEM instructions issued
  };
  // per-lane flags are kept as 0/1 words (VGPRs), not lane masks (SGPR pairs)
  auto desc_read = [&](uint32_t u, uint32_t slot, uint32_t &off, uint32_t &end) -> uint32_t {
    const uint32_t v = u * 64u + lane < n ? 1u : 0u;
    const uint32_t o = v ? min(lds_u32(dslots + slot * 512u + 4u * lane), dlen) : 0u;
    const uint32_t l = v ? min(lds_u32(dslots + slot * 512u + 256u + 4u * lane), dlen - o) : 0u;
    off = o;  // a packet reaching past data_len is clamped to the buffer
    end = o + l;
    return v;
  };
  auto covered = [&](const Window &w, uint32_t pend, uint32_t off, uint32_t end) -> uint32_t {
    return (pend && off >= w.base && end - w.base <= (uint32_t)STAGE) ? 1u : 0u;
  };

  // prologue: descriptors of the first two tiles, then the first window
  desc_issue(tp, 0);
  desc_issue(tp + nwaves, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t slot = 0;  // descriptor slot of the planner's tile
  uint32_t off_p, end_p;
  uint32_t valid_p = desc_read(tp, slot, off_p, end_p);
  uint32_t pend_p = (valid_p && end_p - off_p <= fits) ? 1u : 0u;  // still to be given a window
  const uint32_t big0 = valid_p & (pend_p ^ 1u);
  Window Wd = plan_window<STAGE>(pend_p != 0, off_p, end_p);
  uint32_t cov_d = covered(Wd, pend_p, off_p, end_p);
  pend_p &= cov_d ^ 1u;
  issue_window(P.data, Wd, bufs, L, nt);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot read before it is restaged
  uint32_t nwait = desc_issue(tp + 2u * nwaves, slot);

  // decode state: the window in flight belongs to tile td
  uint32_t td = tp, off_d = off_p, end_d = end_p;
  uint32_t valid_d = valid_p, big_d = big0;
  bool first_d = true;
  uint32_t cur = 0;  // buffer of the window to decode
  Out res{0, 0, 0, 0, 0, 0};
  for (;;) {
    // window cur landed: wait for all but the VMEM instructions issued after it
    if (!(P.options & kDiagNoWait)) {
      switch (nwait) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      }
    }
    // ---- plan and issue the next window
    Window Wn{0, 0, 0};
    uint32_t cov_n = 0;
    bool has_next = false, new_tile = false;
    if (__any(pend_p != 0)) {  // more of the planner's tile
      Wn = plan_window<STAGE>(pend_p != 0, off_p, end_p);
      has_next = true;
    } else if (tp + nwaves < ntiles) {  // the next tile's first window
      tp += nwaves;
      slot ^= 1u;
      valid_p = desc_read(tp, slot, off_p, end_p);
      pend_p = (valid_p && end_p - off_p <= fits) ? 1u : 0u;
      Wn = plan_window<STAGE>(pend_p != 0, off_p, end_p);
      has_next = new_tile = true;
    }
    nwait = 0;
    if (has_next) {
      cov_n = covered(Wn, pend_p, off_p, end_p);
      pend_p &= cov_n ^ 1u;
      issue_window(P.data, Wn, bufs + (cur ^ 1u) * STAGE, L, nt);
      if (new_tile) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot read before it is restaged
        nwait = desc_issue(tp + 2u * nwaves, slot);
      }
    }
    // ---- decode window cur (tile td, the lanes it covers)
    const uint32_t i = td * 64u + lane;
    const uint32_t clen = end_d - off_d;
    if (first_d && big_d)  // larger than a window
      res = decode_packet<EXT>(GlbSrc{P.data, off_d}, clen, T, P.first, options, EXT ? P.ext + i : nullptr,
                               P.detail ? P.detail + i : nullptr);
    const uint32_t buf = bufs + cur * STAGE;
    if (cov_d && (P.options & kDiagSkipDecode)) {  // diagnostics: data movement only
      res = Out{g_lds[buf + ((off_d - Wd.base) & ~15u)], 0, 0, 0, 0, 0};
    } else if (cov_d) {
      const LdsSrc<true> src{buf, off_d - Wd.base};
      res = decode_packet<EXT>(src, clen, T, P.first, options, EXT ? P.ext + i : nullptr,
                               P.detail ? P.detail + i : nullptr);
    }
    // ---- the tile is complete when the next window belongs to another tile (or none)
    if (!has_next || new_tile) {
      if (valid_d) store_out(P, i, res);
      nwait += nst;
    }
    if (!has_next) break;
    if (new_tile) {
      td = tp;
      off_d = off_p;
      end_d = end_p;
      valid_d = valid_p;
      big_d = (valid_p && end_p - off_p > fits) ? 1u : 0u;
      first_d = true;
    } else {
      first_d = false;
    }
    Wd = Wn;
    cov_d = cov_n;
    cur ^= 1u;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads of the freed buffer done
  }
}

// As many workgroups per CU as LDS admits, always four rounds of them; no fallback regions (and
// neither gpd_tuning.waves_per_simd nor grid_rounds: they tune the fast kernels).
template <int STAGE, bool EXT, bool PAGES>
static hipError_t launch_t(KParams &P, hipStream_t stream, int num_cus) {
  const LaunchGeom g = launch_geom(P.image_words, kGenWaves * (size_t)wave_lds_bytes(STAGE), kGenWaves, 0,
                                   kNoResidencyCap, 0, kGridRounds, num_cus, (P.n + 63) / 64);
  return launch_kernel(decode_kernel<STAGE, EXT, PAGES>, 64 * kGenWaves, g, P, stream, num_cus);
}

template <bool EXT, bool PAGES>
static hipError_t launch_s(KParams &P, hipStream_t stream, int num_cus) {
  if (P.stage == 4096) return launch_t<4096, EXT, PAGES>(P, stream, num_cus);
  return launch_t<8192, EXT, PAGES>(P, stream, num_cus);
}

// ---------------------------------------------------------------- IPv4 fragment hand-off
// include/gpd_defrag.h: the packets for which IPv4Defragmenter.DefragIPv4 does not return the
// layer unchanged (dontDefrag, ip4defrag/defrag.go:162-172), in packet order, with the key and
// securityChecks verdict (:175-198).  Four launches: per-2048-packet candidate counts (and one
// candidate bit per packet), their exclusive scan, the candidates' packet indices in order, and
// one record per candidate.

// Can packet i's IPv4 object (as the call leaves it: the last IPv4 in decoded, or a later IPv4
// call that failed after assigning its fields) be a fragment?  From the result words first: a fragmented IPv4 layer ends the decode (ip4.go:281-286, its next layer is
// gopacket.Fragment, which decodes nothing further), so decoded ends [.., IPv4, Fragment], or
// [.., IPv4] with Fragment unregistered (stop type 3) or the payload empty (stop 0).  Then the
// flags/offset word of the header (ip4.go:193,200-201), which also rules out DF (:164-166).
__device__ __forceinline__ bool frag_candidate(const KParams &P, uint32_t i) {
  uint32_t st;
  uint64_t lw;
  if (P.rec) {
    st = P.rec[i].status;
    lw = P.rec[i].layers;
  } else {
    st = P.status[i];
    lw = P.layers[i];
  }
  if (GPD_STATUS_NET_EPT(st) != 1u) return false;  // the last network layer is not IPv4
  const uint32_t nl = GPD_STATUS_NLAYERS(st);
  // After a decode error the ip4 object may hold a later, failed IPv4 header (ip4.go:195-210
  // assign its fields before the Length/IHL checks) wherever decoded ends: the header decides.
  if (GPD_STATUS_CLASS(st) != GPD_ST_DECODE_ERROR && nl <= GPD_CORE_MAX_LAYERS &&
      !GPD_STATUS_SATURATED(st)) {
    const uint32_t last = GPD_LAYERS_CODE(lw, nl - 1), stop = GPD_LAYERS_STOP(lw);
    const bool maybe = (last == GPD_C_FRAGMENT && nl >= 2 && GPD_LAYERS_CODE(lw, nl - 2) == GPD_C_IPV4) ||
                       (last == GPD_C_IPV4 && (stop == 0 || stop == GPD_LT_FRAGMENT));
    if (!maybe) return false;
  }
  const uint32_t net = GPD_HDR_NET(P.hdr_off[i]);
  if (net == GPD_HDR_NONE) return true;  // header past byte 65534: the record pass decides
  const uint32_t dlen = (uint32_t)P.data_len;
  const uint32_t off = min(P.offset[i], dlen);
  const uint8_t *h = P.data + off + net;  // a decoded IPv4 header: 20 bytes inside the packet
  const uint32_t flags = h[6] >> 5, fo = ((h[6] & 0x1Fu) << 8) | h[7];
  if (flags & 2u) return false;  // IPv4DontFragment
  return (flags & 1u) || fo != 0;
}

// The compaction (gpd_compact.h, shared with the tcpassembly hand-off): candidate bits and
// per-block counts, their exclusive scan, the candidates' packet indices in order (fragments are
// rare: the index pass usually writes nothing at all).
__global__ __launch_bounds__(256) void frag_count_kernel(FragArgs A) {
  compact_count((uint32_t)A.P.n, A.mask, A.blk, [&A](uint32_t i) { return frag_candidate(A.P, i); });
}

__global__ __launch_bounds__(1024) void frag_scan_kernel(FragArgs A) { compact_scan(A.blk, A.nblk); }

__global__ __launch_bounds__(64) void frag_index_kernel(FragArgs A) {
  compact_index(A.blk, A.mask, A.idx, (uint32_t)A.P.n);
}

// One lane per candidate: the generic decoder re-runs the packet for the IPv4 object's exact
// state (its Contents/Payload, so a TSO Length of 0 and truncation come out as the reference
// leaves them), then dontDefrag and securityChecks on it.
template <bool PAGES>
__global__ __launch_bounds__(256) void frag_record_kernel(FragArgs A) {
  const KParams &P = A.P;
  const uint32_t cnt = min(A.blk[A.nblk], A.max_out);
  if (cnt <= blockIdx.x * 256u) return;
  for (uint32_t k = threadIdx.x; k < P.image_words; k += 256) reinterpret_cast<uint32_t *>(g_lds)[k] = P.image[k];
  __syncthreads();
  const Tab<PAGES> T = make_tab<PAGES>(P);
  const uint32_t dlen = (uint32_t)P.data_len;
  const uint32_t options = P.options & ~kDiagMask;
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < cnt; j += gridDim.x * 256u) {
    const uint32_t i = A.idx[j];
    const uint32_t off = min(P.offset[i], dlen), len = min(P.caplen[i], dlen - off);
    gpd_ext_rec e;
    decode_packet<true>(GlbSrc{P.data, off}, len, T, P.first, options, &e);
    const gpd_layer_rec o = e.obj[GPD_OBJ_IPV4];
    gpd_ip4_frag r{};
    r.packet = i;
    r.verdict = GPD_FRAG_WHOLE;
    if (e.obj_valid & (1u << GPD_OBJ_IPV4)) {
      const uint8_t *h = P.data + off + o.contents_off;
      const uint32_t raw_len = ((uint32_t)h[2] << 8) | h[3], ff = ((uint32_t)h[6] << 8) | h[7];
      r.net_off = o.contents_off;
      for (int b = 0; b < 4; ++b) {
        r.src[b] = h[12 + b];
        r.dst[b] = h[16 + b];
      }
      r.id = (uint16_t)(((uint32_t)h[4] << 8) | h[5]);
      r.flags = (uint8_t)(ff >> 13);
      r.frag_offset = (uint16_t)(ff & 0x1FFFu);
      r.ihl = h[0] & 0x0Fu;
      // ip4.go:214-218: Length 0 => len(data); the decode then keeps all of data, so it is
      // Contents + Payload
      r.length = (uint16_t)(raw_len ? raw_len : o.contents_len + o.payload_len);
      r.payload_len = o.payload_len;
      const bool dont = (r.flags & 2u) || (!(r.flags & 1u) && r.frag_offset == 0);  // defrag.go:162-172
      const uint16_t frag_size = (uint16_t)(r.length - (uint16_t)(r.ihl * 4u));        // :176
      if (dont) r.verdict = GPD_FRAG_WHOLE;
      else if (frag_size < 8u) r.verdict = GPD_FRAG_TOO_SMALL;                           // :179
      else if (r.frag_offset > 8183u) r.verdict = GPD_FRAG_OFFSET;                       // :185
      else if ((uint16_t)(r.frag_offset * 8u + r.length) > 65535u) r.verdict = GPD_FRAG_OVERRUN;  // :192, uint16
      else r.verdict = GPD_FRAG_INSERT;
    }
    A.out[j] = r;
  }
}

hipError_t launch_ip4_frag(const FragArgs &A, hipStream_t stream, int num_cus) {
  if (A.nblk == 0) return hipSuccess;
  hipLaunchKernelGGL(frag_count_kernel, dim3(A.nblk), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(frag_scan_kernel, dim3(1), dim3(1024), 0, stream, A);
  hipLaunchKernelGGL(frag_index_kernel, dim3(A.nblk), dim3(64), 0, stream, A);
  if (A.max_out == 0) return hipGetLastError();
  const size_t lds = (A.P.image_words * 4u + 15u) & ~15u;
  const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)num_cus * 2, (A.max_out + 255u) / 256u);
  if (A.P.use_pages) hipLaunchKernelGGL(frag_record_kernel<true>, dim3(grid), dim3(256), lds, stream, A);
  else hipLaunchKernelGGL(frag_record_kernel<false>, dim3(grid), dim3(256), lds, stream, A);
  return hipGetLastError();
}

bool fast_eligible(const KParams &P) {
  // the fast kernel: Ethernet first and registered, hashed tables, no extended records
  return !P.ext && !P.use_pages && P.fixed && P.first == GPD_LT_ETHERNET &&
         (P.decoders & GPD_DEC_ETHERNET);
}

// The fast path's kernel family for a batch.
static hipError_t launch_fast(KParams &P, hipStream_t stream, int num_cus) {
  if (P.options & kRounds)  // header-once over 8 KiB rounds of each tile's run (ro_kernel)
    return launch_fast_ro(P, stream, num_cus);
  // (the split kernel writes gpd_records: with the five SoA arrays its seven decoders per
  // workgroup ran 0.397 ms against the register loop's 0.319 on config 2, same box; the
  // diagnostic library's skeleton runs are rs_kernel's)
  if (P.stage == 4096 && P.split && P.rec && !(P.options & kDiagSkipDecode)) return launch_fast_sp(P, stream, num_cus);
  return launch_fast_rs(P, stream, num_cus);
}

hipError_t launch_decode(const KParams &P0, hipStream_t stream, int num_cus, hipEvent_t mid,
                         uint32_t *fb_waves) {
  KParams P = P0;
  P.fb_waves = 0;
  if (P.n > kMaxLaunchPackets) return hipErrorInvalidValue;
  if (fast_eligible(P)) {
    if (!P.fb_list || !P.fb_wcount) return hipErrorInvalidValue;
    hipError_t e = launch_fast(P, stream, num_cus);
    if (e != hipSuccess) return e;
    if (fb_waves) *fb_waves = P.fb_waves;
    if (mid && (e = hipEventRecord(mid, stream)) != hipSuccess) return e;
    return hipSuccess;  // (each fast wave decodes its own fallback list: one launch)
  }
  if (P.ext) return P.use_pages ? launch_s<true, true>(P, stream, num_cus)
                                : launch_s<true, false>(P, stream, num_cus);
  return P.use_pages ? launch_s<false, true>(P, stream, num_cus)
                     : launch_s<false, false>(P, stream, num_cus);
}

}  // namespace gpd
