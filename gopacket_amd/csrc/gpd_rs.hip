// gpd_rs.hip — rs_kernel, the fast path's register-staged streaming loop (4 KiB and 8 KiB
// windows, with the header-once and aligned-window variants), its launch, and the choice among
// its instances (the skeleton instances of the diagnostic library included).
#include <hip/hip_runtime.h>

#include "gpd_dev_fast.h"
#include "gpd_dev_generic.h"
#include "gpd_launch.h"

namespace gpd {

#ifdef GPD_PHASE_TIMING
__device__ unsigned long long g_phase[8];  // the PH_* marks' totals (gpd_dev_common.h)
#endif

// LDS bytes per wave of rs_kernel: one window (the next one waits in VGPRs), plus the chunk
// prefix sums of the cooperative checksum for windows of 8 KiB and more.
__host__ __device__ constexpr uint32_t rs_wave_lds_bytes(int stage) {
  return (uint32_t)stage + 16u + (stage >= 8192 ? (uint32_t)stage / 4u + 16u : 0u);
}
static_assert(4 * rs_wave_lds_bytes(4096) == 16448 && 4 * rs_wave_lds_bytes(8192) == 41088,
              "the workgroup LDS bytes gpd_launch.h pins launch_geom with");

// The fast path's streaming loop with the window staged through registers: a window's bytes
// are loaded with plain 16-byte-per-lane loads (nt: read once) into VGPRs while the previous
// window is decoded out of the wave's single LDS buffer, then copied into that buffer with
// ds_write_b128 at the top of the next iteration.  Descriptors are register loads two tiles
// ahead.  Every load is compiler-visible, so each wait is the compiler's, placed at the first
// use.  Measured on this part (tools/micro/hbm_mix.hip): the decode kernel's 72-B-read /
// 32-B-write traffic shape streams at ~6.0 TB/s through registers against ~5.2 TB/s through
// LDS-DMA, and one LDS buffer per wave (instead of two) frees LDS for more waves.
// Iteration k:  commit window k (VGPR -> LDS)  ->  store the results of the tile the previous
// window finished (deferred one iteration, so that after the next window's loads nothing else
// is issued and the wait at the next commit covers exactly those loads)  ->  plan and load
// window k+1  ->  decode window k from LDS.
template <int STAGE, bool CS, bool HASH, int MINW, bool DEFER = false, bool RPFX = true, bool HO = false,
          bool AL = false, bool DIAG = kDiagBuild>
__global__ __launch_bounds__(256, MINW) void rs_kernel(KParams P) {
  constexpr int WAVES = 4;
  constexpr int NC = STAGE / 1024;              // 16-byte chunks per lane per window
  constexpr bool COOP = STAGE >= 8192;          // long segments: wave-cooperative checksum
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t k = threadIdx.x; k < P.image_words; k += 64 * WAVES)
    reinterpret_cast<uint32_t *>(g_lds)[k] = P.image[k];
  __syncthreads();
  const uint32_t img = (P.image_words * 4u + 15u) & ~15u;
  const uint32_t buf = img + wave * rs_wave_lds_bytes(STAGE);
  const uint32_t pfx = buf + STAGE + 16u;
  const uint32_t n = P.n_dev ? min((uint32_t)P.n, *P.n_dev) : (uint32_t)P.n;
  const uint32_t ntiles = (n + 63u) >> 6;
  const uint32_t nwaves = gridDim.x * WAVES;
  const uint32_t dlen = (uint32_t)P.data_len;
  const uint32_t fits = (uint32_t)STAGE - 15u;
  const uint32_t options = P.options & ~kDiagMask;
  const FastCtx F = fast_ctx(P, options);

  uint32_t tp = blockIdx.x * WAVES + wave;  // the planner's tile
  // Fallback list: wave w (tiles w, w + nwaves, ...) owns the region of 64 x its tile count
  // that starts after the regions of waves 0..w-1, so its appends need no atomic (a shared
  // counter took one same-address atomic per tile with leftovers; on the traffic mix that is
  // every tile, serialised at the memory side); the wave decodes its region after its tiles.
  const uint32_t gw = tp;
  const uint32_t fb_start = 64u * (gw * (ntiles / nwaves) + min(gw, ntiles % nwaves));
  uint32_t fb_c = 0;
  if (tp >= ntiles) {
    if (lane == 0u) P.fb_wcount[gw] = 0u;
    return;
  }
  const TileDesc D{P, lane, n, ntiles, dlen};
  auto covered = [&](const Window &w, uint32_t pend, uint32_t off, uint32_t end) -> uint32_t {
    return (pend && off >= w.base && end - w.base <= (uint32_t)STAGE) ? 1u : 0u;
  };
  // Window loads are unconditional (a chunk past the window's end re-reads its first 16
  // bytes, a cached line), so every lane's registers come from this window's loads and the
  // compiler needs no merge of older values: its only wait is at the commit.
  v4u32 wv[NC];
  const bool ntl = (P.options & kDiagNtLoad) != 0;  // read-once policy (default on; A/B knob)
  auto wload = [&](const Window &w) {
#pragma unroll
    for (int j = 0; j < NC; j++) {
      const uint32_t c = 1024u * j + 16u * lane;
      const v4u32 *a = reinterpret_cast<const v4u32 *>(P.data + w.base + (c < w.nbytes ? c : 0u));
      wv[j] = ntl ? __builtin_nontemporal_load(a) : *a;
    }
    __builtin_amdgcn_sched_barrier(0);  // issue them here, ahead of the decode
  };
  // Shifted copies pay for themselves where windows hold many small frames; the host sets
  // the bit from the batch's mean slot (measured: tools/ab_shift.sh).
  const bool noshift = AL || (P.options & kShiftWindows) == 0;  // (AL: launched for unshifted windows only)
  auto wshift = [&](const Window &w) -> uint32_t { return noshift ? 0u : w.shift; };
  // COOP: the chunk prefix sums of a window are computed from the registers as it is
  // committed when the wave's previous window needed them (`pfx_pred`); otherwise, if this
  // window turns out to need them, window_prefix reads them back from LDS.
  bool pfx_pred = COOP, pfx_done = false;
  auto wcommit = [&](const Window &w) {
    const uint32_t sh = wshift(w);
    uint32_t cs[NC];
    pfx_done = false;
    const bool sums = COOP && RPFX && pfx_pred && sh == 0u;
    if (sh == 0u) {
#pragma unroll
      for (int j = 0; j < NC; j++)
        *reinterpret_cast<v4u32 *>(g_lds + buf + 1024u * j + 16u * lane) = wv[j];
      if (sums) {
#pragma unroll
        for (int j = 0; j < NC; j++)
          cs[j] = dot2(wv[j].w, 0x00010001u, dot2(wv[j].z, 0x00010001u,
                       dot2(wv[j].y, 0x00010001u, dot2(wv[j].x, 0x00010001u, 0u))));
      }
    } else {
      // (shifted windows leave the prefix to window_prefix: measured, pcap64 +2 % otherwise)
      const uint32_t o = 16u - sh, r = o & 3u;
      switch (o >> 2) {
        case 0: commit_shifted<0, NC, false>(wv, buf, lane, r, cs); break;
        case 1: commit_shifted<1, NC, false>(wv, buf, lane, r, cs); break;
        case 2: commit_shifted<2, NC, false>(wv, buf, lane, r, cs); break;
        default: commit_shifted<3, NC, false>(wv, buf, lane, r, cs); break;
      }
    }
    if (sums) {
      rows_prefix<NC>(cs, pfx, lane);
      pfx_done = true;
    }
  };

  // prologue: this tile's descriptors (waited for), the next two tiles' in flight
  uint32_t o_a, c_a, o_b, c_b, off_p, end_p;
  {
    uint32_t o0, c0;
    D.load(tp, o0, c0);
    D.load(tp + nwaves, o_a, c_a);
    D.load(tp + 2u * nwaves, o_b, c_b);
    (void)D.read(tp, o0, c0, off_p, end_p);
  }
  uint32_t valid_p = tp * 64u + lane < n ? 1u : 0u;
  uint32_t pend_p = (valid_p && end_p - off_p <= fits) ? 1u : 0u;
  uint32_t l3m = 14u;  // network header offset mod 16 the window shift aims at (learned)
  Window Wd = plan_window<STAGE>(pend_p != 0, off_p, end_p, l3m);
  uint32_t cov_d = covered(Wd, pend_p, off_p, end_p);
  pend_p &= cov_d ^ 1u;
  wload(Wd);
  uint32_t td = tp, off_d = off_p, end_d = end_p, valid_d = valid_p;
  uint32_t big_d = valid_p & ((end_p - off_p <= fits) ? 0u : 1u);
  bool first_d = true;
  Out res{0, 0, 0, 0, 0, 0};
  uint32_t fb = 0;
  Hdr hh{};          // HO: the lane's packet as seg_pass staged it
  uint32_t got = 0;  // HO: ... in one of this tile's windows (2: decoded there in full)
  const bool vxreg = (P.decoders & GPD_DEC_VXLAN) != 0;
  // results of a finished tile, stored one iteration later
  bool st_pending = false;
  uint32_t st_i = 0, st_valid = 0;
  Out st_res{0, 0, 0, 0, 0, 0};
  PH_DECL
  for (;;) {
    PH_MARK(5);  // loop overhead / tail of the previous iteration
    // Wait order: every load issued in the previous iteration (descriptors two tiles ahead,
    // then window k) is older than anything the wait below could over-cover, so the
    // compiler's vmcnt at the first use of window k's registers costs nothing extra.
    wcommit(Wd);  // window k: registers -> LDS (the compiler waits for its loads here)
    PH_MARK(0);  // waiting for the window (and copying it)
    // ---- plan the next window (the next tile's descriptors landed long ago)
    Window Wn{0, 0, 0};
    uint32_t cov_n = 0;
    bool has_next = false, new_tile = false;
    if (__any(pend_p != 0)) {  // more of the planner's tile
      has_next = true;
    } else if (tp + nwaves < ntiles) {  // the next tile's first window
      tp += nwaves;
      valid_p = D.read(tp, o_a, c_a, off_p, end_p);
      o_a = o_b;
      c_a = c_b;
      pend_p = (valid_p && end_p - off_p <= fits) ? 1u : 0u;
      has_next = new_tile = true;
    }
    // ---- the previous tile's results (a fallback lane's entry is rewritten later), issued
    // before the next loads so that nothing follows those loads until their wait
    if (DEFER && st_pending) {
      if (st_valid) store_out(P, st_i, st_res);
      st_pending = false;
    }
    if (new_tile) D.load(tp + 2u * nwaves, o_b, c_b);
    if (has_next) {
      Wn = plan_window<STAGE>(pend_p != 0, off_p, end_p, l3m);
      cov_n = covered(Wn, pend_p, off_p, end_p);
      pend_p &= cov_n ^ 1u;
      wload(Wn);
    }
    PH_MARK(1);  // stores of the previous tile, planning and issuing the next window
    // ---- decode window k (tile td, the lanes it covers)
    const uint32_t i = td * 64u + lane;
    if (first_d && big_d) fb = 1;  // larger than a window: the generic decoder
    Seg sg{0, 0, 0};
    if (DIAG && cov_d && (P.options & kDiagSkipDecode)) {  // diagnostics: data movement only
      res = Out{g_lds[buf + ((off_d - Wd.base) & ~15u)], 0, 0, 0, 0, 0};
    } else if (cov_d) {
      if (HO) {
        seg_pass<COOP>(buf + wshift(Wd) + (off_d - Wd.base), end_d - off_d, buf, hh, sg, F, vxreg);
        got = 1;
      } else if (!fast_decode<CS, HASH, COOP, false, AL>(buf + wshift(Wd) + (off_d - Wd.base), end_d - off_d, F,
                                                          res, buf, sg)) {
        fb = 1;
      }
    }
    const uint64_t vxm = HO ? __ballot(cov_d && hh.ok == 2u) : 0ull;
    if (HO && vxm) {  // VXLAN: its inner headers are not staged
      // A few VXLAN lanes go to the generic decoder: the per-window two-pass decode would run
      // for the whole wave in every window that holds one (on the traffic mix, 5 % VXLAN,
      // nearly every window: 0.44 ms against 0.29 without VXLAN registered).  Many lanes
      // (VXLAN-heavy long-frame traffic) decode in full while their window is here.
      if (cov_d && hh.ok == 2u) {
        got = 2;
        if (__popcll(vxm) <= 16) {
          fb = 1;
        } else if (!fast_decode<CS, HASH, COOP, false, AL>(buf + wshift(Wd) + (off_d - Wd.base), end_d - off_d,
                                                            F, res, buf, sg)) {
          fb = 1;
        }
      }
    }
    if constexpr (!AL) {  // learn where this wave's network headers sit (mod 16) for the next windows' shift
      const uint32_t no = res.hoff & 0xFFFFu;
      const uint64_t hm = __ballot(cov_d && no != 0xFFFFu);
      if (hm) l3m = (uint32_t)__builtin_amdgcn_readlane((int)no, (int)__builtin_ctzll(hm)) & 15u;
    }
    PH_MARK(2);  // decode
    if constexpr (COOP) {  // long segments of this window: chunk prefix sums, shared
      pfx_pred = __any(sg.b > sg.a);
      if (pfx_pred) {
        if (!pfx_done) window_prefix<STAGE>(buf, pfx, lane);
        if (sg.b > sg.a) {
          const uint32_t mid = lds_u32(pfx + 4u * sg.b) - lds_u32(pfx + 4u * sg.a);
          if (HO && got == 1u) hh.sum = sg.part + mid;
          else res.csum |= fold_le_not(sg.part + mid) << 16;
        }
      }
    }
    PH_MARK(3);  // cooperative checksum
    // ---- the tile is complete when the next window belongs to another tile (or none)
    if (!has_next || new_tile) {
      if (HO && got == 1u) {  // the tile's one decode, from the staged headers
        Seg none{0, 0, 0};
        if (!fast_decode<CS, HASH, COOP, true>(0u, end_d - off_d, F, res, buf, none, &hh)) fb = 1;
      }
      got = 0;
      // the tile's leftovers go to the fallback list (fb_append inline: called by reference, by
      // value or as a closure it shifts this kernel's register allocation — tools/isa_diff.py)
      const uint64_t m = __ballot(fb != 0);
      if (m) {
        if (fb) P.fb_list[fb_start + fb_c + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                               __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = ((uint64_t)off_d << 32) | i;
        fb_c += (uint32_t)__popcll(m);
      }
      const uint32_t keep = valid_d && !fb;  // a listed packet is stored once, by its decode below
      fb = 0;
      if (DEFER) {
        st_pending = true;
        st_i = i;
        st_valid = keep;
        st_res = res;
      } else if (keep) {
        store_out(P, i, res);
      }
    }
    PH_MARK(4);  // fallback list (and this tile's stores when not deferred)
    if (!has_next) {
      if (DEFER && st_valid) store_out(P, st_i, st_res);
      PH_FLUSH;
      break;
    }
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
  }
  if (lane == 0u) P.fb_wcount[gw] = fb_c;  // (gpd_last_launch_split's count)
  decode_fallback_list<(uint32_t)STAGE / 64u, CS, HASH>(P, buf, fb_start, fb_c, lane, dlen, options);
}

// MINW workgroups of four waves per CU (what LDS admits, fewer under gpd_tuning.waves_per_simd),
// each wave with a fallback region of its own.
template <int STAGE, bool CS, bool HASH, int MINW, bool DEFER = false, bool RPFX = true, bool HO = false,
          bool AL = false, bool DIAG = false>
static hipError_t launch_rs(KParams &P, hipStream_t stream, int num_cus) {
  // rounds of resident workgroups: the AL kernel (VXLAN-sized frames) runs one — each wave's
  // tiles four times longer — measured 2.2 % faster than four (and 1.6 % than two) on config
  // 4; config 2, IMIX, pcap64 and the traffic mix keep four (one: +1-2 %, two: within noise;
  // tools/ab_rounds.sh, profiles/r03/rounds_ab/)
  const uint64_t rounds = P.rounds ? P.rounds : (AL ? 1u : kGridRounds);
  const LaunchGeom g = launch_geom(P.image_words, 4 * (size_t)rs_wave_lds_bytes(STAGE), 4, 4, MINW, P.waves, rounds,
                                   num_cus, (P.n + 63) / 64);
  return launch_kernel(rs_kernel<STAGE, CS, HASH, MINW, DEFER, RPFX, HO, AL, DIAG>, 256, g, P, stream, num_cus);
}

// One register budget per kernel sets its waves per SIMD (VGPRs <= 512 / MINW): 4 for 4 KiB
// windows, 3 for 8 KiB — what LDS admits, no spills; gpd_tuning.waves_per_simd caps the
// residency below that through the LDS reservation (launch_geom), it does not pick another
// instantiation.  The register-computed chunk prefix pays off for long frames only (IMIX -3 %);
// with small frames (pcap records, VXLAN) its extra registers and code cost 1-2 %.
template <bool CS, bool HASH>
static hipError_t launch_rs_for(KParams &P, hipStream_t stream, int num_cus) {
  if constexpr (kDiagBuild) {  // libgpd_diag.so: the skeleton (no decode) instantiations
    if (P.options & kDiagSkipDecode) {
      if (P.stage == 4096) return launch_rs<4096, CS, HASH, 4, false, true, false, false, true>(P, stream, num_cus);
      if (P.options & kHeaderOnce) return launch_rs<8192, CS, HASH, 3, false, true, true, false, true>(P, stream, num_cus);
      if (P.options & kRegPrefix) return launch_rs<8192, CS, HASH, 3, false, true, false, false, true>(P, stream, num_cus);
      if (!(P.options & kShiftWindows))
        return launch_rs<8192, CS, HASH, 3, false, false, false, true, true>(P, stream, num_cus);
      return launch_rs<8192, CS, HASH, 3, false, false, false, false, true>(P, stream, num_cus);
    }
  }
  if (P.stage == 4096) return launch_rs<4096, CS, HASH, 4>(P, stream, num_cus);
  if (P.options & kHeaderOnce) return launch_rs<8192, CS, HASH, 3, false, true, true>(P, stream, num_cus);
  if (P.options & kRegPrefix) return launch_rs<8192, CS, HASH, 3>(P, stream, num_cus);
  // unshifted windows of mid-sized frames (VXLAN's 128 B): the aligned-chunk transport checksum
  // and the inner Ethernet bytes from registers (fast_decode AL); shifted windows (pcap records,
  // 65..96-B slots) keep the plain kernel, where both cost ~1 % (measured A/B)
  // (every shipped kernel is compiled without the skeleton diagnostic's branch: round 4
  // measured config 4 -2.2 %, pcap64 -0.7 %; round 6 the 4 KiB kernels too)
  if (!(P.options & kShiftWindows)) return launch_rs<8192, CS, HASH, 3, false, false, false, true>(P, stream, num_cus);
  return launch_rs<8192, CS, HASH, 3, false, false>(P, stream, num_cus);
}

hipError_t launch_fast_rs(KParams &P, hipStream_t stream, int num_cus) {
  return dispatch_cs_hash(P, [&](auto cs, auto hash) {
    return launch_rs_for<decltype(cs)::value, decltype(hash)::value>(P, stream, num_cus);
  });
}

}  // namespace gpd

#ifdef GPD_PHASE_TIMING
extern "C" int gpd_diag_phase(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gpd::g_phase), 6 * sizeof(unsigned long long)) != hipSuccess)
    return -1;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(gpd::g_phase), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
