// gpd_ro.hip — ro_kernel, the round-based header-once loop of long frames, and its launch.
#include <hip/hip_runtime.h>

#include "gpd_dev_fast.h"
#include "gpd_dev_generic.h"
#include "gpd_launch.h"

namespace gpd {

// ro_kernel (gpd_tuning.header_once = 2): the header-once decode of long frames, with each
// 64-packet tile's bytes streamed as ONE contiguous run in rounds of 8 KiB — the traffic shape
// of the attainable probe — instead of windows cut at packet boundaries (IMIX: 3.35 windows of
// 6.8 KiB per 22.7-KiB tile, 21 % of each window's loads re-reading its first chunk).
//  * A packet's header (its first <= 128 bytes) is staged in the round that holds them; the
//    previous round's last 144 bytes stay in front of the window, so a header may straddle the
//    boundary.
//  * Its transport segment [S, E) is summed from the tile's running chunk prefix sums G: the
//    masked head chunk and G(A) where the header is staged, G(B) and the masked tail chunk in
//    the round that holds B (A = S rounded up, B = E rounded down to 16) — one compare per
//    pending lane per round until then.  So a segment may span any number of rounds, and a
//    packet larger than a window stays on the fast path.  An odd-aligned segment is summed in
//    the other byte order (RFC 1071 §2(B)) and swapped back.
//  * The straight-line decode runs once per tile from the staged headers (fast_decode<HO>).
//  * A tile whose packets do not lie nearly back to back (a shuffled or scattered layout: the
//    run much longer than its bytes) is left to the generic decoder whole.
constexpr uint32_t kRoStage = 8192;
constexpr uint32_t kRoCarry = 144;    // bytes of the previous round kept in front of the window
constexpr uint32_t kRoPfxCarry = 12;  // prefix words kept in front of the prefix array (9 used)
constexpr uint32_t kRoHdr = 128;      // header bytes a packet's staging (hdr_parse) reads at most
__host__ __device__ constexpr uint32_t ro_wave_lds_bytes() {
  return kRoCarry + kRoStage + 16u + 4u * kRoPfxCarry + 4u * (kRoStage / 16u + 1u) + 12u;
}
static_assert(ro_wave_lds_bytes() % 16u == 0u, "ro_kernel: 16-byte aligned wave regions");
static_assert(4 * ro_wave_lds_bytes() == 41856, "the workgroup LDS bytes gpd_launch.h pins launch_geom with");

template <bool CS, bool HASH, int MINW>
__global__ __launch_bounds__(256, MINW) void ro_kernel(KParams P) {
  constexpr int WAVES = 4;
  constexpr int NC = (int)kRoStage / 1024;  // 16-byte chunks per lane per round
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t k = threadIdx.x; k < P.image_words; k += 64 * WAVES)
    reinterpret_cast<uint32_t *>(g_lds)[k] = P.image[k];
  __syncthreads();
  const uint32_t img = (P.image_words * 4u + 15u) & ~15u;
  const uint32_t buf = img + wave * ro_wave_lds_bytes() + kRoCarry;  // the round's window
  const uint32_t pfx = buf + kRoStage + 16u + 4u * kRoPfxCarry;      // its chunk prefix sums P[0..512]
  const uint32_t n = P.n_dev ? min((uint32_t)P.n, *P.n_dev) : (uint32_t)P.n;
  const uint32_t ntiles = (n + 63u) >> 6;
  const uint32_t nwaves = gridDim.x * WAVES;
  const uint32_t dlen = (uint32_t)P.data_len;
  const uint32_t options = P.options & ~kDiagMask;
  const FastCtx F = fast_ctx(P, options);
  const bool vxreg = (P.decoders & GPD_DEC_VXLAN) != 0;

  uint32_t tp = blockIdx.x * WAVES + wave;  // the planner's tile
  const uint32_t gw = tp;  // this wave's fallback region (see rs_kernel)
  const uint32_t fb_start = 64u * (gw * (ntiles / nwaves) + min(gw, ntiles % nwaves));
  uint32_t fb_c = 0;
  if (tp >= ntiles) {
    if (lane == 0u) P.fb_wcount[gw] = 0u;
    return;
  }
  const TileDesc D{P, lane, n, ntiles, dlen};
  auto fb_list = [&](uint32_t i, uint32_t off, uint32_t fb) {  // the tile's leftovers: the fallback list
    fb_c = fb_append(P, fb_start, fb_c, i, off, fb);
  };
  // A tile's byte run [t0, t0 + 8192 nr): its packets' extent, in nr rounds; nr = 0 when the
  // packets are not nearly back to back (or hold no bytes): the tile goes to the fallback list.
  uint32_t t0_p = 0, t1_p = 0, nr_p = 0;
  auto tile_plan = [&](uint32_t valid, uint32_t off, uint32_t end) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(wave_min(valid ? (off & ~15u) : 0xFFFFFFFFu));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(wave_max(valid ? end : 0u));
    const uint32_t bytes = __builtin_amdgcn_readfirstlane(wave_sum(valid ? min(end - off, 1u << 24) : 0u));
    t0_p = lo;
    t1_p = hi;
    const uint32_t nr = (uint32_t)(((uint64_t)(hi - lo) + kRoStage - 1u) / kRoStage);
    // (a header's round is kept in 16 bits of the lane state: a run of more than 0xFFFF rounds,
    // 512 MiB, goes to the fallback list too)
    nr_p = (hi > lo && (uint64_t)(hi - lo) <= 2ull * bytes + kRoStage && nr <= 0xFFFFu) ? nr : 0u;
  };
  v4u32 wv[NC];
  auto rload = [&](uint32_t base, uint32_t nbytes) {  // one round's bytes into the registers
#pragma unroll
    for (int j = 0; j < NC; j++) {
      const uint32_t c = 1024u * j + 16u * lane;
      wv[j] = __builtin_nontemporal_load(reinterpret_cast<const v4u32 *>(P.data + base + (c < nbytes ? c : 0u)));
    }
    __builtin_amdgcn_sched_barrier(0);  // issue them here, ahead of the decode
  };

  // prologue: the first tile that has rounds (tiles without go to the fallback list whole)
  uint32_t o_a, c_a, o_b, c_b, off_p, end_p, valid_p;
  {
    uint32_t o0, c0;
    D.load(tp, o0, c0);
    D.load(tp + nwaves, o_a, c_a);
    D.load(tp + 2u * nwaves, o_b, c_b);
    valid_p = D.read(tp, o0, c0, off_p, end_p);
  }
  tile_plan(valid_p, off_p, end_p);
  bool any = true;
  while (nr_p == 0u) {
    fb_list(tp * 64u + lane, off_p, valid_p);
    if (tp + nwaves >= ntiles) { any = false; break; }
    tp += nwaves;
    valid_p = D.read(tp, o_a, c_a, off_p, end_p);
    o_a = o_b;
    c_a = c_b;
    D.load(tp + 2u * nwaves, o_b, c_b);
    tile_plan(valid_p, off_p, end_p);
  }
  if (any) {
    uint32_t rp = 0;  // the planner's round of tile tp
    rload(t0_p, min(kRoStage, ((t1_p - t0_p) + 15u) & ~15u));
    // decode state: round rd of tile td (its run from t0_d, nr_d rounds)
    uint32_t td = tp, t0_d = t0_p, nr_d = nr_p, rd = 0;
    uint32_t off_d = off_p, end_d = end_p;
    uint32_t base = 0;  // G at the round's start: the sum of the tile's earlier rounds' chunks
    // per lane, packed (registers bound the waves per SIMD): ls = its header's round (bits 0-15)
    // | staged | tail pending | odd segment start | fallback | tail bytes (20-23) | valid (24);
    // tB: the pending tail's B (tile-relative); part: the segment's partial sum
    constexpr uint32_t kStaged = 1u << 16, kPend = 1u << 17, kOdd = 1u << 18, kFb = 1u << 19, kValid = 1u << 24;
    uint32_t ls = valid_p ? kValid : 0u, tB = 0, part = 0;
    Hdr hh;  // (written where the header is staged; read only for a staged lane)
    for (;;) {
      // ---- the previous round's last bytes and prefix words in front of this round's
      if (rd > 0u) {
        if (lane < 9u) {
          const v4u32 q = *reinterpret_cast<const v4u32 *>(g_lds + buf + kRoStage - 144u + 16u * lane);
          const uint32_t pc = lds_u32(pfx + 4u * (503u + lane)) - lds_u32(pfx + 4u * 512u);
          *reinterpret_cast<v4u32 *>(g_lds + buf - 144u + 16u * lane) = q;
          *reinterpret_cast<uint32_t *>(g_lds + pfx - 36u + 4u * lane) = pc;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      // ---- commit round rd: registers -> LDS, and its chunk prefix sums from the registers
      {
        uint32_t cs[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) {
          *reinterpret_cast<v4u32 *>(g_lds + buf + 1024u * j + 16u * lane) = wv[j];
          cs[j] = dot2(wv[j].w, 0x00010001u, dot2(wv[j].z, 0x00010001u,
                       dot2(wv[j].y, 0x00010001u, dot2(wv[j].x, 0x00010001u, 0u))));
        }
        rows_prefix<NC>(cs, pfx, lane);
      }
      // ---- plan and load the next round (the rest of this tile, or the next tile with rounds)
      bool has_next = false, new_tile = false;
      if (rp + 1u < nr_p) {
        rp++;
        has_next = true;
      } else {
        while (tp + nwaves < ntiles) {
          tp += nwaves;
          valid_p = D.read(tp, o_a, c_a, off_p, end_p);
          o_a = o_b;
          c_a = c_b;
          D.load(tp + 2u * nwaves, o_b, c_b);
          tile_plan(valid_p, off_p, end_p);
          if (nr_p) {
            rp = 0;
            has_next = new_tile = true;
            break;
          }
          fb_list(tp * 64u + lane, off_p, valid_p);
        }
      }
      if (has_next) {
        const uint32_t rb = t0_p + kRoStage * rp;
        rload(rb, min(kRoStage, (t1_p - rb + 15u) & ~15u));
      }
      // ---- round rd of tile td
      const uint32_t R0 = t0_d + kRoStage * rd;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the committed round is readable)
      if (rd == 0u && (ls & kValid)) {
        const uint32_t need = max(min(off_d + kRoHdr, end_d), off_d + 1u);
        ls = kValid | ((need - 1u - t0_d) / kRoStage);
      }
      const bool here = (ls & kValid) && (ls & 0xFFFFu) == rd;
      if (here) {  // stage the header; the segment's head, and its tail if in this round
        const uint32_t pl = buf + off_d - R0;  // (>= buf - 128: the carry)
        uint32_t l4 = 0, seg = 0;
        ls |= kStaged;
        if (hdr_parse(pl, end_d - off_d, hh, F, vxreg, l4, seg) && CS) {
          const uint32_t S = pl + l4, E = S + seg, A = (S + 15u) & ~15u, B = E & ~15u;
          ls |= (S & 1u) ? kOdd : 0u;
          if (E <= A) {  // the whole segment inside its first chunk
            part = (A > S) ? chunk_part(A - 16u, S & 15u, E - (A - 16u), 0u) : 0u;
          } else {
            part = (A > S) ? chunk_part(A - 16u, S & 15u, 16u, 0u) : 0u;
            part -= base + lds_u32(pfx + 4u * (uint32_t)((int32_t)(A - buf) >> 4));
            if (E > B ? B < buf + kRoStage : B <= buf + kRoStage) {
              // (B may lie in the carry, in front of buf: a frame whose header round is set by
              // its 128 header bytes while its segment ends before the round, e.g. a short IP
              // packet in a long frame)
              part += base + lds_u32(pfx + 4u * (uint32_t)((int32_t)(B - buf) >> 4));
              if (E > B) part = chunk_part(B, 0u, E - B, part);
            } else {
              ls |= kPend | ((E - B) << 20);
              tB = B - buf + R0 - t0_d;
            }
          }
        }
        // VXLAN frames (their inner headers are not staged) take the generic decoder: a second
        // straight-line decode in the loop would cost the kernel its third wave per SIMD
        if (hh.ok == 2u) ls |= kFb;
      } else if (ls & kPend) {  // a segment's tail in this round?
        const uint32_t rel = tB - (R0 - t0_d), tl = (ls >> 20) & 15u;
        if (tl ? rel < kRoStage : rel <= kRoStage) {
          part += base + lds_u32(pfx + 4u * (rel >> 4));
          if (tl) part = chunk_part(buf + rel, 0u, tl, part);
          ls &= ~kPend;
        }
      }
      base += lds_u32(pfx + 4u * 512u);
      // ---- the tile is complete after its last round: one decode from the staged headers
      if (rd + 1u == nr_d) {
        Out res;
        uint32_t fb = 0;
        if ((ls & (kStaged | kPend | kFb)) == kStaged) {
          // an odd-aligned segment's sum is in the other byte order: folded and swapped back
          const uint32_t f1 = (part >> 16) + (part & 0xFFFFu), f2 = (f1 >> 16) + (f1 & 0xFFFFu);
          hh.sum = (ls & kOdd) ? __builtin_amdgcn_perm(0u, f2, 0x0C0C0001u) : part;
          Seg none{0, 0, 0};
          if (!fast_decode<CS, HASH, true, true>(0u, end_d - off_d, F, res, buf, none, &hh)) fb = 1;
        } else {
          fb = 1;
        }
        const uint32_t i = td * 64u + lane;
        const uint32_t valid = (ls & kValid) ? 1u : 0u;
        fb_list(i, off_d, valid ? fb : 0u);
        if (valid && !fb) store_out(P, i, res);
      }
      if (!has_next) break;
      if (new_tile) {
        td = tp;
        t0_d = t0_p;
        nr_d = nr_p;
        rd = 0;
        off_d = off_p;
        end_d = end_p;
        ls = valid_p ? kValid : 0u;
        base = 0;
      } else {
        rd++;
      }
    }
  }
  if (lane == 0u) P.fb_wcount[gw] = fb_c;  // (gpd_last_launch_split's count)
  decode_fallback_list<kRoStage / 64u, CS, HASH>(P, buf, fb_start, fb_c, lane, dlen, options);
}

// Three workgroups of four waves per CU (ro_kernel's register bound, and what LDS admits; fewer
// under gpd_tuning.waves_per_simd), four rounds of them by default.
hipError_t launch_fast_ro(KParams &P, hipStream_t stream, int num_cus) {
  const LaunchGeom g = launch_geom(P.image_words, 4 * (size_t)ro_wave_lds_bytes(), 4, 4, 3, P.waves,
                                   P.rounds ? P.rounds : kGridRounds, num_cus, (P.n + 63) / 64);
  return dispatch_cs_hash(P, [&](auto cs, auto hash) {
    return launch_kernel(ro_kernel<decltype(cs)::value, decltype(hash)::value, 3>, 256, g, P, stream, num_cus);
  });
}

}  // namespace gpd

