// gpd_launch.h — host side of the decode kernels' translation units: the launch geometry every
// kernel family shares, the launch itself, and the CS / HASH dispatch of the fast families.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "gpd_internal.h"

namespace gpd {

constexpr uint64_t kGridRounds = 4;         // a launch covers at most 4 rounds of resident workgroups
constexpr uint32_t kLdsPerCU = 160u * 1024u;
constexpr uint32_t kNoResidencyCap = ~0u;   // residency bounded by LDS alone

struct LaunchGeom {
  size_t lds;         // dynamic LDS bytes per workgroup
  uint64_t blocks;    // workgroups
  uint32_t fb_waves;  // waves that own a fallback region (KParams::fb_waves)
};

// image_words: the dispatch-table image in front of the workgroup's wg_lds bytes (plus 64 of
// slack).  A workgroup takes wg_tiles tiles per grid step and holds wg_fb_waves waves that own a
// fallback region.  At most max_wgs workgroups are resident per CU, fewer when LDS admits fewer.
// waves_per_simd (gpd_tuning.waves_per_simd, 0: unset) replaces that cap and enforces it by
// reserving 1/W of the CU's LDS per workgroup, rounded down to the 2,048-byte allocation granule
// (3 x 54,608 B do not fit; the kernel's registers alone would admit more).  The grid is capped at
// `rounds` rounds of resident workgroups.
constexpr LaunchGeom launch_geom(uint32_t image_words, size_t wg_lds, uint32_t wg_tiles, uint32_t wg_fb_waves,
                                 uint32_t max_wgs, uint32_t waves_per_simd, uint64_t rounds, int num_cus,
                                 uint64_t ntiles) {
  size_t lds = ((image_words * 4u + 15u) & ~15u) + wg_lds + 64;
  if (waves_per_simd) {
    lds = std::max<size_t>(lds, (kLdsPerCU / waves_per_simd) & ~(size_t)2047u);
    max_wgs = waves_per_simd;
  }
  const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(kLdsPerCU / lds, max_wgs));
  const uint64_t blocks = std::min<uint64_t>((ntiles + wg_tiles - 1) / wg_tiles, (uint64_t)num_cus * per_cu * rounds);
  return LaunchGeom{lds, blocks, (uint32_t)blocks * wg_fb_waves};
}

// The parent formulas' values for 256 CUs and the fixed-layout image (kFixWords = 672 words), at
// n = 2^24 packets (262,144 tiles) and at 4,096 packets (64 tiles: the grid cap does not bind).
// Workgroup LDS bytes are each family's (its translation unit asserts the figure used here).
namespace geom_check {
constexpr bool eq(LaunchGeom g, size_t lds, uint64_t blocks, uint32_t fb_waves) {
  return g.lds == lds && g.blocks == blocks && g.fb_waves == fb_waves;
}
constexpr uint64_t kBig = (1ull << 24) / 64, kSmall = 64;
// rs_kernel<4096>: 4 waves x 4,112 B; 4 workgroups per CU by its register bound; 4 rounds
static_assert(eq(launch_geom(672, 16448, 4, 4, 4, 0, 4, 256, kBig), 19200, 4096, 16384), "rs-4096 default");
static_assert(eq(launch_geom(672, 16448, 4, 4, 4, 2, 4, 256, kBig), 81920, 2048, 8192), "rs-4096 waves = 2");
static_assert(eq(launch_geom(672, 16448, 4, 4, 4, 0, 8, 256, kBig), 19200, 8192, 32768), "rs-4096 rounds = 8");
static_assert(eq(launch_geom(672, 16448, 4, 4, 4, 0, 4, 256, kSmall), 19200, 16, 64), "rs-4096 small batch");
// rs_kernel<8192>: 4 x 10,272 B; 3 per CU; 4 rounds (1 for the AL instance)
static_assert(eq(launch_geom(672, 41088, 4, 4, 3, 0, 4, 256, kBig), 43840, 3072, 12288), "rs-8192 default");
static_assert(eq(launch_geom(672, 41088, 4, 4, 3, 0, 1, 256, kBig), 43840, 768, 3072), "rs-8192 AL default");
static_assert(eq(launch_geom(672, 41088, 4, 4, 3, 2, 4, 256, kBig), 81920, 2048, 8192), "rs-8192 waves = 2");
static_assert(eq(launch_geom(672, 41088, 4, 4, 3, 3, 4, 256, kBig), 53248, 3072, 12288), "rs-8192 waves = 3");
static_assert(eq(launch_geom(672, 41088, 4, 4, 3, 0, 8, 256, kBig), 43840, 6144, 24576), "rs-8192 rounds = 8");
static_assert(eq(launch_geom(672, 41088, 4, 4, 3, 0, 4, 256, kSmall), 43840, 16, 64), "rs-8192 small batch");
// ro_kernel: 4 x 10,464 B; 3 per CU; 4 rounds
static_assert(eq(launch_geom(672, 41856, 4, 4, 3, 0, 4, 256, kBig), 44608, 3072, 12288), "ro default");
static_assert(eq(launch_geom(672, 41856, 4, 4, 3, 2, 4, 256, kBig), 81920, 2048, 8192), "ro waves = 2");
static_assert(eq(launch_geom(672, 41856, 4, 4, 3, 0, 8, 256, kBig), 44608, 6144, 24576), "ro rounds = 8");
static_assert(eq(launch_geom(672, 41856, 4, 4, 3, 0, 4, 256, kSmall), 44608, 16, 64), "ro small batch");
// sp_kernel: one 57,136-B ring; 2 per CU; a block per tile, 7 decoder waves each; one round;
// waves_per_simd is not passed on (its `waves = 2` launch is the default one)
static_assert(eq(launch_geom(672, 57136, 1, 7, 2, 0, 1, 256, kBig), 59888, 512, 3584), "sp default, waves = 2");
static_assert(eq(launch_geom(672, 57136, 1, 7, 2, 0, 8, 256, kBig), 59888, 4096, 28672), "sp rounds = 8");
static_assert(eq(launch_geom(672, 57136, 1, 7, 2, 0, 1, 256, kSmall), 59888, 64, 448), "sp small batch");
// decode_kernel: 4 x 9,216 B (4 KiB windows) or 4 x 17,408 B (8 KiB); what LDS admits; always 4
// rounds and no waves_per_simd (its `waves = 2` and `rounds = 8` launches are the default one);
// no fallback regions
static_assert(eq(launch_geom(672, 36864, 4, 0, kNoResidencyCap, 0, 4, 256, kBig), 39616, 4096, 0), "generic 4096");
static_assert(eq(launch_geom(672, 69632, 4, 0, kNoResidencyCap, 0, 4, 256, kBig), 72384, 2048, 0), "generic 8192");
static_assert(eq(launch_geom(672, 36864, 4, 0, kNoResidencyCap, 0, 4, 256, kSmall), 39616, 16, 0), "generic small batch");
}  // namespace geom_check

// Launch `kernel` over the geometry g with `threads` threads per workgroup; P.fb_waves is set
// whether or not anything is launched.
template <class K>
hipError_t launch_kernel(K kernel, unsigned threads, const LaunchGeom &g, KParams &P, hipStream_t stream, int num_cus) {
  P.fb_waves = g.fb_waves;
  if (g.blocks == 0) return hipSuccess;
  if (g.fb_waves > (uint32_t)num_cus * kMaxFastWavesPerCU) return hipErrorInvalidValue;  // (sizes fb_wcount)
  hipLaunchKernelGGL(kernel, dim3((unsigned)g.blocks), dim3(threads), g.lds, stream, P);
  return hipGetLastError();
}

// f(cs, hash) with the fused checksums / flow hashes requested by P's options as constants.
template <class F>
hipError_t dispatch_cs_hash(const KParams &P, F f) {
  const bool cs = !(P.options & GPD_OPT_NO_CHECKSUMS), hash = !(P.options & GPD_OPT_NO_FLOW_HASH);
  return cs ? (hash ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{}))
            : (hash ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{}));
}

}  // namespace gpd
