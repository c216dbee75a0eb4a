// gpd_runtime.cpp — host runtime behind the C-ABI in include/gpd.h.
//
// Owns the per-(thread, GPU) context: the snapshot of the dispatch tables in
// device memory (the reference reads mutable package globals on every packet,
// layers/enums.go:288-345, layers/ports.go:62-128; a context freezes them at
// creation like a parser built from them), the registered-decoder mask and
// options (parser.go:182-195, 336-350), HIP timing events, and the decode launch.  The
// context itself is defined in gpd_ctx.h; its staging slots and gpd_decode_host live in
// gpd_staging.cpp, the capture pipelines in gpd_capture.cpp.
#include <hip/hip_runtime.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cerrno>

#include "gpd_ctx.h"

using gpd::set_error;

static thread_local char g_err[512] = "";

int gpd::set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

namespace {

// Reference defaults, restated as data: layers/enums.go:304-345, layers/ports.go:62-74,105-122.
const uint32_t kEtherDefaults[][2] = {
    {0x0000, 22}, {0x0800, 20}, {0x86DD, 21}, {0x0806, 10}, {0x8100, 15}, {0x880B, 25},
    {0x8863, 26}, {0x8864, 26}, {0x9000, 12}, {0x2000, 11}, {0x01A2, 61}, {0x88CC, 58},
    {0x8847, 24}, {0x8848, 24}, {0x888E, 56}, {0x88A8, 15}, {0x6558, 17}, {0x88BE, 145}};
const uint32_t kProtoDefaults[][2] = {
    {4, 20},  {6, 44},  {17, 45}, {1, 19},  {58, 57},  {132, 28}, {41, 21}, {94, 20},
    {97, 16}, {27, 27}, {47, 18}, {0, 46},  {43, 47},  {44, 48},  {60, 49}, {89, 123},
    {51, 50}, {50, 51}, {136, 52}, {137, 24}, {59, 2}, {2, 62}, {112, 119}};
const uint32_t kTcpDefaults[][2] = {{53, 107}, {443, 140}, {502, 141}, {636, 140},
                                    {989, 140}, {990, 140}, {992, 140}, {993, 140},
                                    {994, 140}, {995, 140}, {5061, 140}};
const uint32_t kUdpDefaults[][2] = {{53, 107},   {123, 117},  {4789, 116}, {67, 118},
                                    {68, 118},   {546, 134},  {547, 134},  {666, 147},
                                    {1000, 149}, {5060, 133}, {6343, 114}, {6081, 120},
                                    {3784, 122}, {2152, 129}, {623, 142},  {1812, 146}};

template <size_t N>
void fill(uint16_t *t, size_t size, const uint32_t (&e)[N][2]) {
  memset(t, 0, size * sizeof(uint16_t));
  for (size_t k = 0; k < N; k++) t[e[k][0]] = (uint16_t)e[k][1];
}

// Two-level page encoding of the three 64K tables (see gpd_internal.h).
std::vector<uint16_t> encode_tables(const uint16_t *eth, const uint16_t *proto,
                                    const uint16_t *tcp, const uint16_t *udp) {
  std::vector<uint16_t> out(gpd::kTabPages + 256, 0);  // page 0 = zeros
  std::memcpy(out.data() + gpd::kTabIpProto, proto, 256 * sizeof(uint16_t));
  std::map<std::vector<uint16_t>, uint16_t> pages;
  pages[std::vector<uint16_t>(256, 0)] = 0;
  auto encode = [&](const uint16_t *t, uint32_t dir) {
    for (uint32_t hi = 0; hi < 256; hi++) {
      std::vector<uint16_t> pg(t + hi * 256, t + hi * 256 + 256);
      auto it = pages.find(pg);
      uint16_t idx;
      if (it == pages.end()) {
        idx = (uint16_t)pages.size();
        pages[pg] = idx;
        out.insert(out.end(), pg.begin(), pg.end());
      } else {
        idx = it->second;
      }
      out[dir + hi] = idx;
    }
  };
  encode(eth, gpd::kTabEthDir);
  encode(tcp, gpd::kTabTcpDir);
  encode(udp, gpd::kTabUdpDir);
  return out;
}

// Decoder id per LayerType for the registered set (the DecodingLayerMap of parser.go:147-164,
// filled from each decoder's CanDecode, layertypes.go:193-198 for the extension class) and
// the 4-bit code the `layers` word uses for it (include/gpd.h GPD_C_*).
void type_lut(uint32_t decoders, uint8_t lut[128]) {
  struct E { uint32_t lt, dec, code; };
  static const E kMap[] = {{17, 0, 1},  {15, 1, 2},  {20, 2, 3},  {21, 3, 4},  {46, 4, 5},
                           {47, 4, 6},  {48, 4, 7},  {49, 4, 8},  {44, 5, 9},  {45, 6, 10},
                           {116, 7, 11}, {2, 8, 12}, {3, 9, 13}, {19, 10, 14}, {22, 11, 15}};
  memset(lut, 0xFF, 128);
  for (const E &e : kMap)
    if (decoders & (1u << e.dec)) lut[e.lt] = (uint8_t)(e.dec | (e.code << 4));
}

// Two-way bucketed hash of the nonzero entries of a 64K table: 2^bits buckets of two u32
// slots {key << 16 | LayerType << 8 | lut[LayerType]}, bucket = key_hash(key, mult, bits).
// The multiplier is searched so that no bucket holds more than two keys, which makes every
// device lookup one ds_read_b64 and two compares (no probe loop).  Unused slots hold a key
// absent from the table with "LayerType 0, not registered", so they read as a miss.
struct HashKeys {
  std::vector<uint32_t> keys;
  uint32_t empty = 0;
  bool ok = false;  // every LayerType < 256 and some key absent
};
HashKeys hash_keys(const uint16_t *t) {
  HashKeys h;
  std::vector<uint8_t> present(65536, 0);
  for (uint32_t k = 0; k < 65536; k++) {
    if (t[k] >= 256) return h;
    if (t[k]) { h.keys.push_back(k); present[k] = 1; }
  }
  uint32_t absent = 0;
  while (absent < 65536 && present[absent]) absent++;
  if (absent == 65536) return h;
  h.empty = (absent << 16) | 0xFFu;
  h.ok = true;
  return h;
}
bool fill_hash(const HashKeys &h, const uint16_t *t, const uint8_t lut[128], uint32_t mult,
               uint32_t bits, std::vector<uint32_t> &slots) {
  const uint32_t nb = 1u << bits;
  if (h.keys.size() > 2 * nb) return false;
  slots.assign(2 * nb, h.empty);
  std::vector<uint8_t> fill(nb, 0);
  for (uint32_t k : h.keys) {
    const uint32_t b = gpd::key_hash(k, mult, bits);
    if (fill[b] == 2) return false;
    slots[2 * b + fill[b]++] = (k << 16) | ((uint32_t)t[k] << 8) | (t[k] < 128 ? lut[t[k]] : 0xFFu);
  }
  return true;
}
uint32_t next_mult(uint32_t m) { return ((m * 2654435761u + 0x9E37u) & 0xFFFFu) | 1u; }

// Any layout: the smallest bits (<= max_words) with some multiplier.
bool build_hash(const uint16_t *t, const uint8_t lut[128], uint32_t max_words,
                std::vector<uint32_t> &slots, uint32_t &mult_out, uint32_t &bits_out) {
  const HashKeys h = hash_keys(t);
  if (!h.ok) return false;
  for (uint32_t bits = 2; bits <= 15 && (2u << bits) <= max_words; bits++) {
    uint32_t mult = 40503u;  // golden-ratio start, then a fixed odd sequence
    for (int attempt = 0; attempt < 512; attempt++, mult = next_mult(mult)) {
      if (fill_hash(h, t, lut, mult, bits, slots)) {
        mult_out = mult;
        bits_out = bits;
        return true;
      }
    }
  }
  return false;
}

// The fixed layout the fast kernel compiles in (gpd_internal.h kFix*): 2^kFixBits buckets
// per table at fixed bases, one multiplier shared by the three tables.
bool build_fixed(const uint16_t *eth, const uint16_t *tcp, const uint16_t *udp,
                 const uint8_t lut[128], std::vector<uint32_t> &he, std::vector<uint32_t> &ht,
                 std::vector<uint32_t> &hu, uint32_t &mult_out) {
  const HashKeys ke = hash_keys(eth), kt = hash_keys(tcp), ku = hash_keys(udp);
  if (!ke.ok || !kt.ok || !ku.ok) return false;
  uint32_t mult = 40503u;
  for (int attempt = 0; attempt < 4096; attempt++, mult = next_mult(mult)) {
    if (fill_hash(ke, eth, lut, mult, gpd::kFixBits, he) &&
        fill_hash(kt, tcp, lut, mult, gpd::kFixBits, ht) &&
        fill_hash(ku, udp, lut, mult, gpd::kFixBits, hu)) {
      mult_out = mult;
      return true;
    }
  }
  return false;
}

}  // namespace

namespace gpd {
int ctx_device(const gpd_ctx *ctx) { return ctx->device; }
int ctx_num_cus(const gpd_ctx *ctx) { return ctx->num_cus; }
void *ctx_scratch(gpd_ctx *ctx, int slot, size_t bytes) {
  if (slot < 0 || slot >= (int)(sizeof ctx->scratch / sizeof ctx->scratch[0])) return nullptr;
  auto &sc = ctx->scratch[slot];
  if (sc.bytes < bytes) {
    if (sc.d) (void)hipFree(sc.d);
    sc.d = nullptr;
    sc.bytes = 0;
    const size_t want = bytes + bytes / 4;  // headroom: a slightly larger walk reuses it
    if (hipMalloc(&sc.d, want) != hipSuccess) return nullptr;
    sc.bytes = want;
  }
  return sc.d;
}
}  // namespace gpd

extern "C" {

int gpd_abi_version(void) { return GPD_ABI_VERSION; }

const char *gpd_last_error_string(void) { return g_err; }

void gpd_default_tables(uint16_t *ethertype, uint16_t *ipproto, uint16_t *tcp_port,
                        uint16_t *udp_port) {
  if (ethertype) fill(ethertype, 65536, kEtherDefaults);
  if (ipproto) fill(ipproto, 256, kProtoDefaults);
  if (tcp_port) fill(tcp_port, 65536, kTcpDefaults);
  if (udp_port) fill(udp_port, 65536, kUdpDefaults);
}

// Builds the dispatch image (and the PAGES blob) of `decoders` over the given tables into new
// device buffers; only when every step succeeded are they swapped into ctx (the old ones
// freed), so a failed rebuild leaves the context exactly as it was.  The callers
// commit their decoder mask / table snapshot after a GPD_OK only.
static int build_image(gpd_ctx *ctx, uint32_t decoders, const std::vector<uint16_t> &eth,
                       const std::vector<uint16_t> &proto, const std::vector<uint16_t> &tcp,
                       const std::vector<uint16_t> &udp) {
  // LDS image: LUT (32 words) + ipproto with LUT entries (256 words) + the three hashes
  std::vector<uint32_t> img(gpd::kHashLutWords + gpd::kHashProtoWords, 0);
  uint8_t *lut = reinterpret_cast<uint8_t *>(img.data());
  type_lut(decoders, lut);
  for (uint32_t p = 0; p < 256; p++) {
    const uint32_t lt = proto[p];
    img[gpd::kHashLutWords + p] = lt | ((lt < 128 ? lut[lt] : 0xFFu) << 16);
  }
  std::vector<uint32_t> he, ht, hu;
  const uint32_t room = gpd::kHashMaxWords - (uint32_t)img.size();
  uint32_t me = 0, mt = 0, mu = 0, be = 0, bt = 0, bu = 0;
  const bool fixed = build_fixed(eth.data(), tcp.data(), udp.data(), lut, he, ht, hu, me);
  bool hashed = fixed;
  if (fixed) {
    mt = mu = me;
    be = bt = bu = gpd::kFixBits;
  } else {
    hashed = build_hash(eth.data(), lut, room / 2, he, me, be) &&
             build_hash(tcp.data(), lut, room / 4, ht, mt, bt) &&
             build_hash(udp.data(), lut, room / 4, hu, mu, bu);
  }
  uint32_t eth_base = 0, tcp_base = 0, udp_base = 0;
  std::vector<uint16_t> blob;
  if (hashed) {  // every hash starts on an 8-byte boundary (ds_read_b64 buckets)
    auto put = [&](const std::vector<uint32_t> &h, uint32_t &base) {
      if (img.size() & 1) img.push_back(0);
      base = (uint32_t)img.size();
      img.insert(img.end(), h.begin(), h.end());
    };
    put(he, eth_base);
    put(ht, tcp_base);
    put(hu, udp_base);
    if (fixed && (eth_base != gpd::kFixEthBase || tcp_base != gpd::kFixTcpBase || udp_base != gpd::kFixUdpBase))
      return set_error(GPD_ERR_INVALID, "internal: fixed table layout mismatch");
  } else {
    blob = encode_tables(eth.data(), proto.data(), tcp.data(), udp.data());
  }
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  uint32_t *d_image = nullptr;
  uint16_t *d_pages = nullptr;
  hipError_t e = hipMalloc(&d_image, img.size() * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(d_image, img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess && !hashed) e = hipMalloc(&d_pages, blob.size() * sizeof(uint16_t));
  if (e == hipSuccess && !hashed)
    e = hipMemcpy(d_pages, blob.data(), blob.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d_image) (void)hipFree(d_image);
    if (d_pages) (void)hipFree(d_pages);
    return set_error(e == hipErrorOutOfMemory ? GPD_ERR_NOMEM : GPD_ERR_HIP, "dispatch image: %s",
                   hipGetErrorString(e));
  }
  if (ctx->d_image) (void)hipFree(ctx->d_image);
  if (ctx->d_pages) (void)hipFree(ctx->d_pages);
  ctx->d_image = d_image;
  ctx->d_pages = d_pages;
  ctx->image_words = (uint32_t)img.size();
  ctx->fixed = fixed;
  ctx->use_pages = hashed ? 0 : 1;
  if (hashed) {
    ctx->eth_base = eth_base; ctx->eth_bits = be; ctx->eth_mult = me;
    ctx->tcp_base = tcp_base; ctx->tcp_bits = bt; ctx->tcp_mult = mt;
    ctx->udp_base = udp_base; ctx->udp_bits = bu; ctx->udp_mult = mu;
  }
  return GPD_OK;
}

int gpd_ctx_reload_tables(gpd_ctx *ctx, const gpd_config *cfg) {
  if (!ctx || !cfg) return set_error(GPD_ERR_INVALID, "gpd_ctx_reload_tables: null argument");
  std::vector<uint16_t> eth(65536, 0), proto(256, 0), tcp(65536, 0), udp(65536, 0);
  gpd_default_tables(eth.data(), proto.data(), tcp.data(), udp.data());
  if (cfg->ethertype) std::memcpy(eth.data(), cfg->ethertype, 65536 * 2);
  if (cfg->ipproto) std::memcpy(proto.data(), cfg->ipproto, 256 * 2);
  if (cfg->tcp_port) std::memcpy(tcp.data(), cfg->tcp_port, 65536 * 2);
  if (cfg->udp_port) std::memcpy(udp.data(), cfg->udp_port, 65536 * 2);
  const int rc = build_image(ctx, ctx->decoders, eth, proto, tcp, udp);
  if (rc != GPD_OK) return rc;  // the context keeps its previous snapshot and image
  ctx->t_eth.swap(eth);
  ctx->t_proto.swap(proto);
  ctx->t_tcp.swap(tcp);
  ctx->t_udp.swap(udp);
  return GPD_OK;
}

// Options the caller may set: the reference's two fields and the engine knobs (bits 24-29
// are the runtime's own launch flags).  The diagnostic library (libgpd_diag.so, -DGPD_DIAG)
// also takes bench.py's two ablation bits (30: no DMA wait, 31: no decode), which give wrong
// results by design; the shipped libgpd.so refuses them like any unknown bit (gpd.h).
#ifdef GPD_DIAG
static constexpr uint32_t kDiagOptions = (1u << 30) | (1u << 31);
#else
static constexpr uint32_t kDiagOptions = 0;
#endif
static constexpr uint32_t kUserOptions = GPD_OPT_IGNORE_UNSUPPORTED | GPD_OPT_IGNORE_PANIC |
                                         GPD_OPT_NO_CHECKSUMS | GPD_OPT_NO_FLOW_HASH | kDiagOptions;

int gpd_ctx_set_options(gpd_ctx *ctx, uint32_t options) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_ctx_set_options: ctx is NULL");
  if (options & ~kUserOptions)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_set_options: unknown option bits 0x%x",
                   options & ~kUserOptions);
  ctx->options = options;
  return GPD_OK;
}

int gpd_ctx_set_decoders(gpd_ctx *ctx, uint32_t decoders) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_ctx_set_decoders: ctx is NULL");
  if (decoders & ~GPD_DEC_ALL)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_set_decoders: unknown decoder bits 0x%x", decoders);
  if (decoders == ctx->decoders) return GPD_OK;
  const int rc = build_image(ctx, decoders, ctx->t_eth, ctx->t_proto, ctx->t_tcp, ctx->t_udp);
  if (rc == GPD_OK) ctx->decoders = decoders;  // a failed rebuild keeps the old mask and image
  return rc;
}

int gpd_ctx_add_decoders(gpd_ctx *ctx, uint32_t decoders) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_ctx_add_decoders: ctx is NULL");
  if (decoders & ~GPD_DEC_ALL)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_add_decoders: unknown decoder bits 0x%x", decoders);
  if ((ctx->decoders | decoders) == ctx->decoders) return GPD_OK;
  const uint32_t next = ctx->decoders | decoders;
  const int rc = build_image(ctx, next, ctx->t_eth, ctx->t_proto, ctx->t_tcp, ctx->t_udp);
  if (rc == GPD_OK) ctx->decoders = next;
  return rc;
}

int gpd_ctx_create(int device, const gpd_config *cfg, gpd_ctx **out) {
  if (!out) return set_error(GPD_ERR_INVALID, "gpd_ctx_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  const hipError_t dc = hipGetDeviceCount(&ndev);
  if (dc != hipSuccess || ndev == 0)
    return set_error(GPD_ERR_NODEVICE, "gpd_ctx_create: no HIP device available (%s, %d devices)",
                   hipGetErrorString(dc), ndev);
  if (device < 0 || device >= ndev)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_create: device %d out of range [0,%d)", device, ndev);
  gpd_config defaults{};
  defaults.first_layer = GPD_LT_ETHERNET;
  defaults.decoders = GPD_DEC_ALL;
  if (!cfg) cfg = &defaults;
  if (cfg->decoders & ~GPD_DEC_ALL)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_create: unknown decoder bits 0x%x", cfg->decoders);
  gpd_ctx *ctx = new gpd_ctx;
  ctx->device = device;
  ctx->first = cfg->first_layer;
  ctx->decoders = cfg->decoders;
  if (cfg->options & ~kUserOptions) {
    delete ctx;
    return set_error(GPD_ERR_INVALID, "gpd_ctx_create: unknown option bits 0x%x",
                   cfg->options & ~kUserOptions);
  }
  ctx->options = cfg->options;
  hipDeviceProp_t prop;
  gpd::DeviceScope dscope_;
  if (dscope_.set(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
    delete ctx;
    return set_error(GPD_ERR_HIP, "gpd_ctx_create: cannot query device %d", device);
  }
  ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  int rc = gpd_ctx_reload_tables(ctx, cfg);
  if (rc) {
    delete ctx;
    return rc;
  }
  *out = ctx;
  return GPD_OK;
}

int gpd_ctx_destroy(gpd_ctx *ctx) {
  if (!ctx) return GPD_OK;
  gpd::DeviceScope dscope_;
  (void)dscope_.set(ctx->device);
  gpd::free_slots(ctx);
  if (ctx->d_image) (void)hipFree(ctx->d_image);
  if (ctx->d_pages) (void)hipFree(ctx->d_pages);
  for (auto &kv : ctx->fallback) {
    if (kv.second.d) (void)hipFree(kv.second.d);
    if (kv.second.wc) (void)hipFree(kv.second.wc);
  }
  for (auto &sc : ctx->scratch)
    if (sc.d) (void)hipFree(sc.d);
  for (const auto &r : ctx->registered) (void)hipHostUnregister((void *)r.first);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->evm) (void)hipEventDestroy(ctx->evm);
  delete ctx;
  return GPD_OK;
}

int gpd_last_launch_split(gpd_ctx *ctx, uint64_t *fallback, float *fast_ms, float *list_ms) {
  if (!ctx || !fallback || !fast_ms || !list_ms)
    return set_error(GPD_ERR_INVALID, "gpd_last_launch_split: null argument");
  if (!ctx->timed || !ctx->timed_split)
    return set_error(GPD_ERR_INVALID, "gpd_last_launch_split: no timed fast-path launch "
                                    "(gpd_ctx_set_timing(1), then one gpd_decode of <= 2^30 packets)");
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventElapsedTime(fast_ms, ctx->ev0, ctx->evm));
  HIP_TRY(hipEventElapsedTime(list_ms, ctx->evm, ctx->ev1));
  // the launch's per-wave counts stay until the launch after next on the stream rewrites them
  std::vector<uint32_t> wc(ctx->timed_fb_waves);
  if (!wc.empty())
    HIP_TRY(hipMemcpy(wc.data(), ctx->timed_fb_wc, wc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint64_t c = 0;
  for (uint32_t v : wc) c += v;
  *fallback = c;
  return GPD_OK;
}

int gpd_ctx_set_tuning(gpd_ctx *ctx, const gpd_tuning *t) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_ctx_set_tuning: null ctx");
  const gpd_tuning automatic{0, -1, -1, 0, -1, -1, 0, -1};  // (waves_per_simd 0: automatic)
  if (!t) t = &automatic;
  if (t->window_bytes != 0 && t->window_bytes != 4096 && t->window_bytes != 8192)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_set_tuning: window_bytes %u (0, 4096 or 8192)", t->window_bytes);
  if (t->shift < -1 || t->shift > 1 || t->reg_prefix < -1 || t->reg_prefix > 1 || t->header_once < -1 ||
      t->header_once > 2 || t->device_walk < -1 || t->device_walk > 1)
    return set_error(GPD_ERR_INVALID,
                   "gpd_ctx_set_tuning: shift / reg_prefix / device_walk outside {-1, 0, 1}, header_once "
                   "outside {-1, 0, 1, 2}");
  if (t->waves_per_simd != 0 && (t->waves_per_simd < 2 || t->waves_per_simd > 4))
    return set_error(GPD_ERR_INVALID, "gpd_ctx_set_tuning: waves_per_simd %d (0, 2, 3 or 4)", t->waves_per_simd);
  if (t->grid_rounds < 0 || t->grid_rounds > 8)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_set_tuning: grid_rounds %d (0 .. 8)", t->grid_rounds);
  if (t->split < -1 || t->split > 1)
    return set_error(GPD_ERR_INVALID, "gpd_ctx_set_tuning: split %d (-1, 0 or 1)", t->split);
  ctx->tune = *t;
  return GPD_OK;
}

int gpd_ctx_set_timing(gpd_ctx *ctx, int enable) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_ctx_set_timing: null ctx");
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  if (enable && !ctx->ev0) {
    HIP_TRY(hipEventCreate(&ctx->ev0));
    HIP_TRY(hipEventCreate(&ctx->ev1));
    HIP_TRY(hipEventCreate(&ctx->evm));
  }
  ctx->timing = enable != 0;
  ctx->timed = false;
  return GPD_OK;
}

float gpd_last_kernel_ms(gpd_ctx *ctx) {
  if (!ctx || !ctx->timed) return -1.0f;
  float ms = -1.0f;
  if (hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0f;
  if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0f;
  return ms;
}

static int check_batch(const gpd_batch *in, const gpd_result *out) {
  if (!in || !out) return set_error(GPD_ERR_INVALID, "gpd_decode: null batch or result");
  if (in->n == 0) return GPD_OK;
  if (!in->data || !in->offset || !in->caplen)
    return set_error(GPD_ERR_INVALID, "gpd_decode: batch data/offset/caplen must be non-NULL");
  if (out->records) {
    if (out->status || out->layers || out->net_hash || out->tp_hash || out->csum)
      return set_error(GPD_ERR_INVALID, "gpd_decode: records excludes the status/layers/net_hash/tp_hash/csum arrays");
  } else if (!out->status || !out->layers) {
    return set_error(GPD_ERR_INVALID, "gpd_decode: result status/layers must be non-NULL");
  }
  if ((reinterpret_cast<uintptr_t>(in->data) & 15) != 0)
    return set_error(GPD_ERR_INVALID, "gpd_decode: data pointer must be 16-byte aligned");
  if (in->data_len > 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "gpd_decode: data_len %llu exceeds the 32-bit offset range",
                   (unsigned long long)in->data_len);
  if (in->n > gpd::kMaxBatchPackets)  // (packet and tile counts stay 32-bit in every kernel)
    return set_error(GPD_ERR_INVALID, "gpd_decode: batch of %llu packets (max 2^32 - 256)",
                   (unsigned long long)in->n);
  return GPD_OK;
}

}  // extern "C"

void gpd::ctx_fill_kparams(const gpd_ctx *ctx, KParams &P) {
  P.image = ctx->d_image;
  P.pages = ctx->d_pages;
  P.image_words = ctx->image_words;
  P.use_pages = ctx->use_pages;
  P.eth_base = ctx->eth_base; P.tcp_base = ctx->tcp_base; P.udp_base = ctx->udp_base;
  P.eth_bits = ctx->eth_bits; P.tcp_bits = ctx->tcp_bits; P.udp_bits = ctx->udp_bits;
  P.eth_mult = ctx->eth_mult; P.tcp_mult = ctx->tcp_mult; P.udp_mult = ctx->udp_mult;
  P.fixed = ctx->fixed;
  P.first = ctx->first;
  P.decoders = ctx->decoders;
  P.options = ctx->options;
}

int gpd::decode_launch(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *out, hipStream_t stream, bool record,
                       const uint32_t *n_dev, uint64_t geom_n, uint64_t geom_bytes) {
  gpd::KParams P{};
  P.data = in->data;
  P.data_len = in->data_len;
  P.offset = in->offset;
  P.caplen = in->caplen;
  P.n = in->n;
  P.n_dev = n_dev;
  res_to_kparams(P, *out);
  ctx_fill_kparams(ctx, P);
  // LDS window per buffer: the smallest of 4/8 KiB that holds a typical 64-packet tile
  const uint64_t gn = geom_n ? geom_n : in->n;
  const uint64_t mean_slot = ((geom_bytes ? geom_bytes : in->data_len) + gn - 1) / gn;
  P.stage = mean_slot * 64 <= 4096 ? 4096u : 8192u;
  if (ctx->tune.window_bytes) P.stage = ctx->tune.window_bytes;
  // streamed bytes and results use the nt cache policy (read once / written once)
  P.options |= 3u << 28;
  // Window copies shifted so that network headers sit 16-byte aligned in LDS, for batches of
  // small frames (mean slot <= 96 B: a window holds 40+ packets and the saved misaligned reads
  // outweigh the shifted copy; with IMIX-sized frames they do not).  gpd_ctx_set_tuning can
  // force either copy (the parity tests cover both).
  const bool shift = ctx->tune.shift >= 0 ? ctx->tune.shift != 0 : mean_slot <= 96;
  if (shift) P.options |= 1u << 27;
  // long frames (mean slot > 160 B): 8 KiB windows whose chunk prefix sums are computed from
  // the registers at commit
  if (ctx->tune.reg_prefix >= 0 ? ctx->tune.reg_prefix != 0 : (mean_slot > 160 && !shift))
    P.options |= 1u << 26;
  // ... whose 64-packet tiles span several windows: decoded once per tile from the headers the
  // windows stage (seg_pass), not once per window with the lanes each window holds — by default
  // over 8 KiB rounds of each tile's contiguous run (ro_kernel) rather than windows cut at packet
  // boundaries (IMIX 0.319 -> 0.296 ms, same box, profiles/r04/ro_ab/)
  const int ho = ctx->tune.header_once >= 0 ? ctx->tune.header_once : (mean_slot > 160 && !shift ? 2 : 0);
  if (P.stage == 8192 && ho == 1) P.options |= 1u << 25;
  if (ho == 2) P.options |= 1u << 24;
  P.waves = (uint32_t)ctx->tune.waves_per_simd;
  P.rounds = (uint32_t)ctx->tune.grid_rounds;
  // 4 KiB windows of small frames by the loader / decoder split kernel (automatic: on; config 2
  // 0.319 -> 0.297 ms, tcp64 0.321 -> 0.304, same box)
  P.split = ctx->tune.split >= 0 ? (uint32_t)ctx->tune.split : 1u;
  P.nstores = P.rec ? 2u + (P.hdr_off != nullptr)
                     : 2u + (P.net_hash != nullptr) + (P.tp_hash != nullptr) + (P.csum != nullptr) +
                           (P.hdr_off != nullptr);
  if (gpd::fast_eligible(P)) {  // fallback list scratch for this stream, sized for one launch
    const uint64_t need = std::min<uint64_t>(in->n, gpd::kMaxLaunchPackets);
    auto &fb = ctx->fallback[stream];
    if (fb.cap < need) {
      if (fb.d) {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipFree(fb.d));
        HIP_TRY(hipFree(fb.wc));
        fb.d = fb.wc = nullptr;
        fb.cap = 0;
      }
      // the list: 64 entries per tile (each wave's region spans its tiles), after the flags
      HIP_TRY(hipMalloc(&fb.d, 128 * sizeof(uint32_t) + (need + 64) * sizeof(uint64_t)));
      HIP_TRY(hipMemset(fb.d, 0, 128 * sizeof(uint32_t)));  // both flags start at zero
      HIP_TRY(hipMalloc(&fb.wc, 2ull * ctx->num_cus * gpd::kMaxFastWavesPerCU * sizeof(uint32_t)));
      fb.cap = need;
      fb.parity = 0;
    }
    P.fb_list = reinterpret_cast<uint64_t *>(fb.d + 128);
  }
  if (record) HIP_TRY(hipEventRecord(ctx->ev0, stream));
  const bool split = record && in->n <= gpd::kMaxLaunchPackets && gpd::fast_eligible(P);
  ctx->timed_split = false;
  // launches of <= kMaxLaunchPackets packets keep every packet/tile index 32-bit in the kernel
  for (uint64_t lo = 0; lo < in->n; lo += gpd::kMaxLaunchPackets) {
    gpd::KParams Q = P;
    Q.n = std::min<uint64_t>(gpd::kMaxLaunchPackets, in->n - lo);
    Q.offset = in->offset + lo;
    Q.caplen = in->caplen + lo;
    res_to_kparams(Q, shifted(out, lo));
    if (gpd::fast_eligible(P)) {  // per-wave counts, two arrays used alternately (a timed
      auto &fb = ctx->fallback[stream];  // launch's counts survive the next launch for the split)
      Q.fb_wcount = fb.wc + (size_t)ctx->num_cus * gpd::kMaxFastWavesPerCU * fb.parity;
      fb.parity ^= 1u;
    }
    uint32_t fbw = 0;
    hipError_t e = gpd::launch_decode(Q, stream, ctx->num_cus, split ? ctx->evm : nullptr, &fbw);
    if (e != hipSuccess) return set_error(GPD_ERR_HIP, "decode kernel launch: %s", hipGetErrorString(e));
    if (split) {
      ctx->timed_fb_wc = Q.fb_wcount;
      ctx->timed_fb_waves = fbw;
    }
  }
  if (record) {
    HIP_TRY(hipEventRecord(ctx->ev1, stream));
    ctx->timed = true;
    ctx->timed_split = split;
  }
  return GPD_OK;
}

extern "C" {

int gpd_decode(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *out, void *stream) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_decode: null ctx");
  int rc = check_batch(in, out);
  if (rc || in->n == 0) return rc;
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  return gpd::decode_launch(ctx, in, out, (hipStream_t)stream, ctx->timing);
}

int gpd_sync(gpd_ctx *ctx, void *stream) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_sync: null ctx");
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return GPD_OK;
}

// ---- IPv4 fragment hand-off (include/gpd_defrag.h) ----
int gpd_ip4_fragments(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res, gpd_ip4_frag *out,
                      uint64_t max_out, uint64_t *count, void *stream) {
  if (!ctx || !in || !res || !count) return set_error(GPD_ERR_INVALID, "gpd_ip4_fragments: null argument");
  *count = 0;
  if (in->n == 0) return GPD_OK;
  if (in->n > 0xFFFFFF00ull) return set_error(GPD_ERR_INVALID, "gpd_ip4_fragments: batch of %llu packets (max 2^32 - 256)",
                                            (unsigned long long)in->n);
  if (!in->data || !in->offset || !in->caplen)
    return set_error(GPD_ERR_INVALID, "gpd_ip4_fragments: batch data/offset/caplen must be non-NULL");
  if (!res->hdr_off || (!res->records && (!res->status || !res->layers)))
    return set_error(GPD_ERR_INVALID, "gpd_ip4_fragments: needs hdr_off and status + layers (or records)");
  if (max_out && !out) return set_error(GPD_ERR_INVALID, "gpd_ip4_fragments: null out with max_out > 0");
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  gpd::FragArgs A{};
  gpd::KParams &P = A.P;
  P.data = in->data;
  P.data_len = in->data_len;
  P.offset = in->offset;
  P.caplen = in->caplen;
  P.n = in->n;
  P.status = res->status;
  P.layers = res->layers;
  P.rec = res->records;
  P.hdr_off = res->hdr_off;
  gpd::ctx_fill_kparams(ctx, P);
  A.out = out;
  A.max_out = (uint32_t)std::min<uint64_t>(max_out, in->n);
  A.nblk = (uint32_t)((in->n + 2047) / 2048);
  A.blk = static_cast<uint32_t *>(gpd::ctx_scratch(ctx, 12, ((size_t)A.nblk + 1) * 4));
  A.idx = static_cast<uint32_t *>(gpd::ctx_scratch(ctx, 13, (size_t)in->n * 4));
  A.mask = static_cast<uint64_t *>(gpd::ctx_scratch(ctx, 14, ((size_t)in->n + 63) / 64 * 8));
  if (!A.blk || !A.idx || !A.mask) return set_error(GPD_ERR_NOMEM, "gpd_ip4_fragments: scratch allocation failed");
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = gpd::launch_ip4_frag(A, s, ctx->num_cus);
  if (e != hipSuccess) return set_error(GPD_ERR_HIP, "gpd_ip4_fragments launch: %s", hipGetErrorString(e));
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, A.blk + A.nblk, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *count = total;
  return GPD_OK;
}

int gpd_host_register(gpd_ctx *ctx, const void *ptr, uint64_t len) {
  if (!ctx || !ptr || !len) return set_error(GPD_ERR_INVALID, "gpd_host_register: bad argument");
  gpd::DeviceScope dscope_;
  HIP_TRY(dscope_.set(ctx->device));
  HIP_TRY(hipHostRegister(const_cast<void *>(ptr), len, hipHostRegisterDefault));
  ctx->registered.emplace_back((const uint8_t *)ptr, len);
  return GPD_OK;
}

// The NUMA node of a device's PCI function (sysfs), -1 when unknown.
static int device_numa_node(int device) {
  char bus[64] = {0};
  int count = 0;
  // (a failed HIP call would stay the thread's last error, and the caller's next launch check,
  // torch's included, would report it: clear it)
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count ||
      hipDeviceGetPCIBusId(bus, (int)sizeof bus - 1, device) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  for (char *c = bus; *c; c++) *c = (char)tolower((unsigned char)*c);
  char path[160];
  std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
  FILE *f = std::fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (std::fscanf(f, "%d", &node) != 1) node = -1;
  std::fclose(f);
  return node;
}

int gpd_host_bind_local(int device, void *ptr, uint64_t len, int *node_out) {
  if (node_out) *node_out = -1;
  if (!ptr || !len) return set_error(GPD_ERR_INVALID, "gpd_host_bind_local: bad argument");
  const int node = device_numa_node(device);
  if (node_out) *node_out = node;
  if (node < 0) return GPD_OK;  // one node, or the platform does not say
  if (node >= 1024) return set_error(GPD_ERR_INVALID, "gpd_host_bind_local: node %d", node);
  const uint64_t page = (uint64_t)sysconf(_SC_PAGESIZE);
  const uint64_t lo = ((uint64_t)ptr + page - 1) & ~(page - 1), hi = ((uint64_t)ptr + len) & ~(page - 1);
  if (hi <= lo) return GPD_OK;
  unsigned long mask[1024 / (8 * sizeof(unsigned long))] = {0};
  mask[node / (8 * sizeof(unsigned long))] = 1ul << (node % (8 * sizeof(unsigned long)));
  // MPOL_PREFERRED (1): the node while it has free pages; MPOL_MF_MOVE (2): migrate pages
  // already placed elsewhere
  if (syscall(SYS_mbind, (void *)lo, hi - lo, 1, mask, (unsigned long)(8 * sizeof mask), 2u) != 0)
    return set_error(GPD_ERR_INVALID, "gpd_host_bind_local: mbind: %s", std::strerror(errno));
  return GPD_OK;
}

int gpd_host_unregister(gpd_ctx *ctx, const void *ptr) {
  if (!ctx) return set_error(GPD_ERR_INVALID, "gpd_host_unregister: null ctx");
  for (size_t k = 0; k < ctx->registered.size(); k++) {
    if (ctx->registered[k].first == ptr) {
      gpd::DeviceScope dscope_;
      HIP_TRY(dscope_.set(ctx->device));
      for (auto &s : ctx->slot)
        if (s.stream) HIP_TRY(hipStreamSynchronize(s.stream));
      HIP_TRY(hipHostUnregister(const_cast<void *>(ptr)));
      ctx->registered.erase(ctx->registered.begin() + (long)k);
      return GPD_OK;
    }
  }
  return set_error(GPD_ERR_INVALID, "gpd_host_unregister: pointer not registered");
}
}  // extern "C"
