// gpd_bpf.hip — a classic BPF program over a device batch, one packet per lane: include/gpd_bpf.h.
//
// Classic BPF only jumps forward, so a wave needs no per-lane instruction fetch and no divergent
// switch over 60 codes.  bpf_kernel sweeps the program once: pc goes 0, 1, 2, ... as a scalar,
// each lane holds the index of the instruction it executes next, and at step pc the lanes whose
// index is pc execute it under the EXEC mask.  The instruction word is the same for the whole
// wave: its index goes through readfirstlane, so it is fetched with a scalar load and the switch
// on its code is a scalar branch.  A step no lane is on costs a ballot and a branch.  The sweep
// ends at len, or at the first empty step after every lane has returned.  The instruction's
// meaning is bpf_step (gpd_bpf_vm.h), the code gpd_bpf_run_host runs.
//
// Packet bytes are read per lane at data + offset[i] + pos as the (at most two) aligned 32-bit
// words that hold them, shifted together in registers; bpf_step has checked pos + size <= buflen
// first, so both words start inside [0, round_up(data_len, 16)), which is all the batch contract
// promises.  M[16] exists only in the instance for programs that use it (gpd_bpf_create knows):
// 16 x 256 words of LDS, cell k of thread t at [k][t], so the wave-uniform k gives a
// conflict-free access; the other instance has no LDS and no scratch.  keep and ret leave as one
// coalesced store per wave each.
#include <hip/hip_runtime.h>

#include "gpd_internal.h"
#include "gpd_launch.h"
#include "gpd_bpf_host.h"
#include "gpd_bpf_vm.h"

struct gpd_bpf {
  int device;
  int num_cus;
  uint2 *prog;  // device: {code | jt << 16 | jf << 24, k} per instruction (gpd_bpf_insn's bytes)
  uint32_t len;
  bool uses_mem;
};

namespace gpd {
namespace {

static_assert(sizeof(gpd_bpf_insn) == 8, "gpd_bpf_insn is pcap.BPFInstruction: 8 bytes");

constexpr uint32_t kBpfWaves = 4;                  // waves per workgroup, a 64-packet tile each
constexpr uint32_t kBpfThreads = 64 * kBpfWaves;
constexpr uint32_t kBpfMaxWgs = 8;                 // workgroups resident per CU (32 waves)
constexpr uint32_t kDone = 0xFFFFFFFFu;            // a lane's next index once it has returned

struct BpfArgs {
  const uint8_t *data;
  uint32_t dlen;            // data_len (32-bit, as the decode reads it)
  uint64_t lim;             // round_up(data_len, 16): no load starts at or beyond it
  const uint32_t *offset, *caplen;
  const uint32_t *wirelen;  // may be NULL
  uint64_t n, ntiles;
  uint8_t *keep;
  uint32_t *ret;            // may be NULL
  uint32_t len;             // instructions
};

struct DevPkt {
  const uint8_t *data;
  uint64_t lim;
  uint32_t off;
  // the big-endian value of the `size` bytes at packet position pos (pos + size <= buflen)
  __device__ uint32_t load(uint32_t pos, uint32_t size) const {
    const uint64_t a = (uint64_t)off + pos, a0 = a & ~3ull;
    const uint32_t s = (uint32_t)a & 3u;
    const uint32_t lo = *reinterpret_cast<const uint32_t *>(data + a0);
    uint32_t hi = 0;  // needed when the bytes run into the next word, which then lies below lim
    if (s + size > 4u && a0 + 4u < lim) hi = *reinterpret_cast<const uint32_t *>(data + a0 + 4u);
    return __builtin_bswap32(__funnelshift_r(lo, hi, s * 8u)) >> (32u - 8u * size);
  }
};

template <bool MEM>
struct Scratch;
template <>
struct Scratch<false> {  // a program without M: nothing
  __device__ void clear() {}
  __device__ uint32_t get(uint32_t) const { return 0; }
  __device__ void set(uint32_t, uint32_t) {}
};
template <>
struct Scratch<true> {
  uint32_t *cell;  // this thread's column of the workgroup's [16][256] words
  __device__ Scratch() {
    __shared__ uint32_t m[kBpfMemWords * kBpfThreads];
    cell = m + threadIdx.x;
  }
  __device__ void clear() {
#pragma unroll
    for (uint32_t k = 0; k < kBpfMemWords; ++k) cell[k * kBpfThreads] = 0;
  }
  __device__ uint32_t get(uint32_t k) const { return cell[k * kBpfThreads]; }
  __device__ void set(uint32_t k, uint32_t v) { cell[k * kBpfThreads] = v; }
};

template <bool MEM>
__global__ __launch_bounds__(kBpfThreads) void bpf_kernel(BpfArgs A, const uint2 *__restrict__ prog) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  Scratch<MEM> M;
  for (uint64_t t = (uint64_t)blockIdx.x * kBpfWaves + w; t < A.ntiles; t += (uint64_t)gridDim.x * kBpfWaves) {
    const uint64_t i = t * 64u + lane;
    const bool live = i < A.n;
    uint32_t off = 0, buflen = 0, wirelen = 0;
    if (live) {  // clamped to the buffer as the decode clamps a descriptor
      off = min(A.offset[i], A.dlen);
      buflen = min(A.caplen[i], A.dlen - off);
      wirelen = A.wirelen ? A.wirelen[i] : buflen;
    }
    const DevPkt P{A.data, A.lim, off};
    M.clear();
    uint32_t next = live ? 0u : kDone, a = 0, x = 0, ret = 0;
    for (uint32_t pc = 0; pc < A.len; ++pc) {
      if (__ballot(next == pc) == 0ull) {
        if (__ballot(next != kDone) == 0ull) break;  // every lane has returned
        continue;
      }
      const uint2 q = prog[__builtin_amdgcn_readfirstlane(pc)];
      const uint32_t word = __builtin_amdgcn_readfirstlane(q.x), k = __builtin_amdgcn_readfirstlane(q.y);
      if (next == pc) {
        uint32_t skip, r;
        if (bpf_step(word & 0xFFFFu, (word >> 16) & 0xFFu, word >> 24, k, a, x, M, P, buflen, wirelen, skip, r)) {
          ret = r;
          next = kDone;
        } else {
          next = pc + 1u + skip;
        }
      }
    }
    if (live) {
      A.keep[i] = ret != 0u ? 1 : 0;
      if (A.ret) A.ret[i] = ret;
    }
  }
}

}  // namespace
}  // namespace gpd

extern "C" {

int gpd_bpf_create(gpd_ctx *ctx, const gpd_bpf_insn *prog, uint32_t len, gpd_bpf **out) {
  using namespace gpd;
  const char *who = "gpd_bpf_create";
  if (!ctx || !out) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  *out = nullptr;
  bool uses_mem = false;
  const int rc = bpf_validate(who, prog, len, &uses_mem);
  if (rc) return rc;
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(ctx_device(ctx)));
  uint2 *d = nullptr;
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), (size_t)len * sizeof(gpd_bpf_insn));
  if (e != hipSuccess)
    return set_error(e == hipErrorOutOfMemory ? GPD_ERR_NOMEM : GPD_ERR_HIP, "%s: program upload: %s", who,
                     hipGetErrorString(e));
  const hipError_t c = hipMemcpy(d, prog, (size_t)len * sizeof(gpd_bpf_insn), hipMemcpyHostToDevice);
  if (c != hipSuccess) {
    (void)hipFree(d);
    return set_error(GPD_ERR_HIP, "%s: program upload: %s", who, hipGetErrorString(c));
  }
  *out = new gpd_bpf{ctx_device(ctx), ctx_num_cus(ctx), d, len, uses_mem};
  return GPD_OK;
}

void gpd_bpf_destroy(gpd_bpf *f) {
  if (!f) return;
  gpd::DeviceScope dscope_;
  if (dscope_.set(f->device) == hipSuccess) (void)hipFree(f->prog);
  delete f;
}

int gpd_bpf_filter(gpd_bpf *f, const gpd_batch *in, const uint32_t *wirelen, uint8_t *keep, uint32_t *ret,
                   void *stream) {
  using namespace gpd;
  const char *who = "gpd_bpf_filter";
  if (!f || !in) return set_error(GPD_ERR_INVALID, "%s: null argument", who);
  if (in->n == 0) return GPD_OK;
  if (in->n > 0xFFFFFF00ull)
    return set_error(GPD_ERR_INVALID, "%s: batch of %llu packets (max 2^32 - 256)", who, (unsigned long long)in->n);
  if (!in->data || !in->offset || !in->caplen)
    return set_error(GPD_ERR_INVALID, "%s: batch data/offset/caplen must be non-NULL", who);
  if (in->data_len >= 0xFFFFFFF0ull)
    return set_error(GPD_ERR_INVALID, "%s: data_len %llu outside the 32-bit offset range", who,
                     (unsigned long long)in->data_len);
  if (!keep) return set_error(GPD_ERR_INVALID, "%s: null keep", who);
  DeviceScope dscope_;
  GPD_TRY(dscope_.set(f->device));
  BpfArgs A{};
  A.data = in->data;
  A.dlen = (uint32_t)in->data_len;
  A.lim = (in->data_len + 15ull) & ~15ull;
  A.offset = in->offset;
  A.caplen = in->caplen;
  A.wirelen = wirelen;
  A.n = in->n;
  A.ntiles = (in->n + 63u) / 64u;
  A.keep = keep;
  A.ret = ret;
  A.len = f->len;
  const LaunchGeom g = launch_geom(0, f->uses_mem ? kBpfMemWords * kBpfThreads * 4u : 0u, kBpfWaves, 0, kBpfMaxWgs,
                                   0, kGridRounds, f->num_cus, A.ntiles);
  const hipStream_t s = (hipStream_t)stream;
  // (M is static LDS of its instance; g.lds, which counts a dispatch image no filter has, is not passed)
  if (f->uses_mem)
    hipLaunchKernelGGL(bpf_kernel<true>, dim3((unsigned)g.blocks), dim3(kBpfThreads), 0, s, A, f->prog);
  else
    hipLaunchKernelGGL(bpf_kernel<false>, dim3((unsigned)g.blocks), dim3(kBpfThreads), 0, s, A, f->prog);
  GPD_TRY(hipGetLastError());
  return GPD_OK;
}

}  // extern "C"
