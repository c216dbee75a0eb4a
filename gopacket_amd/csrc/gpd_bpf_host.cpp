// gpd_bpf_host.cpp — the host half of include/gpd_bpf.h: the validator and one packet through
// the interpreter of gpd_bpf_vm.h.  Plain C++ with no device code and no HIP header, so that a
// stand-alone program can be built from this file alone (tests/c/bpf_host.c, with
// -DGPD_BPF_STANDALONE, which supplies the error text the runtime otherwise keeps).
#include <stdarg.h>
#include <stdio.h>

#include "../../include/gpd_bpf.h"
#include "gpd_bpf_host.h"
#include "gpd_bpf_vm.h"

#ifdef GPD_BPF_STANDALONE
namespace {
thread_local char g_bpf_err[256];
}
namespace gpd {
int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_bpf_err, sizeof g_bpf_err, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace gpd
extern "C" const char *gpd_last_error_string(void) { return g_bpf_err; }
#else
namespace gpd {
int set_error(int code, const char *fmt, ...);  // gpd_runtime.cpp
}
#endif

namespace gpd {

int bpf_validate(const char *who, const gpd_bpf_insn *prog, uint32_t len, bool *uses_mem) {
  bool mem = false;
  if (uses_mem) *uses_mem = false;
  if (!prog) return set_error(GPD_ERR_INVALID, "%s: null program", who);
  if (len < 1) return set_error(GPD_ERR_INVALID, "%s: bpfInstructions must not be empty", who);
  if (len > kBpfMaxInsns)
    return set_error(GPD_ERR_INVALID, "%s: bpfInstructions must not be larger than %u (got %u)", who,
                     kBpfMaxInsns, len);
  for (uint32_t i = 0; i < len; ++i) {
    const gpd_bpf_insn &q = prog[i];
    const char *why = bpf_check_insn(q.code, q.jt, q.jf, q.k, i, len, mem);
    if (why)
      return set_error(GPD_ERR_INVALID, "%s: instruction %u {0x%02x, %u, %u, 0x%08x}: %s", who, i, q.code, q.jt,
                       q.jf, q.k, why);
  }
  const uint32_t last = prog[len - 1].code;
  if (last != (BPF_RET | BPF_K) && last != (BPF_RET | BPF_A))
    return set_error(GPD_ERR_INVALID, "%s: instruction %u {0x%02x, ...}: the last instruction is not a RET", who,
                     len - 1, last);
  if (uses_mem) *uses_mem = mem;
  return GPD_OK;
}

namespace {
struct HostPkt {
  const uint8_t *p;
  uint32_t load(uint32_t pos, uint32_t size) const {
    uint32_t v = 0;
    for (uint32_t b = 0; b < size; ++b) v = (v << 8) | p[pos + b];
    return v;
  }
};
struct HostMem {
  uint32_t m[kBpfMemWords] = {};
  uint32_t get(uint32_t k) const { return m[k]; }
  void set(uint32_t k, uint32_t v) { m[k] = v; }
};
}  // namespace

}  // namespace gpd

extern "C" {

int gpd_bpf_validate(const gpd_bpf_insn *prog, uint32_t len) {
  return gpd::bpf_validate("gpd_bpf_validate", prog, len, nullptr);
}

uint32_t gpd_bpf_run_host(const gpd_bpf_insn *prog, uint32_t len, const uint8_t *data, uint32_t caplen,
                          uint32_t wirelen) {
  using namespace gpd;
  if (bpf_validate("gpd_bpf_run_host", prog, len, nullptr) != GPD_OK) return 0;
  if (!data) caplen = 0;
  HostPkt P{data};
  HostMem M;
  uint32_t A = 0, X = 0, skip = 0, ret = 0;
  for (uint64_t pc = 0; pc < len; pc += 1ull + skip) {  // (the bound the validator proves)
    const gpd_bpf_insn &q = prog[pc];
    if (bpf_step(q.code, q.jt, q.jf, q.k, A, X, M, P, caplen, wirelen, skip, ret)) return ret;
  }
  return 0;
}

}  // extern "C"
