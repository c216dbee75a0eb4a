// gpd_bpf_host.h — what gpd_bpf.hip takes from gpd_bpf_host.cpp (not public ABI).
#pragma once
#include <stdint.h>

#include "../../include/gpd_bpf.h"

namespace gpd {
// The validator of include/gpd_bpf.h: GPD_OK, or GPD_ERR_INVALID with the error text set
// (prefixed with `who`).  *uses_mem (may be NULL): the program holds an instruction on M.
int bpf_validate(const char *who, const gpd_bpf_insn *prog, uint32_t len, bool *uses_mem);
}  // namespace gpd
