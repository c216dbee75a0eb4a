// gpd_bpf_vm.h — the classic-BPF machine of include/gpd_bpf.h, one instruction at a time.
//
// bpf_step is the whole semantics of an instruction: the kernel (gpd_bpf.hip, a lane per packet)
// and gpd_bpf_run_host (gpd_bpf_host.cpp) both call it, so a test of the host entry point tests
// the code the GPU runs.  What differs between the two is only how they reach their operands:
//
//   Pkt  .load(pos, size)  the big-endian value of `size` (1, 2 or 4) packet bytes at `pos`;
//                          bpf_step has checked pos + size <= buflen before it asks
//   Mem  .get(k) / .set(k, v)   the scratch cell M[k], k < 16 (the validator's rule)
//
// bpf_check is the validator; it also says whether the program touches M at all.
#pragma once
#include <stdint.h>

#if defined(__HIP__)  // compiled as HIP: the kernel's translation unit
#include <hip/hip_runtime.h>
#define GPD_BPF_HD __host__ __device__
#else
#define GPD_BPF_HD
#endif

namespace gpd {

constexpr uint32_t kBpfMaxInsns = 4096;  // pcap.MaxBpfInstructions (pcap/pcap.go:36)
constexpr uint32_t kBpfMemWords = 16;    // BPF_MEMWORDS

// linux/bpf_common.h, linux/filter.h
enum : uint32_t {
  BPF_LD = 0x00, BPF_LDX = 0x01, BPF_ST = 0x02, BPF_STX = 0x03, BPF_ALU = 0x04, BPF_JMP = 0x05,
  BPF_RET = 0x06, BPF_MISC = 0x07,
  BPF_W = 0x00, BPF_H = 0x08, BPF_B = 0x10,
  BPF_IMM = 0x00, BPF_ABS = 0x20, BPF_IND = 0x40, BPF_MEM = 0x60, BPF_LEN = 0x80, BPF_MSH = 0xa0,
  BPF_ADD = 0x00, BPF_SUB = 0x10, BPF_MUL = 0x20, BPF_DIV = 0x30, BPF_OR = 0x40, BPF_AND = 0x50,
  BPF_LSH = 0x60, BPF_RSH = 0x70, BPF_NEG = 0x80, BPF_MOD = 0x90, BPF_XOR = 0xa0,
  BPF_JA = 0x00, BPF_JEQ = 0x10, BPF_JGT = 0x20, BPF_JGE = 0x30, BPF_JSET = 0x40,
  BPF_K = 0x00, BPF_X = 0x08, BPF_A = 0x10,
  BPF_TAX = 0x00, BPF_TXA = 0x80,
};

// One instruction.  Returns true when the program ends (ret holds its return value); otherwise
// `skip` is the number of instructions to jump over: the next one is pc + 1 + skip.
template <class Pkt, class Mem>
GPD_BPF_HD inline bool bpf_step(uint32_t code, uint32_t jt, uint32_t jf, uint32_t k, uint32_t &A, uint32_t &X,
                                Mem &M, const Pkt &P, uint32_t buflen, uint32_t wirelen, uint32_t &skip,
                                uint32_t &ret) {
  skip = 0;
  ret = 0;  // every failing load and every division by zero ends the program with 0
  switch (code) {
    // ---- loads from the packet: the comparisons as libpcap writes them, no wrapped sum
    case BPF_LD | BPF_W | BPF_ABS:
      if (k > buflen || 4u > buflen - k) return true;
      A = P.load(k, 4);
      return false;
    case BPF_LD | BPF_H | BPF_ABS:
      if (k > buflen || 2u > buflen - k) return true;
      A = P.load(k, 2);
      return false;
    case BPF_LD | BPF_B | BPF_ABS:
      if (k >= buflen) return true;
      A = P.load(k, 1);
      return false;
    case BPF_LD | BPF_W | BPF_IND:
      if (k > buflen || X > buflen - k || 4u > buflen - (X + k)) return true;
      A = P.load(X + k, 4);
      return false;
    case BPF_LD | BPF_H | BPF_IND:
      if (k > buflen || X > buflen - k || 2u > buflen - (X + k)) return true;
      A = P.load(X + k, 2);
      return false;
    case BPF_LD | BPF_B | BPF_IND:
      if (k >= buflen || X >= buflen - k) return true;
      A = P.load(X + k, 1);
      return false;
    case BPF_LDX | BPF_B | BPF_MSH:
      if (k >= buflen) return true;
      X = (P.load(k, 1) & 0xfu) << 2;
      return false;
    // ---- the other loads, and the stores
    case BPF_LD | BPF_IMM: A = k; return false;
    case BPF_LDX | BPF_IMM: X = k; return false;
    case BPF_LD | BPF_MEM: A = M.get(k); return false;
    case BPF_LDX | BPF_MEM: X = M.get(k); return false;
    case BPF_LD | BPF_W | BPF_LEN: A = wirelen; return false;
    case BPF_LDX | BPF_W | BPF_LEN: X = wirelen; return false;
    case BPF_ST: M.set(k, A); return false;
    case BPF_STX: M.set(k, X); return false;
    // ---- ALU, mod 2^32 (a constant divisor of 0 and a constant shift >= 32 never get here)
    case BPF_ALU | BPF_ADD | BPF_K: A += k; return false;
    case BPF_ALU | BPF_ADD | BPF_X: A += X; return false;
    case BPF_ALU | BPF_SUB | BPF_K: A -= k; return false;
    case BPF_ALU | BPF_SUB | BPF_X: A -= X; return false;
    case BPF_ALU | BPF_MUL | BPF_K: A *= k; return false;
    case BPF_ALU | BPF_MUL | BPF_X: A *= X; return false;
    case BPF_ALU | BPF_DIV | BPF_K: A /= k; return false;
    case BPF_ALU | BPF_DIV | BPF_X:
      if (X == 0) return true;
      A /= X;
      return false;
    case BPF_ALU | BPF_MOD | BPF_K: A %= k; return false;
    case BPF_ALU | BPF_MOD | BPF_X:
      if (X == 0) return true;
      A %= X;
      return false;
    case BPF_ALU | BPF_AND | BPF_K: A &= k; return false;
    case BPF_ALU | BPF_AND | BPF_X: A &= X; return false;
    case BPF_ALU | BPF_OR | BPF_K: A |= k; return false;
    case BPF_ALU | BPF_OR | BPF_X: A |= X; return false;
    case BPF_ALU | BPF_XOR | BPF_K: A ^= k; return false;
    case BPF_ALU | BPF_XOR | BPF_X: A ^= X; return false;
    case BPF_ALU | BPF_LSH | BPF_K: A <<= k; return false;
    case BPF_ALU | BPF_LSH | BPF_X: A = X < 32u ? A << X : 0u; return false;
    case BPF_ALU | BPF_RSH | BPF_K: A >>= k; return false;
    case BPF_ALU | BPF_RSH | BPF_X: A = X < 32u ? A >> X : 0u; return false;
    case BPF_ALU | BPF_NEG: A = 0u - A; return false;
    // ---- jumps, unsigned
    case BPF_JMP | BPF_JA: skip = k; return false;
    case BPF_JMP | BPF_JEQ | BPF_K: skip = A == k ? jt : jf; return false;
    case BPF_JMP | BPF_JEQ | BPF_X: skip = A == X ? jt : jf; return false;
    case BPF_JMP | BPF_JGT | BPF_K: skip = A > k ? jt : jf; return false;
    case BPF_JMP | BPF_JGT | BPF_X: skip = A > X ? jt : jf; return false;
    case BPF_JMP | BPF_JGE | BPF_K: skip = A >= k ? jt : jf; return false;
    case BPF_JMP | BPF_JGE | BPF_X: skip = A >= X ? jt : jf; return false;
    case BPF_JMP | BPF_JSET | BPF_K: skip = (A & k) ? jt : jf; return false;
    case BPF_JMP | BPF_JSET | BPF_X: skip = (A & X) ? jt : jf; return false;
    // ---- return and misc
    case BPF_RET | BPF_K: ret = k; return true;
    case BPF_RET | BPF_A: ret = A; return true;
    case BPF_MISC | BPF_TAX: X = A; return false;
    case BPF_MISC | BPF_TXA: A = X; return false;
  }
  return true;  // (no validated program holds another code)
}

// The validator's verdict on one instruction: nullptr, or the reason it is refused.
inline const char *bpf_check_insn(uint32_t code, uint32_t jt, uint32_t jf, uint32_t k, uint32_t i, uint32_t len,
                                  bool &uses_mem) {
  const uint64_t after = (uint64_t)i + 1u;  // jump targets are after + offset, without a wrap
  switch (code) {
    case BPF_LD | BPF_W | BPF_ABS: case BPF_LD | BPF_H | BPF_ABS: case BPF_LD | BPF_B | BPF_ABS:
    case BPF_LD | BPF_W | BPF_IND: case BPF_LD | BPF_H | BPF_IND: case BPF_LD | BPF_B | BPF_IND:
    case BPF_LDX | BPF_B | BPF_MSH:
    case BPF_LD | BPF_IMM: case BPF_LDX | BPF_IMM:
    case BPF_LD | BPF_W | BPF_LEN: case BPF_LDX | BPF_W | BPF_LEN:
      return nullptr;
    case BPF_LD | BPF_MEM: case BPF_LDX | BPF_MEM: case BPF_ST: case BPF_STX:
      uses_mem = true;
      return k < kBpfMemWords ? nullptr : "scratch memory index out of range (M has 16 cells)";
    case BPF_ALU | BPF_ADD | BPF_K: case BPF_ALU | BPF_ADD | BPF_X:
    case BPF_ALU | BPF_SUB | BPF_K: case BPF_ALU | BPF_SUB | BPF_X:
    case BPF_ALU | BPF_MUL | BPF_K: case BPF_ALU | BPF_MUL | BPF_X:
    case BPF_ALU | BPF_DIV | BPF_X: case BPF_ALU | BPF_MOD | BPF_X:
    case BPF_ALU | BPF_AND | BPF_K: case BPF_ALU | BPF_AND | BPF_X:
    case BPF_ALU | BPF_OR | BPF_K: case BPF_ALU | BPF_OR | BPF_X:
    case BPF_ALU | BPF_XOR | BPF_K: case BPF_ALU | BPF_XOR | BPF_X:
    case BPF_ALU | BPF_LSH | BPF_X: case BPF_ALU | BPF_RSH | BPF_X:
    case BPF_ALU | BPF_NEG:
      return nullptr;
    case BPF_ALU | BPF_DIV | BPF_K: case BPF_ALU | BPF_MOD | BPF_K:
      return k != 0 ? nullptr : "division by the constant 0";
    case BPF_ALU | BPF_LSH | BPF_K: case BPF_ALU | BPF_RSH | BPF_K:
      return k < 32u ? nullptr : "shift by a constant of 32 or more";
    case BPF_JMP | BPF_JA:
      return after + k < len ? nullptr : "jump target beyond the program";
    case BPF_JMP | BPF_JEQ | BPF_K: case BPF_JMP | BPF_JEQ | BPF_X:
    case BPF_JMP | BPF_JGT | BPF_K: case BPF_JMP | BPF_JGT | BPF_X:
    case BPF_JMP | BPF_JGE | BPF_K: case BPF_JMP | BPF_JGE | BPF_X:
    case BPF_JMP | BPF_JSET | BPF_K: case BPF_JMP | BPF_JSET | BPF_X:
      return after + jt < len && after + jf < len ? nullptr : "jump target beyond the program";
    case BPF_RET | BPF_K: case BPF_RET | BPF_A:
    case BPF_MISC | BPF_TAX: case BPF_MISC | BPF_TXA:
      return nullptr;
  }
  return "unknown instruction code";
}

}  // namespace gpd
