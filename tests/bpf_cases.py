"""Programs and packets the BPF tests share (tests/test_bpf.py on the host entry points,
tests/test_bpf_gpu.py on the device, tests/c/bpf_host.c under the sanitizers): one program per
instruction form and edge of include/gpd_bpf.h, programs that break one validation rule each,
and seeded random programs that are valid by construction.  Expected values always come from the
checker (tests/bpf_ref.py), never from the code under test."""
import json
import os

import numpy as np

import bpf_ref as R
from bpf_ref import (A, ABS, ADD, ALU, AND, B, DIV, H, IMM, IND, JA, JEQ, JGE, JGT, JMP, JSET, K, LD, LDX, LEN,
                     LSH, MEM, MISC, MOD, MSH, MUL, NEG, OR, RET, RSH, ST, STX, SUB, TAX, TXA, W, X, XOR)

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "bpf_vectors.json")))
PACKET = bytes.fromhex(VEC["packet"]["hex"])  # pcap/bpf_test.go's 38 bytes
PORT80 = [tuple(q) for q in VEC["filters"][0]["program"]]  # ip and tcp and port 80
UDP80 = [tuple(q) for q in VEC["filters"][1]["program"]]

L = 20  # the edge packet's capture length
RET_A = (RET | A, 0, 0, 0)


def ret_k(k):
    return (RET | K, 0, 0, k)


def edge_packets():
    """(data, wirelen) pairs every edge program runs over: L nonzero bytes (a load that works
    never gives the 0 of a load that fails), one byte, none, and 5 bytes of a longer packet."""
    rng = np.random.default_rng(20)
    body = rng.integers(1, 256, L, dtype=np.uint8).tobytes()
    return [(body, L), (body[:1], 1), (b"", 0), (body[:5], 1000), (b"", 77)]


def edge_programs():
    """(name, program) pairs."""
    out = []
    # packet loads around the end of the buffer, and far beyond it (the Linux ancillary offsets)
    for sz, name in ((W, "w"), (H, "h"), (B, "b")):
        for k in [0, 1] + list(range(L - 4, L + 2)) + [0xFFFFF000, 0xFFFFFFFC, 0xFFFFFFFF]:
            out.append((f"ld_{name}_abs_{k:#x}", [(LD | sz | ABS, 0, 0, k), RET_A]))
        for x in (0, 1, L - 1, L, 0xFFFFFFFF):
            for k in (0, 1, 3, L - 4, L - 2, L - 1, L, L + 1, 0xFFFFFFFF):
                out.append((f"ld_{name}_ind_x{x:#x}_k{k:#x}",
                            [(LDX | IMM, 0, 0, x), (LD | sz | IND, 0, 0, k), RET_A]))
    for k in (0, 4, L - 1, L, 0xFFFFFFFF):
        out.append((f"ldx_msh_{k:#x}", [(LDX | B | MSH, 0, 0, k), (MISC | TXA, 0, 0, 0), RET_A]))
    # the loads that never fail
    out.append(("ld_imm", [(LD | IMM, 0, 0, 0xDEADBEEF), RET_A]))
    out.append(("ldx_imm_txa", [(LDX | IMM, 0, 0, 0xCAFEF00D), (MISC | TXA, 0, 0, 0), RET_A]))
    out.append(("tax_txa", [(LD | IMM, 0, 0, 77), (MISC | TAX, 0, 0, 0), (LD | IMM, 0, 0, 1), (MISC | TXA, 0, 0, 0),
                            RET_A]))
    out.append(("ld_len", [(LD | W | LEN, 0, 0, 0), RET_A]))
    out.append(("ldx_len", [(LDX | W | LEN, 0, 0, 0), (MISC | TXA, 0, 0, 0), RET_A]))
    out.append(("ret_k", [ret_k(0xFFFFFFFF)]))
    out.append(("ret_k_0", [ret_k(0)]))
    out.append(("ret_a_initial", [RET_A]))  # A starts at 0
    out.append(("x_initial", [(MISC | TXA, 0, 0, 0), (ALU | ADD | K, 0, 0, 1), RET_A]))  # so does X
    # M: every cell both ways, all 16 at once, and a read before any write
    for c in range(16):
        out.append((f"st_ld_mem_{c}", [(LD | IMM, 0, 0, 0x1000 + c), (ST, 0, 0, c), (LD | IMM, 0, 0, 0),
                                       (LD | MEM, 0, 0, c), RET_A]))
        out.append((f"stx_ldx_mem_{c}", [(LDX | IMM, 0, 0, 0x2000 + c), (STX, 0, 0, c), (LDX | IMM, 0, 0, 0),
                                         (LDX | MEM, 0, 0, c), (MISC | TXA, 0, 0, 0), RET_A]))
    prog = []
    for c in range(16):
        prog += [(LD | IMM, 0, 0, (c + 1) * 0x01010101), (ST, 0, 0, c)]
    prog.append((LD | IMM, 0, 0, 0))
    for c in range(16):
        prog += [(LDX | MEM, 0, 0, c), (ALU | ADD | X, 0, 0, 0), (ALU | MUL | K, 0, 0, 3)]
    out.append(("mem_all_16", prog + [RET_A]))
    out.append(("mem_read_before_write", [(LD | MEM, 0, 0, 5), (ALU | ADD | K, 0, 0, 1), RET_A]))
    out.append(("memx_read_before_write", [(LDX | MEM, 0, 0, 15), (MISC | TXA, 0, 0, 0), (ALU | ADD | K, 0, 0, 1),
                                           RET_A]))
    out.append(("mem_packet_dependent", [(LD | B | ABS, 0, 0, 0), (ST, 0, 0, 3), (LDX | B | MSH, 0, 0, 0),
                                         (STX, 0, 0, 4), (LD | MEM, 0, 0, 4), (LDX | MEM, 0, 0, 3),
                                         (ALU | ADD | X, 0, 0, 0), RET_A]))
    # ALU: every operation with K and with X; + 1 tells a result of 0 from a failure
    a0, s0 = 0x80000001, 7
    for op, name in ((ADD, "add"), (SUB, "sub"), (MUL, "mul"), (DIV, "div"), (MOD, "mod"), (AND, "and"), (OR, "or"),
                     (XOR, "xor"), (LSH, "lsh"), (RSH, "rsh")):
        out.append((f"{name}_k", [(LD | IMM, 0, 0, a0), (ALU | op | K, 0, 0, s0), (ALU | ADD | K, 0, 0, 1), RET_A]))
        out.append((f"{name}_x", [(LD | IMM, 0, 0, a0), (LDX | IMM, 0, 0, s0), (ALU | op | X, 0, 0, 0),
                                  (ALU | ADD | K, 0, 0, 1), RET_A]))
    for op, name in ((DIV, "div"), (MOD, "mod")):
        out.append((f"{name}_x_zero", [(LD | IMM, 0, 0, 7), (ALU | op | X, 0, 0, 0), ret_k(5)]))
    for op, name in ((LSH, "lsh"), (RSH, "rsh")):
        for s in (0, 1, 31, 32, 33, 0xFFFFFFFF):
            out.append((f"{name}_x_{s:#x}", [(LD | IMM, 0, 0, a0), (LDX | IMM, 0, 0, s), (ALU | op | X, 0, 0, 0),
                                             (ALU | ADD | K, 0, 0, 1), RET_A]))
        out.append((f"{name}_k_31", [(LD | IMM, 0, 0, a0), (ALU | op | K, 0, 0, 31), (ALU | ADD | K, 0, 0, 1), RET_A]))
    out.append(("neg_0", [(ALU | NEG, 0, 0, 0), (ALU | ADD | K, 0, 0, 1), RET_A]))
    out.append(("neg_5", [(LD | IMM, 0, 0, 5), (ALU | NEG, 0, 0, 0), RET_A]))
    out.append(("mul_k_wrap", [(LD | IMM, 0, 0, 0x10001), (ALU | MUL | K, 0, 0, 0xFFFF0001), RET_A]))
    out.append(("mul_x_wrap", [(LD | IMM, 0, 0, 0xFFFFFFFF), (LDX | IMM, 0, 0, 0xFFFFFFFF), (ALU | MUL | X, 0, 0, 0),
                               RET_A]))
    out.append(("add_wrap", [(LD | IMM, 0, 0, 0xFFFFFFFF), (ALU | ADD | K, 0, 0, 2), RET_A]))
    out.append(("sub_wrap", [(ALU | SUB | K, 0, 0, 1), RET_A]))
    # jumps
    out.append(("ja_to_last", [(JMP | JA, 0, 0, 1), ret_k(7), ret_k(9)]))
    out.append(("ja_0", [(JMP | JA, 0, 0, 0), ret_k(7)]))
    for op, name in ((JEQ, "jeq"), (JGT, "jgt"), (JGE, "jge"), (JSET, "jset")):
        for a in (0x7FFFFFFF, 0x80000000, 0x80000001, 0):  # around s = 2^31: the comparisons are unsigned
            s = 0x80000000
            tail = [ret_k(1), ret_k(2), ret_k(3)]
            out.append((f"{name}_k_a{a:#x}", [(LD | IMM, 0, 0, a), (JMP | op | K, 0, 1, s)] + tail))
            out.append((f"{name}_x_a{a:#x}", [(LD | IMM, 0, 0, a), (LDX | IMM, 0, 0, s), (JMP | op | X, 2, 0, 0)]
                        + tail))
    out.append(("jump_255", [(LD | B | ABS, 0, 0, 0), (JMP | JGT | K, 255, 0, 0x7F)] + [ret_k(10 + i) for i in range(256)]))
    out.append(("port80", PORT80))
    out.append(("udp80", UDP80))
    for name, prog in out:
        assert R.validate(prog) is None, (name, R.validate(prog))
    return out


def max_length_program():
    """4095 x ADD #1 then RET A: returns 4095."""
    return [(ALU | ADD | K, 0, 0, 1)] * 4095 + [RET_A]


def invalid_programs():
    """(name, program, index of the refused instruction): each breaks one rule only."""
    ok = ret_k(1)
    out = [
        ("unknown_code_ffff", [(0xFFFF, 0, 0, 0), ok], 0),
        ("unknown_ret_x", [(RET | X, 0, 0, 0)], 0),
        ("unknown_ld_h_imm", [ok, (LD | H | IMM, 0, 0, 0), ok], 1),
        ("unknown_ldx_abs", [(LDX | W | ABS, 0, 0, 0), ok], 0),
        ("unknown_neg_x", [(ALU | NEG | X, 0, 0, 0), ok], 0),
        ("unknown_alu_op", [(ALU | 0xB0, 0, 0, 1), ok], 0),
        ("unknown_jmp_op", [(JMP | 0x50, 0, 0, 0), ok], 0),
        ("unknown_high_bits", [(0x0100 | RET | K, 0, 0, 0), ok], 0),
        ("ld_mem_16", [(LD | MEM, 0, 0, 16), ok], 0),
        ("ldx_mem_16", [(LDX | MEM, 0, 0, 16), ok], 0),
        ("st_16", [(ST, 0, 0, 16), ok], 0),
        ("stx_big", [ok, (STX, 0, 0, 0xFFFFFFFF), ok], 1),
        ("div_k_0", [(ALU | DIV | K, 0, 0, 0), ok], 0),
        ("mod_k_0", [(ALU | MOD | K, 0, 0, 0), ok], 0),
        ("lsh_k_32", [(ALU | LSH | K, 0, 0, 32), ok], 0),
        ("rsh_k_big", [(ALU | RSH | K, 0, 0, 0xFFFFFFFF), ok], 0),
        ("ja_past_end", [(JMP | JA, 0, 0, 1), ok], 0),
        ("ja_wraps", [ok, (JMP | JA, 0, 0, 0xFFFFFFFE), ok], 1),  # 2 + 0xFFFFFFFE = 0 mod 2^32
        ("ja_wraps_to_self", [(JMP | JA, 0, 0, 0xFFFFFFFF), ok], 0),
        ("jt_past_end", [(JMP | JEQ | K, 1, 0, 0), ok], 0),
        ("jf_past_end", [(JMP | JSET | X, 0, 1, 0), ok], 0),
        ("jt_255", [(JMP | JGE | K, 255, 0, 0)] + [ok] * 255, 0),
        ("last_not_ret", [(LD | IMM, 0, 0, 0)], 0),
        ("last_not_ret_2", [ok, (ALU | ADD | K, 0, 0, 1)], 1),
    ]
    for name, prog, idx in out:
        got = R.validate(prog)
        assert got is not None and got[0] == idx, (name, got)
    return out


def _random_insn(rng, room):
    """One random instruction that is valid with `room` instructions after it (room >= 1)."""
    small = lambda: int(rng.integers(0, 90))
    anyk = lambda: int(rng.choice([small(), small(), int(rng.integers(0, 1 << 32)), 0xFFFFFFFF, 0]))
    kind = int(rng.integers(0, 12))
    if kind <= 2:
        return (LD | int(rng.choice([W, H, B])) | int(rng.choice([ABS, IND])), 0, 0, int(rng.choice([small(), anyk()])))
    if kind == 3:
        return (int(rng.choice([LD | IMM, LDX | IMM, LD | W | LEN, LDX | W | LEN, MISC | TAX, MISC | TXA])), 0, 0,
                int(rng.choice([small(), anyk()])))
    if kind == 4:
        return (LDX | B | MSH, 0, 0, small())
    if kind == 5:
        return (int(rng.choice([LD | MEM, LDX | MEM, ST, STX])), 0, 0, int(rng.integers(0, 16)))
    if kind <= 7:
        op, src = int(rng.choice(R.BINOPS + (NEG,))), int(rng.choice([K, X]))
        if op == NEG:
            return (ALU | NEG, 0, 0, anyk())
        k = anyk()
        if src == K and op in (DIV, MOD):
            k = k or 3
        if src == K and op in (LSH, RSH):
            k %= 32
        return (ALU | op | src, 0, 0, k)
    if kind == 8:
        return (JMP | JA, 0, 0, int(rng.integers(0, min(room, 6))))
    if kind <= 10:
        hi = min(room, 256, 12)
        return (JMP | int(rng.choice([JEQ, JGT, JGE, JSET])) | int(rng.choice([K, X])), int(rng.integers(0, hi)),
                int(rng.integers(0, hi)), int(rng.choice([small(), anyk()])))
    return (RET | int(rng.choice([K, A])), 0, 0, anyk())


def random_program(seed):
    """A valid program of 1..64 instructions."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 65))
    prog = [_random_insn(rng, n - 1 - i) for i in range(n - 1)]
    prog.append((RET | int(rng.choice([K, A])), 0, 0, int(rng.integers(0, 1 << 32))))
    assert R.validate(prog) is None, R.validate(prog)
    return prog


def random_packets(seed, count=64):
    """(data, wirelen) pairs: lengths 0..100, most bytes small so that MSH and IND stay in range."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.choice([0, 1, 2, 3, 4, 14, 34, 54, 60, 64, int(rng.integers(0, 101))]))
        data = np.where(rng.integers(0, 3, n) == 0, rng.integers(0, 256, n), rng.integers(0, 24, n)).astype(np.uint8)
        out.append((data.tobytes(), n + int(rng.integers(0, 3)) * 700))
    return out
