"""A plain-Python restatement of the classic-BPF machine of include/gpd_bpf.h — test
infrastructure: the yardstick gpd_bpf_validate, gpd_bpf_run_host and gpd_bpf_filter are compared
with.  Nothing under gopacket_amd/ imports it, and it shares no code with the interpreter under
test (gopacket_amd/csrc/gpd_bpf_vm.h): it is written from the rules, libpcap's bpf_filter as the
header restates them.

  validate(prog)            None, or (instruction index, reason) of the first broken rule
  run(prog, data, wirelen)  the program's return value for one packet (Matches is `!= 0`)

A program is a sequence of (code, jt, jf, k).  A, X and M[0..15] are u32 and start at 0; a failing
packet load and a division by X == 0 end the program with 0.
"""
MAX_INSNS = 4096
MEMWORDS = 16
U32 = 0xFFFFFFFF

# instruction classes, sizes, modes, ALU / jump operations, sources (linux/bpf_common.h, filter.h)
LD, LDX, ST, STX, ALU, JMP, RET, MISC = range(8)
W, H, B = 0x00, 0x08, 0x10
IMM, ABS, IND, MEM, LEN, MSH = 0x00, 0x20, 0x40, 0x60, 0x80, 0xA0
ADD, SUB, MUL, DIV, OR, AND, LSH, RSH, NEG, MOD, XOR = (0x00, 0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70,
                                                        0x80, 0x90, 0xA0)
JA, JEQ, JGT, JGE, JSET = 0x00, 0x10, 0x20, 0x30, 0x40
K, X, A = 0x00, 0x08, 0x10
TAX, TXA = 0x00, 0x80

SIZE = {W: 4, H: 2, B: 1}
PKT_LOADS = {LD | sz | mode: (mode, SIZE[sz]) for sz in (W, H, B) for mode in (ABS, IND)}
BINOPS = (ADD, SUB, MUL, DIV, MOD, AND, OR, XOR, LSH, RSH)
ALU_CODES = {ALU | op | src: (op, src) for op in BINOPS for src in (K, X)}
ALU_CODES[ALU | NEG] = (NEG, K)
COND_CODES = {JMP | op | src: (op, src) for op in (JEQ, JGT, JGE, JSET) for src in (K, X)}
MEM_CODES = (LD | MEM, LDX | MEM, ST, STX)
OTHER_CODES = (LD | IMM, LDX | IMM, LD | W | LEN, LDX | W | LEN, LDX | B | MSH, JMP | JA, RET | K, RET | A,
               MISC | TAX, MISC | TXA)
ALL_CODES = sorted(set(PKT_LOADS) | set(ALU_CODES) | set(COND_CODES) | set(MEM_CODES) | set(OTHER_CODES))


def validate(prog):
    n = len(prog)
    if n < 1:
        return (0, "empty")
    if n > MAX_INSNS:
        return (0, "too long")
    for i, (code, jt, jf, k) in enumerate(prog):
        if code not in ALL_CODES:
            return (i, "unknown code")
        if code in MEM_CODES and k >= MEMWORDS:
            return (i, "M index")
        if code in (ALU | DIV | K, ALU | MOD | K) and k == 0:
            return (i, "division by 0")
        if code in (ALU | LSH | K, ALU | RSH | K) and k >= 32:
            return (i, "shift")
        if code == JMP | JA and i + 1 + k >= n:  # Python integers: no wrap
            return (i, "jump")
        if code in COND_CODES and (i + 1 + jt >= n or i + 1 + jf >= n):
            return (i, "jump")
    if prog[-1][0] not in (RET | K, RET | A):
        return (n - 1, "last not RET")
    return None


def _be(data, pos, size):
    return int.from_bytes(data[pos:pos + size], "big")


def run(prog, data, wirelen=None):
    assert validate(prog) is None
    data = bytes(data)
    buflen = len(data)
    wirelen = buflen if wirelen is None else wirelen
    a = x = 0
    m = [0] * MEMWORDS
    pc = 0
    while True:
        code, jt, jf, k = prog[pc]
        pc += 1
        if code in PKT_LOADS:
            mode, size = PKT_LOADS[code]
            if mode == ABS:
                if size == 1:
                    if k >= buflen:
                        return 0
                elif k > buflen or size > buflen - k:
                    return 0
                pos = k
            else:
                if size == 1:
                    if k >= buflen or x >= buflen - k:
                        return 0
                elif k > buflen or x > buflen - k or size > buflen - (x + k):
                    return 0
                pos = x + k
            a = _be(data, pos, size)
        elif code == LDX | B | MSH:
            if k >= buflen:
                return 0
            x = (data[k] & 0xF) << 2
        elif code == LD | IMM:
            a = k
        elif code == LDX | IMM:
            x = k
        elif code == LD | MEM:
            a = m[k]
        elif code == LDX | MEM:
            x = m[k]
        elif code == LD | W | LEN:
            a = wirelen
        elif code == LDX | W | LEN:
            x = wirelen
        elif code == ST:
            m[k] = a
        elif code == STX:
            m[k] = x
        elif code in ALU_CODES:
            op, src = ALU_CODES[code]
            s = x if src == X else k
            if op == ADD:
                a = (a + s) & U32
            elif op == SUB:
                a = (a - s) & U32
            elif op == MUL:
                a = (a * s) & U32
            elif op in (DIV, MOD):
                if s == 0:
                    return 0
                a = a // s if op == DIV else a % s
            elif op == AND:
                a &= s
            elif op == OR:
                a |= s
            elif op == XOR:
                a ^= s
            elif op == LSH:
                a = (a << s) & U32 if s < 32 else 0
            elif op == RSH:
                a = a >> s if s < 32 else 0
            elif op == NEG:
                a = (0 - a) & U32
        elif code == JMP | JA:
            pc += k
        elif code in COND_CODES:
            op, src = COND_CODES[code]
            s = x if src == X else k
            cond = {JEQ: a == s, JGT: a > s, JGE: a >= s, JSET: (a & s) != 0}[op]
            pc += jt if cond else jf
        elif code == RET | K:
            return k
        elif code == RET | A:
            return a
        elif code == MISC | TAX:
            x = a
        elif code == MISC | TXA:
            a = x
        else:
            raise AssertionError(code)
