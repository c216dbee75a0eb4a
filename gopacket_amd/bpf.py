"""BPF filtering (the filter step of every gopacket pipeline): a classic BPF program over a
DeviceBatch, giving the `keep` mask pcapwrite.write_device and pcapwrite.select take.

The reference hands BPF programs to libpcap: pcap.NewBPFInstructionFilter and (*BPF).Matches
(pcap/pcap.go:553-583, pcap/pcap_unix.go:342-352), Handle.SetBPFInstructionFilter
(pcap/pcap.go:465-514), afpacket.TPacket.SetBPF, pcapgo.EthernetHandle.SetBPF.  Here the packets
are a batch in HBM and the virtual machine runs there, one packet per lane (gpd_bpf_filter,
include/gpd_bpf.h, which states the machine's rules); Matches runs the same interpreter on the
host for one packet.  Programs come as instructions — `tcpdump -dd` output through parse_dd, the
form pcap.go:465-493 tells users to paste.  Compiling a filter expression is libpcap's compiler,
which is not here: NewBPF and CompileBPFFilter raise.

The entry points are bound onto the loaded library here, on first use, from BPF_EXPORTS: they
live in their own header and are not part of _lib.EXPORTS.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import GpdBatch, check

MaxBpfInstructions = 4096  # pcap/pcap.go:36

# linux/bpf_common.h, linux/filter.h
BPF_LD, BPF_LDX, BPF_ST, BPF_STX, BPF_ALU, BPF_JMP, BPF_RET, BPF_MISC = range(8)
BPF_W, BPF_H, BPF_B = 0x00, 0x08, 0x10
BPF_IMM, BPF_ABS, BPF_IND, BPF_MEM, BPF_LEN, BPF_MSH = 0x00, 0x20, 0x40, 0x60, 0x80, 0xA0
BPF_ADD, BPF_SUB, BPF_MUL, BPF_DIV, BPF_OR, BPF_AND = 0x00, 0x10, 0x20, 0x30, 0x40, 0x50
BPF_LSH, BPF_RSH, BPF_NEG, BPF_MOD, BPF_XOR = 0x60, 0x70, 0x80, 0x90, 0xA0
BPF_JA, BPF_JEQ, BPF_JGT, BPF_JGE, BPF_JSET = 0x00, 0x10, 0x20, 0x30, 0x40
BPF_K, BPF_X, BPF_A = 0x00, 0x08, 0x10
BPF_TAX, BPF_TXA = 0x00, 0x80
BPF_MEMWORDS = 16


class GpdBpfInsn(C.Structure):
    _fields_ = [("code", C.c_uint16), ("jt", C.c_uint8), ("jf", C.c_uint8), ("k", C.c_uint32)]


BPF_EXPORTS = {
    # include/gpd_bpf.h — name: (restype, argtypes)
    "gpd_bpf_validate": (C.c_int, [C.POINTER(GpdBpfInsn), C.c_uint32]),
    "gpd_bpf_create": (C.c_int, [C.c_void_p, C.POINTER(GpdBpfInsn), C.c_uint32, C.POINTER(C.c_void_p)]),
    "gpd_bpf_destroy": (None, [C.c_void_p]),
    "gpd_bpf_filter": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "gpd_bpf_run_host": (C.c_uint32, [C.POINTER(GpdBpfInsn), C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32]),
}

_bound = False


def bpf_lib():
    """The loaded library with the filter entry points' signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in BPF_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


class BPFError(ValueError):
    """A program the validator refuses; the text names the instruction and the reason."""


@dataclass(frozen=True)
class BPFInstruction:
    """pcap.BPFInstruction (pcap/pcap.go:113-119)."""
    Code: int
    Jt: int
    Jf: int
    K: int


def _c_program(instructions):
    ins = [i if isinstance(i, BPFInstruction) else BPFInstruction(*i) for i in instructions]
    arr = (GpdBpfInsn * max(1, len(ins)))()
    for j, i in enumerate(ins):
        if not (0 <= i.Code <= 0xFFFF and 0 <= i.Jt <= 0xFF and 0 <= i.Jf <= 0xFF and 0 <= i.K <= 0xFFFFFFFF):
            raise BPFError(f"instruction {j} {i!r}: a field does not fit its width (u16, u8, u8, u32)")
        arr[j] = GpdBpfInsn(i.Code, i.Jt, i.Jf, i.K)
    return ins, arr


def validate(instructions) -> None:
    """gpd_bpf_validate: raises BPFError for a program the machine refuses (no device)."""
    ins, arr = _c_program(instructions)
    if bpf_lib().gpd_bpf_validate(arr, len(ins)) != 0:
        raise BPFError(_lib.lib.gpd_last_error_string().decode())


_DD_LINE = re.compile(r"^\{\s*(0x[0-9a-fA-F]+|\d+)\s*,\s*(0x[0-9a-fA-F]+|\d+)\s*,\s*(0x[0-9a-fA-F]+|\d+)\s*,"
                      r"\s*(0x[0-9a-fA-F]+|\d+)\s*\}\s*,?$")


def parse_dd(text: str) -> list:
    """`tcpdump -dd` output — lines of `{ 0x28, 0, 0, 0x0000000c },` — as BPFInstructions."""
    out = []
    for no, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line:
            continue
        m = _DD_LINE.match(line)
        if not m:
            raise ValueError(f"parse_dd: line {no} is not `{{ code, jt, jf, k }},`: {line!r}")
        code, jt, jf, k = (int(g, 0) for g in m.groups())
        if code > 0xFFFF or jt > 0xFF or jf > 0xFF or k > 0xFFFFFFFF:
            raise ValueError(f"parse_dd: line {no}: a field does not fit its width: {line!r}")
        out.append(BPFInstruction(code, jt, jf, k))
    return out


def format_dd(instructions) -> str:
    """The inverse of parse_dd, in tcpdump's own spelling."""
    return "".join(f"{{ 0x{i.Code:x}, {i.Jt}, {i.Jf}, 0x{i.K:08x} }},\n" for i in instructions)


class BPF:
    """pcap.BPF (pcap/pcap.go:553-583) on a device context."""

    def __init__(self, instructions, parser_or_ctx, orig: str = "BPF Instruction Filter"):
        from .pcapwrite import _ctx_handle
        self.instructions, self._prog = _c_program(instructions)
        self.orig = orig
        self._keep_alive = parser_or_ctx  # the filter must go before its context
        self.h = None
        if parser_or_ctx is None:  # a host-only filter: Matches and run, no device
            validate(self.instructions)
            self.device = None
            return
        ctx = parser_or_ctx.ctx() if hasattr(parser_or_ctx, "ctx") else parser_or_ctx
        self.device = ctx.device
        h = C.c_void_p()
        rc = bpf_lib().gpd_bpf_create(_ctx_handle(parser_or_ctx), self._prog, len(self.instructions), C.byref(h))
        if rc == _lib.GPD_ERR_INVALID:
            raise BPFError(_lib.lib.gpd_last_error_string().decode())
        check(rc, "gpd_bpf_create")
        self.h = h

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            _lib.lib.gpd_bpf_destroy(h)
            self.h = None

    def String(self) -> str:
        """pcap/pcap.go:576-578."""
        return self.orig

    def run(self, data: bytes, length=None) -> int:
        """The program's return value for one host packet (gpd_bpf_run_host)."""
        data = bytes(data)
        return bpf_lib().gpd_bpf_run_host(self._prog, len(self.instructions), data, len(data),
                                          len(data) if length is None else int(length) & 0xFFFFFFFF)

    def Matches(self, ci, data: bytes) -> bool:
        """pcap/pcap.go:581-583 for one host packet: caplen = len(data), len = ci.Length."""
        return self.run(data, None if ci is None else ci.Length) != 0

    def match_device(self, dbatch, length=None, stream=None, want_ret: bool = False):
        """`keep[i] = Matches(ci[i], data[i])` over a DeviceBatch (gpd_bpf_filter): a uint8 device
        tensor of 1 / 0, which pcapwrite.write_device(keep=...) and pcapwrite.select take as is.
        length (CaptureInfo.Length; None: the capture length) is a torch device tensor or a numpy
        array.  The call is queued on `stream` (None: the current one) and does not wait.  With
        want_ret, returns (keep, the programs' return values as an int32 tensor holding the
        uint32 bits)."""
        if self.h is None:
            raise RuntimeError("BPF.match_device: the filter was made without a parser or context")
        from .parser import _torch
        from .pcapwrite import _dev, _ptr
        torch = _torch()
        dev, n = dbatch.device, dbatch.n
        tdev = torch.device("cuda", dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        wl = _dev(length, np.uint32, dev, n, "length")
        with torch.cuda.stream(s):  # (the outputs' allocations belong to the stream that writes them)
            keep = torch.empty(n, dtype=torch.uint8, device=tdev)
            ret = torch.empty(n, dtype=torch.int32, device=tdev) if want_ret else None
        b = dbatch.c_batch()
        check(bpf_lib().gpd_bpf_filter(self.h, C.byref(b), _ptr(wl), _ptr(keep), _ptr(ret),
                                       C.c_void_p(s.cuda_stream)), "gpd_bpf_filter")
        return (keep, ret) if want_ret else keep


def NewBPFInstructionFilter(instructions, parser_or_ctx) -> BPF:
    """pcap.NewBPFInstructionFilter (pcap/pcap.go:553-570): `parser_or_ctx` is the
    DecodingLayerParser (or its context) whose device the filter runs on; None gives a filter
    for host packets only (Matches, run)."""
    return BPF(instructions, parser_or_ctx)


_NO_COMPILER = ("compiling the filter expression %r needs libpcap's compiler, which is not part of this "
                "package: compile it elsewhere (`tcpdump -dd %s`) and pass the instructions to "
                "NewBPFInstructionFilter(parse_dd(text), parser)")


def NewBPF(expr: str, *args, **kwargs):
    """pcap.NewBPF (pcap/pcap.go:520-551): not available, see the module text."""
    raise NotImplementedError(_NO_COMPILER % (expr, expr))


def CompileBPFFilter(expr: str, *args, **kwargs):
    """pcap.CompileBPFFilter (pcap/pcap.go:434-452): not available, see the module text."""
    raise NotImplementedError(_NO_COMPILER % (expr, expr))
