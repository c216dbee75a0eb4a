"""gpd_bpf_filter on the device against the checker (tests/bpf_ref.py): `keep` and `ret` for every
packet, exact equality, nothing skipped.  The outputs of the raw C-ABI calls are carved from
buffers filled with 0xA5 whose entries after n must survive.

A wave takes 64 packets and a workgroup 4 waves, so the sizes at which the kernel takes another
path are 64 (a second wave) and 256 (a second workgroup); 1025 packets leave a one-lane wave.

On the input side the bounds are checked by reading the code (DevPkt::load reads the aligned
words that hold bytes bpf_step has already found inside the packet); the "ends_at_data_len"
layout documents the case: its last packet ends exactly at data_len, the device buffer ends at
round_up(data_len, 16) and the bytes in between are not zero.
"""
import ctypes as C
import os

import numpy as np
import pytest

import bpf_cases as BC
import bpf_ref as R
import golden_cases as G
import oracle_ref as O
import pcapwrite_ref as WR
from gopacket_amd import layers as L
from gopacket_amd import pcap
from gopacket_amd.batch import PacketBatch
from test_parity_gpu import ALL, _parser, assert_same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CAPTURES = ["test_dns.pcap", "test_ethernet.pcap", "test_loopback.pcap"]
GUARD = 64
LAYOUTS = ["dense", "shuffled", "ends_at_data_len"]
COUNTS = [1, 63, 64, 65, 1025]


def _mods():
    import torch
    from gopacket_amd import bpf as B
    from gopacket_amd import parser as P
    from gopacket_amd import pcapwrite as PW
    return torch, P, PW, B


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    twin = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(twin) if twin else a).cuda()


def _layout(packets, layout, seed=0):
    """The (data, wirelen) pairs' data as a PacketBatch in the layout."""
    pk = [d for d, _ in packets]
    b = PacketBatch.from_packets(pk, align=1)
    if layout == "shuffled":
        order = np.random.default_rng(seed).permutation(b.n)
        # the descriptors stay in packet order; the bytes lie in another
        shuffled = PacketBatch.from_packets([pk[i] for i in order], align=1)
        off = np.zeros(b.n, np.uint32)
        off[order] = shuffled.offset
        b = PacketBatch(shuffled.data, shuffled.data_len, off, b.caplen)
    if layout == "ends_at_data_len":
        lim = (b.data_len + 15) // 16 * 16
        data = b.data[:lim].copy()
        data[b.data_len:] = 0xEE  # bytes past data_len never influence a result
        b = PacketBatch(data, b.data_len, b.offset, b.caplen)
    for i in (0, b.n - 1):
        assert b.packet(i) == pk[i]
    return b


class Dev:
    """A batch with its wire lengths and a context on the device."""

    def __init__(self, packets, layout="dense", seed=0):
        torch, P, PW, B = _mods()
        self.packets = packets
        self.batch = b = _layout(packets, layout, seed)
        self.p = _parser()
        if layout == "ends_at_data_len":
            assert int(b.offset[-1]) + int(b.caplen[-1]) == b.data_len and len(b.data) == (b.data_len + 15) // 16 * 16
            self.db = P.DeviceBatch.from_tensors(_t(b.data), b.data_len, _t(b.offset), _t(b.caplen))
        else:
            self.db = P.DeviceBatch(b)
        self.wirelen = np.array([w for _, w in packets], np.uint32)
        self.d_wirelen = _t(self.wirelen)
        self._filters = {}

    def filter(self, prog):
        B = _mods()[3]
        key = tuple(prog)
        if key not in self._filters:
            self._filters[key] = B.NewBPFInstructionFilter(prog, self.p)
        return self._filters[key]

    def expect(self, prog, use_wirelen=True):
        ret = np.array([R.run(prog, d, w if use_wirelen else len(d)) for d, w in self.packets], np.uint32)
        return (ret != 0).astype(np.uint8), ret

    def raw(self, prog, use_wirelen=True, want_ret=True):
        """One gpd_bpf_filter through the C-ABI into guarded buffers: (keep, ret) as queued."""
        torch, P, PW, B = _mods()
        n = self.batch.n
        keep = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        ret = torch.full((n + GUARD,), -0x5A5A5A5B, dtype=torch.int32, device="cuda") if want_ret else None
        b = self.db.c_batch()
        rc = B.bpf_lib().gpd_bpf_filter(self.filter(prog).h, C.byref(b),
                                        C.c_void_p(self.d_wirelen.data_ptr()) if use_wirelen else None,
                                        C.c_void_p(keep.data_ptr()), C.c_void_p(ret.data_ptr()) if want_ret else None,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, B.bpf_lib().gpd_last_error_string()
        return keep, ret

    def check(self, prog, use_wirelen=True, want_ret=True, what=""):
        keep, ret = self.raw(prog, use_wirelen, want_ret)
        self.compare(prog, keep, ret, use_wirelen, what)

    def compare(self, prog, keep, ret, use_wirelen=True, what=""):
        n = self.batch.n
        wk, wr = self.expect(prog, use_wirelen)
        k = keep.cpu().numpy()
        bad = np.nonzero(k[:n] != wk)[0]
        assert len(bad) == 0, (what, "keep", int(bad[0]), self.packets[int(bad[0])][0].hex())
        assert (k[n:] == 0xA5).all(), (what, "a keep byte after entry n was written")
        if ret is not None:
            r = ret.cpu().numpy().view(np.uint32)
            bad = np.nonzero(r[:n] != wr)[0]
            assert len(bad) == 0, (what, "ret", int(bad[0]), int(r[bad[0]]), int(wr[bad[0]]))
            assert (r[n:] == 0xA5A5A5A5).all(), (what, "a ret word after entry n was written")


def _mixed_packets(n, seed):
    """The edge packets, then random ones: n (data, wirelen) pairs."""
    pk = BC.edge_packets() + BC.random_packets(seed, max(0, n - 5))
    pk = pk[:n]
    if n > 1:
        pk[-1] = (pk[-1][0] + b"\x45\x07\x09", pk[-1][1])  # the last packet is never empty
    return pk


SWEEP_PROGRAMS = ["port80", "ld_w_abs_0x10", "ld_w_ind_x0x1_k0x3", "ld_h_ind_x0x13_k0x0", "ldx_msh_0x4",
                  "mem_all_16", "mem_packet_dependent", "ld_len", "jump_255", "div_x", "ret_k"]


# ---- 1. device == checker: sizes and layouts -------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", COUNTS)
def test_sizes_and_layouts(n, layout):
    by_name = dict(BC.edge_programs())
    d = Dev(_mixed_packets(n, 100 + n), layout, seed=n)
    for name in SWEEP_PROGRAMS:
        d.check(by_name[name], what=name)
    d.check(by_name["port80"], use_wirelen=False, want_ret=False, what="port80, no wirelen, no ret")
    d.check(by_name["ld_len"], use_wirelen=False, what="ld_len, wirelen NULL = caplen")


def test_every_edge_program():
    """Each instruction form and edge, over the edge packets and 64 random ones, at every byte
    alignment of a packet's start (a dense layout of odd lengths)."""
    d = Dev(_mixed_packets(69, 7), "dense")
    for name, prog in BC.edge_programs():
        d.check(prog, what=name)


def test_loads_at_every_alignment():
    """A packet load reads the one or two aligned 32-bit words that hold its bytes: loads of every
    size around a 64-byte line's end, for every alignment of the packet's start mod 16."""
    rng = np.random.default_rng(31)
    packets = [(rng.integers(1, 256, 101, dtype=np.uint8).tobytes(), 101) for _ in range(33)]
    d = Dev(packets, "dense")
    assert {int(o) % 16 for o in d.batch.offset} == set(range(16))
    for sz in (R.W, R.H, R.B):
        for k in range(42, 68):
            d.check([(R.LD | sz | R.ABS, 0, 0, k), BC.RET_A], what=f"abs size {sz} k {k}")
        for k in (41, 45, 47, 50, 59, 61, 62, 63, 64, 97, 99):
            d.check([(R.LDX | R.IMM, 0, 0, 1), (R.LD | sz | R.IND, 0, 0, k), BC.RET_A], what=f"ind size {sz} k {k}")
    for k in (47, 48, 60, 63, 64, 100, 101):
        d.check([(R.LDX | R.B | R.MSH, 0, 0, k), (R.MISC | R.TXA, 0, 0, 0), BC.RET_A], what=f"msh {k}")


def test_random_programs():
    d = Dev(_mixed_packets(1025, 11), "shuffled", seed=3)
    for seed in range(20):
        d.check(BC.random_program(seed), what=f"random program {seed}")


def test_max_length_program():
    d = Dev(_mixed_packets(65, 12))
    prog = BC.max_length_program()
    d.check(prog, what="4095 x add, ret a")
    assert (d.expect(prog)[1] == 4095).all()
    # and one whose lanes return at its first and at its last instruction
    prog = [(R.LD | R.B | R.ABS, 0, 0, 0)] + [(R.ALU | R.ADD | R.K, 0, 0, 1)] * 4094 + [(R.RET | R.A, 0, 0, 0)]
    d.check(prog, what="ld, 4094 x add, ret a")


def test_descriptors_beyond_data_len_are_clamped():
    """offset and caplen clamped to the buffer, as gpd_decode reads a descriptor."""
    torch, P, PW, B = _mods()
    rng = np.random.default_rng(5)
    data_len = 100
    data = rng.integers(1, 256, 112, dtype=np.uint8)
    off = np.array([0, 90, 99, 100, 101, 0xFFFFFFF0, 50], np.uint32)
    cap = np.array([100, 20, 5, 1, 1, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    packets = []
    for o, c in zip(off, cap):
        o = min(int(o), data_len)
        c = min(int(c), data_len - o)
        packets.append((data[o:o + c].tobytes(), c))
    d = Dev(packets)
    d.batch = PacketBatch(data, data_len, off, cap)
    d.db = P.DeviceBatch.from_tensors(_t(data), data_len, _t(off), _t(cap))
    by_name = dict(BC.edge_programs())
    for name in ("ld_w_abs_0x10", "ld_b_abs_0x0", "ld_len", "ld_h_ind_x0x1_k0x3", "port80"):
        d.check(by_name[name], use_wirelen=False, what=name)


def test_empty_batch_and_refusals():
    torch, P, PW, B = _mods()
    p = _parser()
    f = B.NewBPFInstructionFilter(BC.PORT80, p)
    e = P.DeviceBatch(PacketBatch.from_packets([]))
    keep = f.match_device(e)
    assert keep.numel() == 0 and keep.dtype == torch.uint8
    b = e.c_batch()
    lib = B.bpf_lib()
    assert lib.gpd_bpf_filter(f.h, C.byref(b), None, None, None, None) == 0  # n == 0: a no-op
    one = P.DeviceBatch(PacketBatch.from_packets([BC.PACKET]))
    b = one.c_batch()
    assert lib.gpd_bpf_filter(f.h, C.byref(b), None, None, None, None) == -1  # null keep
    assert lib.gpd_bpf_filter(None, C.byref(b), None, None, None, None) == -1
    with pytest.raises(B.BPFError) as err:
        B.NewBPFInstructionFilter([(R.JMP | R.JA, 0, 0, 1), BC.ret_k(1)], p)
    assert "instruction 0 " in str(err.value)
    h = C.c_void_p()
    _, arr = B._c_program([BC.ret_k(1)])
    assert lib.gpd_bpf_create(p.ctx().h, arr, 0, C.byref(h)) == -1 and not h.value
    lib.gpd_bpf_destroy(None)


# ---- 2. divergence ---------------------------------------------------------------------------------
def _traffic(n, seed):
    """IPv4/TCP and IPv4/UDP to and from port 80 and elsewhere, with and without IP options,
    fragments, IPv6, ARP-sized runts and caplen-0 packets, mixed within every wave."""
    rng = np.random.default_rng(seed)
    base = bytearray(BC.PACKET + bytes(16))
    out = []
    for _ in range(n):
        kind = int(rng.integers(0, 10))
        p = bytearray(base)
        if kind == 0:
            pass                                   # tcp, dst port 80
        elif kind == 1:
            p[34:38] = b"\x00\x50\xc0\x01"          # tcp, src port 80
        elif kind == 2:
            p[36:38] = b"\x01\xbb"                  # tcp, port 443
        elif kind == 3:
            p[23] = 0x11                           # udp, port 80
        elif kind == 4:
            p[20:22] = b"\x00\x10"                  # a later fragment
        elif kind == 5:
            p[14] = 0x46                           # one word of IP options: the ports move by 4
            p[38:42] = b"\x12\x34\x00\x50"
        elif kind == 6:
            p = bytearray(b"\xff" * 12 + b"\x86\xdd" + bytes(rng.integers(0, 256, 40, dtype=np.uint8)))
        elif kind == 7:
            p = bytearray(b"\xff" * 12 + b"\x08\x06" + bytes(28))
        elif kind == 8:
            p = p[:int(rng.integers(1, 38))]       # cut anywhere
        else:
            p = bytearray()
        out.append((bytes(p), len(p)))
    return out


def test_divergence_port80():
    d = Dev(_traffic(1025, 21), "shuffled", seed=4)
    keep, _ = d.expect(BC.PORT80)
    for w in range(0, 1024, 64):  # every wave holds packets that match and packets that do not
        assert 0 < int(keep[w:w + 64].sum()) < 64
    d.check(BC.PORT80, what="port80")
    d.check(BC.UDP80, what="udp80")


# ---- 3. composition --------------------------------------------------------------------------------
def test_matches_feed_the_writer():
    torch, P, PW, B = _mods()
    d = Dev(_traffic(700, 22))
    f = d.filter(BC.PORT80)
    keep, ret = f.match_device(d.db, length=d.d_wirelen, want_ret=True)
    d.compare(BC.PORT80, torch.cat([keep, torch.full((GUARD,), 0xA5, dtype=torch.uint8, device="cuda")]), None)
    assert (ret.cpu().numpy().view(np.uint32) == d.expect(BC.PORT80)[1]).all()
    ts = np.arange(d.batch.n, dtype=np.uint64) * np.uint64(1000)
    stream, nw = PW.write_device(d.p, d.db, ts, None, keep, file_header=(262144, 1))
    mask = d.expect(BC.PORT80)[0]
    want, rn, _ = WR.write(d.batch, ts, None, mask, False, (262144, 1))
    assert nw == rn == int(mask.sum()) and nw > 50
    assert stream.cpu().numpy().tobytes() == want


def test_select_of_matches_decodes_like_the_oracle():
    torch, P, PW, B = _mods()
    from gopacket_amd.results import BatchResult
    pk = [G.case_bytes(c) for c in G.load()["cases"]] * 3
    packets = [(p, len(p)) for p in pk]
    d = Dev(packets)
    prog = [(R.LD | R.H | R.ABS, 0, 0, 12), (R.JMP | R.JEQ | R.K, 0, 1, 0x800), BC.ret_k(65535), BC.ret_k(0)]  # ip
    mask = d.expect(prog)[0]
    idx = np.nonzero(mask)[0]
    assert 0 < len(idx) < d.batch.n
    keep = d.filter(prog).match_device(d.db)
    sel, index = PW.select(d.p, d.db, keep)
    assert sel.n == len(idx) and (index.cpu().numpy() == idx).all()
    ref = O.decode(d.batch, L.LayerTypeEthernet, ALL, 0, ext=False, nthreads=8)
    sub = BatchResult(*[None if a is None else a[idx] for a in
                        (ref.status, ref.layers, ref.net_hash, ref.tp_hash, ref.csum, None, ref.hdr_off, None)])
    dres = P.DeviceResult(sel.n)
    d.p.decode_device(sel, dres)
    torch.cuda.synchronize()
    assert_same(dres.to_host(), sub, ext=False)


@pytest.mark.parametrize("name", CAPTURES)
def test_golden_capture_through_the_filter(name):
    """The capture's records as pcapgo reads them (data, CaptureInfo.Length), then the filter."""
    raw = open(os.path.join(HERE, "golden", name), "rb").read()
    p = pcap.index(pcap.capture_array(raw))
    assert p.err is None and p.batch.n > 0
    packets = [(p.batch.packet(i), int(p.length[i])) for i in range(p.batch.n)]
    d = Dev(packets)
    by_name = dict(BC.edge_programs())
    udp53 = list(BC.UDP80)
    udp53[8], udp53[10] = (0x15, 2, 0, 53), (0x15, 0, 1, 53)
    for what, prog in (("port80", BC.PORT80), ("udp port 53", udp53), ("ld_len", by_name["ld_len"]),
                       ("mem_packet_dependent", by_name["mem_packet_dependent"])):
        d.check(prog, what=what)
    if name == "test_dns.pcap":
        assert d.expect(udp53)[0].any()


# ---- 4. asynchrony ---------------------------------------------------------------------------------
def test_two_filters_back_to_back_on_one_stream():
    torch, P, PW, B = _mods()
    d = Dev(_traffic(1025, 23))
    f1, f2 = d.filter(BC.PORT80), d.filter(dict(BC.edge_programs())["mem_packet_dependent"])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the uploads above ran on the default stream)
    k1, r1 = f1.match_device(d.db, length=d.d_wirelen, stream=s, want_ret=True)
    k2, r2 = f2.match_device(d.db, length=d.d_wirelen, stream=s, want_ret=True)
    s.synchronize()
    for prog, k, r in ((BC.PORT80, k1, r1), (f2.instructions, k2, r2)):
        prog = [(i.Code, i.Jt, i.Jf, i.K) if hasattr(i, "Code") else i for i in prog]
        wk, wr = d.expect(prog)
        assert (k.cpu().numpy() == wk).all() and (r.cpu().numpy().view(np.uint32) == wr).all()
