"""Checksum arithmetic at its extremes: the frames, the batches and the checker
(tests/test_csum_extremes.py on the CPU, tests/test_csum_extremes_gpu.py on the device).

Every other payload byte in tests/ is uniformly random, so 16-bit words average 0x7FFF, running
sums stay far from 2^32, the second fold almost never carries and the (start, length) edge masks
are met by chance.  The families here are built so that each accumulator of the decode path
(DESIGN.md §6 "Checksum arithmetic at its extremes") reaches its bound, and every structural
property a family claims is asserted here, from the bytes, when the family is built.

The checker is plain Python over numpy byte sums (errpath_cases.ip4_checksum / l4_sum, restating
ip4.go:158-179 and tcpip.go:26-88 with Go's one uint32 wrap made explicit in _fold_not); the
expected checksum words of a family come from it, applied to the byte ranges the oracle's layer
records report, never from the library under test.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

import error_sites as ES
import errpath_cases as EC
import oracle_ref as O
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.batch import PAD, PacketBatch

ALL = 0xFFF  # every decoder (gpd.h GPD_DEC_ALL)
GAP = 0x5A   # the byte between frames of a gappy layout: no fill has it, so a mask that takes
             # one byte too many changes the sum

FILLS = {"00": b"\x00", "ff": b"\xff", "ff00": b"\xff\x00", "00ff": b"\x00\xff", "80": b"\x80"}
STORED = ("right", "zero", "ones")

SAT4 = dict(tos=0xFF, ident=0xFFFF, ttl=0xFF, flags_frag=0xC000, src=b"\xff" * 4, dst=b"\xff" * 4)
SAT6 = dict(tc_flow=0x0FFFFFFF, hlim=0xFF, src=b"\xff" * 16, dst=b"\xff" * 16)
SAT_TCP = dict(sport=0xFFFF, dport=0xFFFF, seq=0xFFFFFFFF, ack=0xFFFFFFFF, window=0xFFFF)
SAT_UDP = dict(sport=0xFFFF, dport=0xFFFF)


def fill(name: str, n: int, rng=None) -> bytes:
    if name == "rand":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    p = FILLS[name]
    return (p * (n // len(p) + 1))[:n]


# ---------------------------------------------------------------- the checker
def fold(s: int) -> int:
    """tcpipChecksum's fold (tcpip.go:66-69) of a sum Go holds in a uint32: the wrap, then the
    loop; the checksum is ~fold & 0xffff."""
    s &= 0xFFFFFFFF  # Go's uint32 dropped the rest while it accumulated
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def second_fold_carries(s: int) -> bool:
    """After one fold the value is still above 0xFFFF."""
    s &= 0xFFFFFFFF
    return (s >> 16) + (s & 0xFFFF) >= 0x10000


def le_sum(pkt: bytes, a: int, b: int, net_kind: str, net_off: int, proto: int) -> int:
    """The same words as errpath_cases.l4_sum, each byte-swapped: the little-endian-domain sum
    the fast decoders keep (gpd_dev_fast.h)."""
    def sw(x):
        a_ = np.frombuffer(bytes(x), np.uint8)
        return int(a_[0::2].sum(dtype=np.uint64)) + (int(a_[1::2].sum(dtype=np.uint64)) << 8)
    ps = sw(pkt[net_off + 12:net_off + 20]) if net_kind == "IPv4" else sw(pkt[net_off + 8:net_off + 40])
    n = b - a
    swap = lambda w: ((w & 0xFF) << 8) | (w >> 8)
    return ps + swap(proto) + swap(n & 0xFFFF) + swap(n >> 16) + sw(pkt[a:b])


def expected(batch: PacketBatch, ref):
    """(csum words, status bits 18-19) of every packet from the checker, over the ranges of the
    oracle's layer records (`ref` decoded with ext=True): the IPv4 object's Contents with bytes
    10-11 read as zero, and the last transport object's Contents + Payload under the pseudo-header
    of the last network object."""
    n = batch.n
    cs, bits = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i in range(n):
        pkt = batch.packet(i)
        st = int(ref.status[i])
        r4 = ref.layer(i, "IPv4")
        if r4 is not None and (r4[0][1] - r4[0][0]) % 2 == 0:  # (odd Contents: Go panics, no value)
            cs[i] |= EC.ip4_checksum(pkt[r4[0][0]:r4[0][1]])
            bits[i] |= 1 << 18
        tp, net = (st >> 24) & 15, (st >> 20) & 15
        if tp in (4, 5) and net in (1, 2):
            (c0, _), (_, p1) = ref.layer(i, "TCP" if tp == 4 else "UDP")
            kind = "IPv4" if net == 1 else "IPv6"
            (n0, _), _ = ref.layer(i, kind)
            cs[i] |= EC.l4_checksum(pkt, c0, p1, kind, n0, 6 if tp == 4 else 17) << 16
            bits[i] |= 1 << 19
    return cs, bits


# ---------------------------------------------------------------- frames
def l4_frame(v6: bool, proto: int, payload: bytes, tags: int = 0, sat: bool = False,
             stored: str = "zero", udp_length=None, ip_length=None, ihl: int = 5, opts: bytes = b"") -> bytearray:
    """Ethernet [Dot1Q]* (IPv4 | IPv6) (TCP | UDP) payload, the stored checksums as asked."""
    if proto == 6:
        l4 = ES.tcp(payload, **(SAT_TCP if sat else {}))
    else:
        l4 = ES.udp(payload, length=udp_length, **(SAT_UDP if sat else {}))
    if v6:
        l3, et = ES.ip6(l4, nh=proto, length=ip_length, **(SAT6 if sat else {})), 0x86DD
    else:
        l3, et = ES.ip4(l4, proto=proto, length=ip_length, ihl=ihl, opts=opts, **(SAT4 if sat else {})), 0x0800
    for k in range(tags):
        l3, et = struct.pack(">HH", 0xFFFF if sat else 100 + k, et) + l3, 0x8100
    f = bytearray(ES.eth(et, l3))
    store(f, 14 + 4 * tags, v6, proto, stored, 4 * ihl)
    return f


def l4_off(v6: bool, tags: int = 0, ihl: int = 5) -> int:
    return 14 + 4 * tags + (40 if v6 else 4 * ihl)


def store(f: bytearray, l3: int, v6: bool, proto: int, mode: str, hl4: int = 20) -> None:
    """Write the stored checksum fields of the frame: the checker's value over the frame as
    built ("right"), 0x0000 or 0xFFFF."""
    l4 = l3 + (40 if v6 else hl4)
    col = l4 + (16 if proto == 6 else 6)
    if mode == "right":
        f[col:col + 2] = b"\0\0"
        v = EC.l4_checksum(bytes(f), l4, len(f), "IPv6" if v6 else "IPv4", l3, proto)
        if not v6:
            f[l3 + 10:l3 + 12] = struct.pack(">H", EC.ip4_checksum(bytes(f[l3:l3 + hl4])))
    else:
        v = 0 if mode == "zero" else 0xFFFF
        if not v6:
            f[l3 + 10:l3 + 12] = struct.pack(">H", v)
    if col + 2 <= len(f):
        f[col:col + 2] = struct.pack(">H", v)


def place(frames, offsets) -> PacketBatch:
    """The frames at the given byte offsets of one buffer, GAP bytes between them."""
    offsets = np.asarray(offsets, np.int64)
    lens = np.fromiter((len(f) for f in frames), np.int64, len(frames))
    total = int((offsets + lens).max())
    data = np.full(total + PAD, GAP, np.uint8)
    data[total:] = 0
    for f, o in zip(frames, offsets):
        data[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    return PacketBatch(data, total, offsets.astype(np.uint32), lens.astype(np.uint32))


def packed(frames, lead: int = 0) -> PacketBatch:
    """Back to back from byte `lead` on."""
    lens = np.fromiter((len(f) for f in frames), np.int64, len(frames))
    return place(frames, lead + np.concatenate([[0], np.cumsum(lens[:-1])]))


class Family:
    """One batch and what the design says about it: `outside` marks the frames the straight-line
    decoder leaves to the generic one in every kernel (IPv4 options, hop-by-hop, header errors),
    `vxlan` those it decodes per window but not per tile."""

    def __init__(self, name, batch, outside=None, vxlan=None, notes=None):
        self.name, self.batch = name, batch
        z = np.zeros(batch.n, bool)
        self.outside = z.copy() if outside is None else np.asarray(outside, bool)
        self.vxlan = z.copy() if vxlan is None else np.asarray(vxlan, bool)
        self.notes = notes or {}
        assert len(self.outside) == batch.n and len(self.vxlan) == batch.n


# ---------------------------------------------------------------- the fast / generic split
# the tunings every family runs under (gpd_ctx_set_tuning)
TUNINGS = [
    ("auto", None),
    ("w4k_split", dict(window_bytes=4096, split=1)),
    ("w4k", dict(window_bytes=4096, split=0)),
    ("w4k_shifted", dict(window_bytes=4096, split=0, shift=1)),
    ("w8k", dict(window_bytes=8192, header_once=0)),
    ("w8k_once", dict(window_bytes=8192, header_once=1)),
    ("w8k_once_lds_prefix", dict(window_bytes=8192, header_once=1, reg_prefix=0)),
    ("rounds_w2", dict(header_once=2, waves_per_simd=2)),
    ("rounds_w3", dict(header_once=2, waves_per_simd=3)),
]


def kernel_of(batch: PacketBatch, tuning, records: bool):
    """(kernel, window bytes) a fast-eligible batch takes: gpd_runtime.cpp decode_launch and
    gpd_kernels.hip launch_fast."""
    t = dict(window_bytes=0, shift=-1, header_once=-1, split=-1)
    t.update(tuning or {})
    mean_slot = -(-batch.data_len // batch.n)
    stage = t["window_bytes"] or (4096 if mean_slot * 64 <= 4096 else 8192)
    shift = t["shift"] != 0 if t["shift"] >= 0 else mean_slot <= 96
    ho = t["header_once"] if t["header_once"] >= 0 else (2 if mean_slot > 160 and not shift else 0)
    if ho == 2:
        return "ro", 8192
    if stage == 4096 and t["split"] != 0 and records:
        return "sp", 4096
    if stage == 8192 and ho == 1:
        return "rs_ho", 8192
    return "rs", stage


def designed_fallback(fam: Family, tuning, records: bool):
    """How many packets of the family the design leaves to the generic decoder under a kernel
    (DESIGN.md §5): the frames outside the straight-line envelope; under the windowed kernels a
    frame longer than window - 15 bytes; under the split kernel a packet its tile's one 4 KiB
    window does not hold; under the round kernel every VXLAN frame; under the windowed
    header-once kernel the VXLAN frames of a window that holds 16 of them or fewer (a window:
    from the tile's first pending packet, rounded down to 16, every pending packet that ends
    within 8 KiB of it — gpd_dev_common.h plan_window)."""
    b = fam.batch
    kern, stage = kernel_of(b, tuning, records)
    fb = fam.outside.copy()
    ln = b.caplen.astype(np.int64)
    off = b.offset.astype(np.int64)
    if kern == "ro":
        fb |= fam.vxlan
    else:
        fb |= ln > stage - 15
    if kern == "rs_ho" and fam.vxlan.any():
        for t0 in range(0, b.n, 64):
            o, e, vx = off[t0:t0 + 64], (off + ln)[t0:t0 + 64], fam.vxlan[t0:t0 + 64]
            pend = e - o <= stage - 15
            while pend.any():
                base = int(o[pend][0]) & ~15
                inw = pend & (o >= base) & (e - base <= stage)
                if 0 < (inw & vx).sum() <= 16:
                    fb[t0:t0 + 64] |= inw & vx
                pend &= ~inw
    if kern == "sp":
        fixedw = b.data_len >= 63 * b.n
        for t0 in range(0, b.n, 64):
            t1 = min(t0 + 64, b.n)
            base = int(off[t0]) & ~15
            if fixedw:
                nbytes = min((b.data_len - base + 15) & ~15, 4096)
            else:
                el = int(off[t1 - 1] + ln[t1 - 1])
                nbytes = min((el - base + 15) & ~15, 4096) if el > base else 0
            fb[t0:t1] |= (off[t0:t1] < base) | (off[t0:t1] + ln[t0:t1] - base > nbytes)
    return int(fb.sum())


# ---------------------------------------------------------------- families
def _pseudo_saturated(f: bytes, v6: bool, tags: int) -> bool:
    l3 = 14 + 4 * tags
    return EC._words(f[l3 + 8:l3 + 40] if v6 else f[l3 + 12:l3 + 20]) == (16 if v6 else 4) * 0xFFFF


def fills(long: bool) -> Family:
    """Each fill under ordinary and under saturated headers (addresses, ports, TOS / traffic class,
    Id, TTL, Seq, Ack, Window all-ones), IPv4 and IPv6, TCP and UDP, untagged and tagged, even
    and odd payload lengths, the stored checksums right, 0x0000 and 0xFFFF; packed back to back,
    so the segments start at every alignment."""
    frames = []
    for name in FILLS:
        for sat in (False, True):
            for v6 in (False, True):
                for proto in (6, 17):
                    for tags in (0, 1):
                        for k, st in enumerate(STORED):
                            pl = (1443 if long else 36) + (k + tags) % 2
                            f = l4_frame(v6, proto, fill(name, pl), tags=tags, sat=sat, stored=st)
                            o = l4_off(v6, tags) + (20 if proto == 6 else 8)
                            assert bytes(f[o:]) == fill(name, pl)
                            assert _pseudo_saturated(bytes(f), v6, tags) == sat
                            frames.append(f)
    return Family("fills_long" if long else "fills_short", packed(frames))


def edge_masks() -> Family:
    """Eth [Dot1Q] IPv4 / IPv6, TCP and UDP, payloads of 0..48 bytes (head only, head + tail,
    head + middle + tail), each laid behind 0..15 gap bytes so that the transport segment starts
    at every address mod 16 for every length mod 16 — all 256 pairs per protocol and fill — with
    the 0x80, the 0xFF and a random fill."""
    rng = np.random.default_rng(0xC5E001)
    frames, offs, pos = [], [], 0
    for name in ("80", "ff", "rand"):
        for proto in (6, 17):
            pairs = set()
            for pl in range(49):
                for s in range(16):
                    v6, tags = bool((pl + s) & 1), ((pl + s) >> 1) & 1
                    f = l4_frame(v6, proto, fill(name, pl, rng), tags=tags, stored=STORED[(pl + s) % 3])
                    o = l4_off(v6, tags)
                    pos += (s - (pos + o)) % 16
                    pairs.add(((pos + o) % 16, (len(f) - o) % 16))
                    frames.append(f)
                    offs.append(pos)
                    pos += len(f)
            assert len(pairs) == 256, (name, proto, len(pairs))
    return Family("edge_masks", place(frames, offs))


BOUNDARIES = (16, 1024, 4096, 8192, 16384)


def boundaries(lead: int) -> Family:
    """Segments that end exactly on, one byte before and one byte after a multiple of 16 B,
    1 KiB, 4 KiB, 8 KiB and 16 KiB of their tile's run (counted from the tile's first 16-aligned
    byte, as ro_kernel's rounds and every kernel's chunks are), TCP and UDP, with the 0xFF,
    FF 00 and 0x80 fills; then the largest IPv4 segments.  Back to back from byte `lead` (0: the
    run starts aligned; 7: at an odd address)."""
    frames, marks, pos, t0 = [], [], lead, 0
    for name in ("ff", "ff00", "80"):
        for proto in (6, 17):
            for bnd in BOUNDARIES:
                for d in (-1, 0, 1):
                    if len(frames) % 64 == 0:
                        t0 = pos & ~15
                    h = 14 + 20 + (20 if proto == 6 else 8)
                    rel = pos + h + 2 - t0                      # the earliest end worth aiming at
                    end = -(-rel // bnd) * bnd + d
                    f = l4_frame(False, proto, fill(name, end - (pos + h - t0)), stored=STORED[len(frames) % 3])
                    marks.append((pos + len(f) - t0, bnd, d))
                    frames.append(f)
                    pos += len(f)
    for e, bnd, d in marks:
        assert (e - d) % bnd == 0
    assert {(bnd, d) for _, bnd, d in marks} == {(bnd, d) for bnd in BOUNDARIES for d in (-1, 0, 1)}
    frames.append(l4_frame(False, 6, fill("ff", 65495), stored="right"))
    frames.append(l4_frame(False, 17, fill("ff", 65507), stored="ones"))
    assert all(len(f) == 14 + 65535 for f in frames[-2:])
    return Family("boundaries_aligned" if lead == 0 else "boundaries_odd", packed(frames, lead))


FOLD_TARGETS = ("be_second_fold", "le_only", "be_only", "zero", "fold_0001", "fold_fffe")


def _fold_frame(v6, proto, pl, rest, target):
    """A frame under saturated headers whose last two payload bytes are searched so that the
    segment's sum meets `target`."""
    f = l4_frame(v6, proto, fill(rest, pl), sat=True, stored="ones")
    kind, l3, l4 = ("IPv6" if v6 else "IPv4"), 14, l4_off(v6)
    f[-2:] = b"\0\0"
    args = (l4, len(f), kind, l3, proto)
    s0, s0le = EC.l4_sum(bytes(f), *args), le_sum(bytes(f), *args)
    seg = len(f) - l4
    wa, wb = (256, 1) if (seg - 2) % 2 == 0 else (1, 256)  # weights of the two bytes in the BE sum
    a, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    s, sle = s0 + wa * a + wb * b, s0le + wb * a + wa * b
    carries = lambda x: (x >> 16) + (x & 0xFFFF) >= 0x10000
    ok = {"be_second_fold": carries(s), "le_only": carries(sle) & ~carries(s),
          "be_only": carries(s) & ~carries(sle), "zero": s % 0xFFFF == 0,
          "fold_0001": s % 0xFFFF == 1, "fold_fffe": s % 0xFFFF == 0xFFFE}[target]
    assert ok.any(), (v6, proto, pl, rest, target)
    k = int(np.argmax(ok))
    f[-2], f[-1] = k // 256, k % 256
    s, sle = EC.l4_sum(bytes(f), *args), le_sum(bytes(f), *args)
    assert s < 1 << 32 and sle < 1 << 32
    want = {"be_second_fold": second_fold_carries(s),
            "le_only": second_fold_carries(sle) and not second_fold_carries(s),
            "be_only": second_fold_carries(s) and not second_fold_carries(sle),
            "zero": fold(s) == 0xFFFF and EC.l4_checksum(bytes(f), *args) == 0x0000,
            "fold_0001": fold(s) == 0x0001 and EC.l4_checksum(bytes(f), *args) == 0xFFFE,
            "fold_fffe": fold(s) == 0xFFFE and EC.l4_checksum(bytes(f), *args) == 0x0001}[target]
    assert want, (v6, proto, pl, rest, target, hex(s), hex(sle))
    return f


def folds() -> Family:
    """Sums chosen by their last two payload bytes: the second fold of the big-endian sum
    carries; that of the byte-swapped sum carries and the big-endian one's does not, and the
    reverse; a multiple of 0xFFFF (checksum 0x0000); folded values 0x0001 and 0xFFFE.  IPv4 and
    IPv6, TCP and UDP, even and odd lengths, each at an even and at an odd segment address."""
    frames, offs, pos = [], [], 0
    for rest in ("00", "ff", "80"):
        for v6 in (False, True):
            for proto in (6, 17):
                for pl in (32, 33):
                    for target in FOLD_TARGETS:
                        f = _fold_frame(v6, proto, pl, rest, target)
                        for parity in (0, 1):
                            pos += (parity - (pos + l4_off(v6))) % 2
                            frames.append(f)
                            offs.append(pos)
                            pos += len(f)
    starts = {(o + (54 if f[12:14] == b"\x86\xdd" else 34)) % 2 for f, o in zip(frames, offs)}
    assert starts == {0, 1}
    return Family("folds", place(frames, offs))


def _wrap_tile(t0: int):
    """64 back-to-back frames from the 16-aligned byte t0 on: three 65,535-byte IPv4 datagrams
    of 0xFF take the running sum of the tile's 16-bit words past 2^32, with a short segment
    before the wrap, one across it, short and long ones after it at even and odd addresses and a
    150-byte segment whose first 128 frame bytes end a round while its tail lies in the next.
    Returns (frames, roles): roles[i] names what frame i is there for."""
    frames, roles, pos = [], [], t0

    def add(f, role=None):
        nonlocal pos
        frames.append(f)
        roles.append(role)
        pos += len(f)

    add(l4_frame(False, 6, fill("ff", 65495), stored="right"))
    add(l4_frame(False, 6, fill("ff", 100), stored="zero"), "before")
    add(l4_frame(False, 17, fill("ff", 65507), stored="ones"), "across")  # (2^32 falls in its last KiB)
    add(l4_frame(False, 17, fill("ff", 65507), stored="zero"), "after")
    add(l4_frame(False, 6, fill("ff", 30000), stored="right"), "after")
    for k, (proto, name, pl) in enumerate(((17, "80", 20), (6, "ff", 21), (6, "ff00", 9001), (17, "00ff", 9000),
                                           (17, "ff", 33), (6, "ff", 17), (6, "ff", 8200), (17, "ff", 8301),
                                           (6, "80", 64), (17, "ff", 63), (6, "ff", 1447), (17, "ff00", 12001))):
        add(l4_frame(False, proto, fill(name, pl), stored=STORED[k % 3]), "after")
    # the pending tail: frame bytes [0, 128) end the round at `edge`, the segment ends 74 bytes on
    edge = -(-(pos - t0 + 54 + 1 + 130) // 8192) * 8192 + t0
    add(l4_frame(False, 6, fill("ff", edge - 130 - pos - 54), stored="right"))
    assert pos == edge - 130
    add(l4_frame(False, 6, fill("ff", 150), stored="right"), "pending")
    k = 0
    while len(frames) < 64:
        add(l4_frame(bool(k & 1), 6 if k % 3 else 17, fill(("ff", "80", "ff00")[k % 3], 600 + 37 * k), tags=k & 1,
                     stored=STORED[k % 3]), "after")
        k += 1
    return frames, roles


def _assert_wrap(batch: PacketBatch, first: int, roles) -> None:
    """The running sums ro_kernel keeps for the tile that starts at packet `first`, from the bytes:
    G[c] = the sum of the 16-bit words of the run's first c 16-byte chunks (exact, uint64)."""
    n = len(roles)
    off = batch.offset[first:first + n].astype(np.int64)
    ln = batch.caplen[first:first + n].astype(np.int64)
    t0 = int(off[0])
    assert t0 % 16 == 0 and np.array_equal(off[1:], (off + ln)[:-1]), "64 contiguous frames, 16-aligned"
    end = int(off[-1] + ln[-1])
    run = np.zeros((end - t0 + 15) // 16 * 16, np.uint8)
    run[:end - t0] = batch.data[t0:end]
    words = run.view("<u2").astype(np.uint64).reshape(-1, 8).sum(axis=1)
    G = np.concatenate([np.zeros(1, np.uint64), np.cumsum(words)])
    seen = set()
    for i, role in enumerate(roles):
        if role is None:
            continue
        S = int(off[i]) - t0 + 34 + (4 if batch.data[off[i] + 12] == 0x81 else 0) + \
            (20 if batch.data[off[i] + 12 + (4 if batch.data[off[i] + 12] == 0x81 else 0)] == 0x86 else 0)
        E = int(off[i] + ln[i]) - t0
        A, B = (S + 15) // 16, E // 16
        if role == "before":
            assert G[B] < 1 << 32
        elif role == "across":
            assert G[A] < 1 << 32 <= G[B]
        else:
            assert G[A] >= 1 << 32, (i, role)
            seen.add((E - S >= 8192, S & 1))
        if role == "pending":
            hdr_round = (int(off[i]) - t0 + 127) // 8192
            assert E - S < 8192 and hdr_round < (B * 16) // 8192, "its tail's chunk lies in a later round"
    if n == 64:
        assert seen >= {(False, 0), (False, 1), (True, 0), (True, 1)}, seen
    assert {r for r in roles if r} >= {"before", "across", "after", "pending"}


def prefix_wrap(mixed: bool) -> Family:
    """ro_kernel's running prefix past 2^32.  Alone: one such tile.  Mixed: an IMIX tile, the wrap
    tile, an IMIX tile, and the wrap tile's first 40 frames as the batch's last, partial tile;
    every tile starts 16-aligned."""
    frames, offs, pos, tiles = [], [], 0, []
    imix = synth.make_imix(128, seed=0xC5E002)

    def tile(fs):
        nonlocal pos
        pos = (pos + 15) & ~15
        for f in fs:
            frames.append(f)
            offs.append(pos)
            pos += len(f)

    if mixed:
        tile([imix.packet(i) for i in range(64)])
    wf, roles = _wrap_tile((pos + 15) & ~15)
    tiles.append((len(frames), roles))
    tile(wf)
    if mixed:
        tile([imix.packet(i) for i in range(64, 128)])
        wf, roles = _wrap_tile((pos + 15) & ~15)
        tiles.append((len(frames), roles[:40]))
        tile(wf[:40])
    b = place(frames, offs)
    for first, roles in tiles:
        assert first % 64 == 0
        _assert_wrap(b, first, roles)
    return Family("prefix_wrap_mixed" if mixed else "prefix_wrap_alone", b)


def ip4_headers() -> Family:
    """IPv4 headers of IHL 5..15 whose option words are one record-route-like TLV of 0xFF bytes
    (after a NOP on every other frame), every fixed field all-ones, the header checksum right,
    0x0000 and 0xFFFF; then the sizes at which the reference stops: IHL*4 beyond Length and
    beyond the capture."""
    frames, outside = [], []
    k = 0
    for rest in ("ff", "80", "00"):
        for ihl in range(5, 16):
            for proto in (6, 17):
                for st in STORED:
                    n = 4 * (ihl - 5)
                    if n == 0:
                        opts = b""
                    elif k % 2:
                        opts = b"\x01" + bytes([7, n - 1]) + b"\xff" * (n - 3)
                    else:
                        opts = bytes([7, n]) + b"\xff" * (n - 2)
                    k += 1
                    l4 = ES.tcp(fill(rest, 32), **SAT_TCP) if proto == 6 else ES.udp(fill(rest, 33), **SAT_UDP)
                    f = bytearray(ES.eth(0x0800, ES.ip4(l4, proto=proto, ihl=ihl, opts=opts, **SAT4)))
                    store(f, 14, False, proto, st, 4 * ihl)
                    assert len(opts) == n and bytes(f[14 + 20:14 + 4 * ihl]).count(0xFF) >= n - 3
                    assert f[15] == 0xFF and f[18:20] == b"\xff\xff" and f[22] == 0xFF and f[26:34] == b"\xff" * 8
                    frames.append(f)
                    outside.append(ihl != 5)
    for ihl in range(6, 16):  # (as test_parity_gpu._ip4_option_frames has them)
        n = 4 * (ihl - 5)
        opts = bytes([7, n]) + b"\xff" * (n - 2)
        for short in (0, n - 1):
            f = bytearray(ES.eth(0x0800, ES.ip4(ES.tcp(fill("ff", 32)), ihl=ihl, opts=opts, length=20 + short, **SAT4)))
            frames.append(f)
            outside.append(True)
            f = bytearray(ES.eth(0x0800, ES.ip4(ES.tcp(fill("ff", 32)), ihl=ihl, opts=opts, **SAT4)))
            frames.append(f[:14 + 20 + short])
            outside.append(True)
    return Family("ip4_headers", PacketBatch.from_packets(frames, align=1), outside=outside)


def trailers_cuts() -> Family:
    """Length under the capture: 1..17 trailing 0xFF bytes behind the IP length that must not be
    summed, and a UDP Length 1..17 under and over the IP payload.  Capture under the length: the
    segment cut at every residue mod 16."""
    frames = []
    k = 0
    for v6 in (False, True):
        for proto in (6, 17):
            for t in range(1, 18):
                frames.append(l4_frame(v6, proto, fill("80", 40), stored=STORED[k % 3]) + b"\xff" * t)
                k += 1
            for r in range(16):
                f = l4_frame(v6, proto, fill("ff", 48), stored=STORED[k % 3])
                frames.append(f[:l4_off(v6) + (20 if proto == 6 else 8) + 16 + r])
                k += 1
        for t in range(1, 18):
            for sign in (-1, 1):
                f = l4_frame(v6, 17, fill("ff", 40), udp_length=48 + sign * t, stored="zero")
                frames.append(f)
    return Family("trailers_cuts", PacketBatch.from_packets(frames, align=1))


JUMBO_SIZES = (65536, 131070, 196608)


def jumbo_frame(proto: int, payload: bytes) -> bytes:
    """Eth / IPv6 (Length 0) / hop-by-hop with the jumbo payload option / transport bytes, as the
    ipv6_jumbogram_dlp golden case is laid out (ip6.go:230-262).  A DecodingLayerParser's IPv6
    keeps the hop-by-hop header in its Payload and names the header after it as the next layer
    (ip6.go:253-262,280-285), so the transport decoder reads the eight hop-by-hop bytes as the
    start of its own header — the golden case ends in "Invalid TCP data offset 0 < 5" for that
    reason.  The TCP frames here are therefore a TCP header without its first eight bytes: the
    hop-by-hop bytes stand for the ports and Seq, the data offset behind them is 5, and the
    segment ComputeChecksum() sums is the whole jumbo payload, hop-by-hop bytes included, with
    length >> 16 in its pseudo-header.  UDP reads the jumbo length's high half as its Length
    (1..3: "UDP packet too small"), so a UDP jumbogram never has a checksum in the reference."""
    rest = ES.tcp(payload)[8:] if proto == 6 else ES.udp(payload, length=0)
    hbh = bytes([proto, 0, 0xC2, 4]) + struct.pack(">I", 8 + len(rest))
    return ES.eth(0x86DD, ES.ip6(hbh + rest, nh=0, length=0))


def jumbograms() -> Family:
    """IPv6 jumbograms of 0xFF and FF 00: 65,536 payload bytes, 131,070 (65,535 words of 0xFFFF:
    just below Go's uint32 wrap) and 196,608 (past it), TCP and (stopping at its decoder) UDP.
    The generic decoder's 256 E + O must wrap exactly as Go's accumulator does, and no fast path
    may fold such a segment in the little-endian domain."""
    frames = []
    for proto in (6, 17):
        for name in ("ff", "ff00"):
            for size in JUMBO_SIZES:
                f = jumbo_frame(proto, fill(name, size))
                s = EC.l4_sum(f, 54, len(f), "IPv6", 14, proto)
                assert (len(f) - 54) >> 16, "the length >> 16 term is live"
                if size == JUMBO_SIZES[0]:
                    assert s < 1 << 32
                if size == JUMBO_SIZES[-1]:
                    assert s > 1 << 32, "the unreduced sum passes 2^32"
                frames.append(f)
    return Family("jumbograms", PacketBatch.from_packets(frames), outside=np.ones(len(frames), bool))


def vxlan_inner() -> Family:
    """Config 4's shape (Eth / IPv4 / UDP 4789 / VXLAN / Eth / IP / TCP | UDP, about 128 bytes)
    whose inner payloads take every fill at lengths 0..48; once at 16-aligned offsets and once
    packed back to back (odd offsets)."""
    frames = []
    k = 0
    for name in FILLS:
        for proto in (6, 17):
            for pl in range(49):
                inner = l4_frame(pl % 5 == 4, proto, fill(name, pl), stored=STORED[k % 3], sat=(k % 7 == 3))
                k += 1
                u = ES.udp(b"\x08\x00\x00\x00\x00\x12\x34\x00" + bytes(inner), sport=40001, dport=4789)
                frames.append(ES.eth(0x0800, ES.ip4(u, proto=17)))
    a = PacketBatch.from_packets(frames, align=16)
    offs = list(a.offset.astype(np.int64))
    pos = a.data_len + 3
    for f in frames:
        offs.append(pos)
        pos += len(f)
    assert {o % 2 for o in offs[len(frames):]} == {0, 1}
    return Family("vxlan_inner", place(frames * 2, offs), vxlan=np.ones(2 * len(frames), bool))


BUILDERS = {
    "fills_short": lambda: fills(False), "fills_long": lambda: fills(True), "edge_masks": edge_masks,
    "boundaries_aligned": lambda: boundaries(0), "boundaries_odd": lambda: boundaries(7), "folds": folds,
    "prefix_wrap_alone": lambda: prefix_wrap(False), "prefix_wrap_mixed": lambda: prefix_wrap(True),
    "ip4_headers": ip4_headers, "trailers_cuts": trailers_cuts, "jumbograms": jumbograms,
    "vxlan_inner": vxlan_inner,
}
NAMES = tuple(BUILDERS)
# the families whose frames all fit a 4 KiB window / the ones with frames of 1.4 KB and more
SHORT = ("fills_short", "edge_masks", "folds", "ip4_headers", "trailers_cuts", "vxlan_inner")
LONG = ("fills_long", "boundaries_aligned", "boundaries_odd", "prefix_wrap_alone", "prefix_wrap_mixed")


@functools.lru_cache(maxsize=None)
def family(name: str) -> Family:
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(the oracle's decode with layer records, the checker's csum words, its status bits 18-19)
    of a family: computed once, shared by the tests, never changed by them."""
    b = family(name).batch
    ref = O.decode(b, L.LayerTypeEthernet, ALL, 0, ext=True, nthreads=8)
    cs, bits = expected(b, ref)
    return ref, cs, bits
