"""Shared inputs of the connection tracker's GPU tests (tests/test_tcptrack_gpu.py) and of
tools/tcptrack_time.py: Eth/IPv4/TCP frames built in bulk from arrays, generated connections that
reach every FSM state, and the size case.  Host only (numpy)."""
import numpy as np

import tcptrack_ref as TR
from gopacket_amd import synth
from gopacket_amd.batch import PacketBatch

FIN, SYN, RST, PSH, ACK = TR.FIN, TR.SYN, TR.RST, TR.PSH, TR.ACK
TCP, UDP, CUT = 0, 1, 2  # a packet's kind: tracked; UDP (keyed, not TCP); cut inside the IPv4 header (no key)
SLOT = 64                # bytes per packet in the batch; frames are 60 bytes (54 of headers, Ethernet padding)

_TEMPLATE = np.frombuffer(synth.tcp_frame(bytes(4), bytes(4), 0, 0, 1, ack=1, flags=ACK, pad_to=60), np.uint8)
assert len(_TEMPLATE) == 60 and _TEMPLATE[23] == 6 and _TEMPLATE[47] == ACK


def frames(src, dst, sport, dport, flags, kind=None):
    """One 60-byte Eth/IPv4/TCP frame per entry: IPv4 addresses as uint32, ports, the flag byte
    (TCP header byte 13).  kind (None: all TCP): UDP turns the protocol to 17 (the ports stay where
    they are), CUT captures 20 bytes only.  The IPv4 checksum is valid; the TCP checksum is not
    recomputed (the decoders do not drop on it)."""
    src, dst = np.asarray(src, np.uint32), np.asarray(dst, np.uint32)
    n = len(src)
    a = np.zeros((n, SLOT), np.uint8)
    a[:, :60] = _TEMPLATE
    for k in range(4):
        a[:, 26 + k] = (src >> np.uint32(24 - 8 * k)) & np.uint32(0xFF)
        a[:, 30 + k] = (dst >> np.uint32(24 - 8 * k)) & np.uint32(0xFF)
    sport, dport = np.asarray(sport, np.uint32), np.asarray(dport, np.uint32)
    a[:, 34], a[:, 35], a[:, 36], a[:, 37] = sport >> 8, sport & 0xFF, dport >> 8, dport & 0xFF
    a[:, 47] = np.asarray(flags, np.uint8)
    caplen = np.full(n, 60, np.uint32)
    if kind is not None:
        kind = np.asarray(kind)
        a[kind == UDP, 23] = 17
        a[kind == UDP, 38:40] = (0, 26)  # UDP Length: the header and the 18 bytes behind it
        caplen[kind == CUT] = 20
    a[:, 24:26] = 0
    w = a[:, 14:34].astype(np.uint32)
    s = ((w[:, 0::2] << 8) | w[:, 1::2]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
    a[:, 24], a[:, 25] = s >> 8, s & 0xFF
    return PacketBatch.from_arrays(a.reshape(-1), np.arange(n, dtype=np.uint32) * SLOT, caplen, data_len=n * SLOT)


class Packets:
    """Parallel lists of packets: endpoints, flags, kind; `batch()` builds the frames and
    `keys()` the model's keys (None for what the tracker does not track by kind)."""

    def __init__(self):
        self.src, self.dst, self.sport, self.dport, self.flags, self.kind = [], [], [], [], [], []

    def add(self, src, dst, sport, dport, flags, kind=TCP):
        for lst, v in zip((self.src, self.dst, self.sport, self.dport, self.flags, self.kind),
                          (src, dst, sport, dport, flags, kind)):
            lst.append(v)

    def __len__(self):
        return len(self.src)

    def batch(self, lo=0, hi=None):
        sl = slice(lo, hi)
        return frames(self.src[sl], self.dst[sl], self.sport[sl], self.dport[sl], self.flags[sl], self.kind[sl])

    def keys(self, lo=0, hi=None):
        hi = len(self) if hi is None else hi
        return [(self.src[i], self.dst[i], self.sport[i], self.dport[i]) if self.kind[i] == TCP else None
                for i in range(lo, hi)]


# One life of a connection that visits every state but Reset and ends Closed: (flags, from the server?)
LIFE = [(SYN, 0), (SYN | ACK, 1), (ACK, 0), (PSH | ACK, 0), (ACK, 1), (PSH | ACK, 1), (FIN | ACK, 0), (FIN | ACK, 1),
        (ACK, 0)]
ALPHABET = [SYN, SYN | ACK, ACK, ACK, PSH | ACK, FIN | ACK, FIN | ACK, FIN, RST, RST | ACK, 0, SYN | FIN]


def endpoints(j):
    """Connection j's client and server (address, port)."""
    return (0x0A000000 + j, 1024 + j % 60000), (0xC0A80000 + j % 251, 80 + j % 3)


def gen_connections(seed, nconn, max_len=40):
    """nconn scripts of 1..max_len (flags, from_server) packets: lives of LIFE, cut short, started
    mid-stream, with packets replaced from a weighted alphabet and directions flipped, so that
    every state, every rejection and the SupportMissingEstablishment guesses occur."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nconn):
        n = int(rng.integers(1, max_len + 1))
        start = int(rng.integers(0, len(LIFE))) if rng.random() < 0.3 else 0
        script = []
        k = start
        while len(script) < n:
            fl, srv = LIFE[k % len(LIFE)]
            r = rng.random()
            if r < 0.12:
                fl = ALPHABET[int(rng.integers(len(ALPHABET)))]
            elif r < 0.18:
                srv ^= 1
            elif r < 0.22:
                k += 1  # a packet lost
            if fl & ACK and fl & PSH == 0 and rng.random() < 0.3:
                script.append((fl, srv))  # a duplicate
            script.append((fl, srv))
            k += 1
        out.append(script[:n])
    return out


def interleaved(scripts, seed, noise=0.0, first_conn=0):
    """The scripts' packets merged in a random order that keeps each script's own, with UDP and
    cut packets of the same endpoints mixed in; returns Packets."""
    rng = np.random.default_rng(seed)
    left = [len(s) for s in scripts]
    order = np.repeat(np.arange(len(scripts)), left)
    rng.shuffle(order)
    at = [0] * len(scripts)
    p = Packets()
    for j in order:
        j = int(j)
        fl, srv = scripts[j][at[j]]
        at[j] += 1
        c, s = endpoints(first_conn + j)
        a, b = (s, c) if srv else (c, s)
        if noise and rng.random() < noise:
            p.add(a[0], b[0], a[1], b[1], ACK, UDP if rng.random() < 0.5 else CUT)
        p.add(a[0], b[0], a[1], b[1], fl)
    return p


def size_case(n, nsmall=1 << 16, one=False):
    """n minimal frames: a quarter of them one connection (its packets at every fourth place),
    the rest spread over nsmall connections, each packet the next of its connection's LIFE; with
    `one` every packet belongs to the one connection.  Returns (batch, keys, flags)."""
    i = np.arange(n, dtype=np.int64)
    big = np.ones(n, bool) if one else i % 4 == 3
    rank = np.where(big, np.cumsum(big) - 1, 0)
    small_i = np.cumsum(~big) - 1
    conn = np.where(big, 0, 1 + small_i % nsmall)
    rank = np.where(big, rank, small_i // nsmall)
    life_fl = np.array([f for f, _ in LIFE], np.uint8)
    life_srv = np.array([s for _, s in LIFE], bool)
    fl, srv = life_fl[rank % len(LIFE)], life_srv[rank % len(LIFE)]
    caddr, cport = (0x0A000000 + conn).astype(np.uint32), (1024 + conn % 60000).astype(np.uint32)
    saddr, sport = (0xC0A80000 + conn % 251).astype(np.uint32), (80 + conn % 3).astype(np.uint32)
    src, dst = np.where(srv, saddr, caddr), np.where(srv, caddr, saddr)
    sp, dp = np.where(srv, sport, cport), np.where(srv, cport, sport)
    batch = frames(src, dst, sp, dp, fl)
    keys = list(zip(src.tolist(), dst.tolist(), sp.tolist(), dp.tolist()))
    return batch, keys, fl


def sparse_case(n, tcp, nconn=37):
    """n minimal frames, TCP where the mask `tcp` says (the k-th such packet is the next of
    connection k % nconn's LIFE) and UDP between the same endpoints elsewhere.  Returns (batch,
    keys with None for the UDP packets, flags)."""
    tcp = np.asarray(tcp, bool)
    k = np.where(tcp, np.cumsum(tcp) - 1, np.arange(n))
    conn, rank = k % nconn, k // nconn
    life_fl = np.array([f for f, _ in LIFE], np.uint8)
    life_srv = np.array([s for _, s in LIFE], bool)
    fl, srv = life_fl[rank % len(LIFE)], life_srv[rank % len(LIFE)] & tcp
    caddr, cport = (0x0A000000 + conn).astype(np.uint32), (1024 + conn).astype(np.uint32)
    saddr, sport = (0xC0A80000 + conn % 251).astype(np.uint32), (80 + conn % 3).astype(np.uint32)
    src, dst = np.where(srv, saddr, caddr), np.where(srv, caddr, saddr)
    sp, dp = np.where(srv, sport, cport), np.where(srv, cport, sport)
    batch = frames(src, dst, sp, dp, fl, np.where(tcp, TCP, UDP))
    keys = [None] * n
    for i in np.nonzero(tcp)[0]:
        keys[i] = (int(src[i]), int(dst[i]), int(sp[i]), int(dp[i]))
    return batch, keys, fl
