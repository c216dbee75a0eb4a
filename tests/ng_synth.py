"""Synthetic pcapng captures for the tests: raw block builders that can write what no writer
would (wrong lengths, short options, unknown types) and the seeded fuzz of tests/test_pcapng.py.
Test infrastructure; nothing under gopacket_amd/ imports it."""
import random
import struct

SHB, IDB, PB, SPB, ISB, EPB = 0x0A0D0D0A, 1, 2, 3, 5, 6


def opt(code, val, e, length=None, pad=True):
    """One option; `length` overrides the length field (the value bytes stay as given)."""
    n = len(val) if length is None else length
    return struct.pack(e + "HH", code, n) + val + (bytes(-len(val) % 4) if pad else b"")


def block(typ, body, e, total=None, trailer=None):
    """A block with `total` / `trailer` overriding the two length fields."""
    t = 12 + len(body) if total is None else total
    return struct.pack(e + "II", typ, t & 0xFFFFFFFF) + body + struct.pack(e + "I", (t if trailer is None else trailer)
                                                                          & 0xFFFFFFFF)


def shb(e="<", opts=b"", version=(1, 0), bom=0x1A2B3C4D, **kw):
    body = struct.pack(e + "IHHq", bom, version[0], version[1], -1) + opts
    return block(SHB, body, e, **kw)


def idb(e="<", linktype=1, snaplen=0, opts=b"", **kw):
    return block(IDB, struct.pack(e + "HHI", linktype, 0, snaplen) + opts, e, **kw)


def epb(data, e="<", ifindex=0, ts=0, caplen=None, wirelen=None, opts=b"", **kw):
    cl = len(data) if caplen is None else caplen
    wl = len(data) if wirelen is None else wirelen
    body = struct.pack(e + "IIIII", ifindex, ts >> 32, ts & 0xFFFFFFFF, cl & 0xFFFFFFFF, wl) + data + bytes(-len(data) % 4) + opts
    return block(EPB, body, e, **kw)


def pb(data, e="<", ifindex=0, drops=0, ts=0, caplen=None, wirelen=None, **kw):
    cl = len(data) if caplen is None else caplen
    wl = len(data) if wirelen is None else wirelen
    body = struct.pack(e + "HHIIII", ifindex, drops, ts >> 32, ts & 0xFFFFFFFF, cl & 0xFFFFFFFF, wl) + data + bytes(-len(data) % 4)
    return block(PB, body, e, **kw)


def spb(data, e="<", wirelen=None, **kw):
    wl = len(data) if wirelen is None else wirelen
    return block(SPB, struct.pack(e + "I", wl) + data + bytes(-len(data) % 4), e, **kw)


def isb(e="<", ifindex=0, ts=0, opts=b"", **kw):
    return block(ISB, struct.pack(e + "III", ifindex, ts >> 32, ts & 0xFFFFFFFF) + opts, e, **kw)


END = {"<": struct.pack("<HH", 0, 0), ">": struct.pack(">HH", 0, 0)}


def fuzz_capture(seed):
    """(bytes, (want_mixed, error_on_mismatch, skip_unknown)) — a capture of a few sections with
    every kind of block and, with some probability each, one of the reader's corner cases."""
    r = random.Random(seed)
    flags = (r.random() < 0.2, r.random() < 0.2, r.random() < 0.3)
    out = []
    p = lambda x: r.random() < x

    def payload():
        return bytes(r.getrandbits(8) for _ in range(r.choice((0, 1, 3, 4, 14, 60, 61, 97))))

    def str_opts(e, codes):
        o = b""
        for c in codes:
            if p(0.4):
                val = bytes(r.choice(b"abcdefgh") for _ in range(r.choice((1, 2, 3, 4, 5, 9))))
                o += opt(c, val, e, length=0 if p(0.05) else None) if not p(0.05) else opt(c, b"", e)
        return o

    for _ in range(r.choice((1, 1, 2, 3))):
        e = r.choice("<>")
        o = str_opts(e, (1, 2, 3, 4, 77))
        if o or p(0.3):
            o += END[e] if not p(0.04) else struct.pack(e + "HH", 0, r.choice((1, 4)))
        ver = (1, 0) if not p(0.1) else r.choice(((1, 1), (2, 0), (0, 0)))
        bom = 0x1A2B3C4D if not p(0.03) else 0x11223344
        out.append(shb(e, o, ver, bom))
        nif = 0
        if p(0.85):  # most sections start as a writer's do
            out.append(idb(e, r.choice((1, 1, 1, 1, 0)), r.choice((0, 0, 48, 65535))))
            nif = 1
        for _ in range(r.randrange(0, 16)):
            k = r.random()
            if k < 0.12:
                o = str_opts(e, (2, 1, 3, 12, 50))
                if p(0.3):
                    o += opt(9, bytes([r.choice((0, 3, 6, 9, 0x80 | 10, 0x80 | 63, 0x80 | 64, 0x80 | 100, 19, 20,
                                                 64, 127))]), e)
                if p(0.03):
                    o += opt(9, b"", e)
                if p(0.25):
                    o += opt(14, struct.pack(e + "Q", r.choice((0, 1, 1 << 40, (1 << 64) - 1))), e)
                if p(0.04):
                    o += opt(14, b"abcd", e)
                if p(0.2):
                    o += opt(11, b"\0tcp port 80", e)
                if p(0.04):
                    o += opt(11, b"", e)
                if o or p(0.3):
                    o += END[e]
                out.append(idb(e, r.choice((1, 1, 1, 0, 105)), r.choice((0, 0, 10, 64, 65535)), o))
                nif += 1
            elif k < 0.55:
                idx = r.randrange(0, nif) if nif and not p(0.02) else r.choice((nif, nif + 3, 0xFFFF, 0x10000))
                d = payload()
                cl = len(d) if not p(0.02) else len(d) + r.choice((1, 4, 5, 1000, 0xFFFFFFF0))
                ts = r.choice((0, 1, r.getrandbits(40), r.getrandbits(64), (1 << 64) - 1))
                mk = epb if p(0.7) else pb
                out.append(mk(d, e, ifindex=idx & (0xFFFFFFFF if mk is epb else 0xFFFF), ts=ts, caplen=cl,
                              wirelen=len(d) + r.choice((0, 0, 7))))
            elif k < 0.67:
                d = payload()
                out.append(spb(d, e, wirelen=len(d) + r.choice((0, 0, 0, 3, 100))))
            elif k < 0.77:
                o = b""
                if p(0.5):
                    o += opt(r.choice((2, 3, 4, 5)), struct.pack(e + "Q", r.getrandbits(64)), e)
                if p(0.08):
                    o += opt(r.choice((2, 3, 4, 5)), b"abc", e)
                if p(0.3):
                    o += opt(1, b"stats", e)
                if o or p(0.3):
                    o += END[e]
                idx = r.randrange(0, nif) if nif and not p(0.05) else nif + r.choice((0, 1))
                out.append(isb(e, idx, r.getrandbits(50), o))
            else:
                typ = r.choice((0, 4, 7, 10, 0xBAD, 0x80000001, 0xFFFFFFFF))
                out.append(block(typ, payload(), e))
            if p(0.02):  # a wrong total length on the block just written
                b = bytearray(out[-1])
                bad = r.choice((0, 4, 8, 9, 11, 13, len(b) - 1, len(b) + 1, len(b) + 4, 0x7FFFFFFF, 0xFFFFFFFF))
                b[4:8] = struct.pack(e + "I", bad)
                out[-1] = bytes(b)
    data = b"".join(out)
    if p(0.15) and data:
        data = data[:r.randrange(0, len(data))]
    if p(0.08) and data:
        b = bytearray(data)
        for _ in range(r.choice((1, 2, 5))):
            b[r.randrange(len(b))] = r.getrandbits(8)
        data = bytes(b)
    return data, flags
