"""TEST INFRASTRUCTURE ONLY: a restatement of tcpassembly's Assembler (tcpassembly/assembly.go),
the stateful consumer of the TCP segment hand-off (gpd_tcp_segments, include/gpd_tcpassembly.h).
The product does not contain it: it exists so that tests can show that the
hand-off's records, in the hand-off's order, drive an assembler to the streams the reference
gives — as oracle/ip4defrag_ref.py does for the fragment hand-off.

Restated: Sequence.Difference / Add (:54-66), the page lists (traverseConn, pushBetween,
:683-710), AssembleWithTimestamp (:533-607), byteSpan (:609-620), sendToConnection (:624-633),
addContiguous (:636-640), closeConnection (:666-676), insertIntoConn (:712-727), pagesFromTCP
(:734-756), addNextFromConn (:760-780) and the MaxBufferedPagesPerConnection /
MaxBufferedPagesTotal limits.  Not restated: the page and connection caches' allocation, the
locks, FlushOlderThan / FlushAll.

The input is a hand-off record (SEG_DTYPE: seq, flags, payload_off, payload_len) and the
packet's bytes; the pool is keyed by whatever the caller supplies (the flow id of the record, or
a tuple of addresses and ports).
"""
from __future__ import annotations

from dataclasses import dataclass, field

INVALID_SEQUENCE = -1
UINT32_SIZE = 1 << 32
PAGE_BYTES = 1900
FIN, SYN, RST = 1, 2, 4


def difference(s: int, t: int) -> int:
    """Sequence.Difference (:54-61): t - s, safe for roll-over between the outer quarters."""
    if s > UINT32_SIZE - UINT32_SIZE // 4 and t < UINT32_SIZE // 4:
        t += UINT32_SIZE
    elif t > UINT32_SIZE - UINT32_SIZE // 4 and s < UINT32_SIZE // 4:
        s += UINT32_SIZE
    return t - s


def add(s: int, t: int) -> int:
    """Sequence.Add (:64-66)."""
    return (s + t) & (UINT32_SIZE - 1)


@dataclass
class Reassembly:
    """:71-85."""
    Bytes: bytes = b""
    Skip: int = 0
    Start: bool = False
    End: bool = False
    Seen: float = 0.0

    def as_tuple(self):
        return (bytes(self.Bytes), self.Skip, self.Start, self.End)


class _Page:
    def __init__(self, ts):
        self.r = Reassembly(Seen=ts)
        self.seq = 0
        self.prev = self.next = None


@dataclass
class _Connection:
    key: object
    stream: object
    created: float
    pages: int = 0
    first: object = None
    last: object = None
    nextSeq: int = INVALID_SEQUENCE
    lastSeen: float = float("-inf")
    closed: bool = False

    def traverse(self, seq):
        """traverseConn (:683-690): backwards from the highest sequence number."""
        prev, current = self.last, None
        while prev is not None and difference(prev.seq, seq) < 0:
            current = prev
            prev = current.prev
        return prev, current

    def push_between(self, prev, nxt, first, last):
        """pushBetween (:696-710)."""
        if nxt is None or self.last is None:
            self.last = last
        else:
            last.next = nxt
            nxt.prev = last
        if prev is None or self.first is None:
            self.first = first
        else:
            first.prev = prev
            prev.next = first


def byte_span(expected: int, received: int, data: bytes):
    """byteSpan (:609-620): the bytes at or past `expected`, and the sequence after them."""
    if expected == INVALID_SEQUENCE:
        return data, add(received, len(data))
    span = difference(received, expected)
    if span <= 0:
        return data, add(received, len(data))
    if len(data) < span:
        return b"", expected
    return data[span:], add(expected, len(data) - span)


class StreamPool:
    """:310-343, 495-512, 659-664 without the locks and the free list."""

    def __init__(self, factory):
        self.factory = factory
        self.conns = {}

    def getConnection(self, key, end: bool, ts):
        conn = self.conns.get(key)
        if end or conn is not None:
            return conn
        conn = _Connection(key, self.factory.New(key), ts)
        self.conns[key] = conn
        return conn

    def remove(self, conn):
        self.conns.pop(conn.key, None)


@dataclass
class Assembler:
    connPool: StreamPool
    MaxBufferedPagesTotal: int = 0
    MaxBufferedPagesPerConnection: int = 0
    used: int = 0  # pageCache.used
    ret: list = field(default_factory=list)

    # ---- the entry point, from a hand-off record
    def AssembleSegment(self, key, rec, pkt, ts=0.0):
        """AssembleWithTimestamp for one handed-over packet: `rec` a SEG_DTYPE record, `pkt` the
        packet's bytes."""
        po, pl = int(rec["payload_off"]), int(rec["payload_len"])
        self.AssembleWithTimestamp(key, int(rec["seq"]), int(rec["flags"]), bytes(pkt[po:po + pl]), ts)

    def AssembleWithTimestamp(self, key, seq: int, flags: int, payload: bytes, ts=0.0):
        """:533-607.  key stands for key{netFlow, t.TransportFlow()}."""
        syn, fin, rst = bool(flags & SYN), bool(flags & FIN), bool(flags & RST)
        if not syn and not fin and not rst and len(payload) == 0:  # :535
            return
        self.ret = []
        conn = self.connPool.getConnection(key, not syn and len(payload) == 0, ts)  # :550-551
        if conn is None:
            return
        if conn.lastSeen < ts:
            conn.lastSeen = ts
        if conn.nextSeq == INVALID_SEQUENCE:
            if syn:  # :569-579
                self.ret.append(Reassembly(Bytes=payload, Skip=0, Start=True, Seen=ts))
                conn.nextSeq = add(seq, len(payload) + 1)
            else:
                self.insertIntoConn(seq, fin or rst, payload, conn, ts)
        elif difference(conn.nextSeq, seq) > 0:  # :586-590
            self.insertIntoConn(seq, fin or rst, payload, conn, ts)
        else:  # :591-602
            data, conn.nextSeq = byte_span(conn.nextSeq, seq, payload)
            self.ret.append(Reassembly(Bytes=data, Skip=0, End=rst or fin, Seen=ts))
        if self.ret:
            self.sendToConnection(conn)

    def sendToConnection(self, conn):
        """:624-633."""
        self.addContiguous(conn)
        conn.stream.Reassembled(self.ret)
        if self.ret[-1].End:
            self.closeConnection(conn)

    def addContiguous(self, conn):
        """:636-640."""
        while conn.first is not None and difference(conn.nextSeq, conn.first.seq) <= 0:
            self.addNextFromConn(conn)

    def closeConnection(self, conn):
        """:666-676."""
        conn.stream.ReassemblyComplete()
        conn.closed = True
        self.connPool.remove(conn)
        p = conn.first
        while p is not None:
            self.used -= 1
            p = p.next

    def insertIntoConn(self, seq, end, payload, conn, ts):
        """:712-727."""
        assert not (conn.first is not None and conn.first.seq == conn.nextSeq), "wtf"
        p, p2, num = self.pagesFromTCP(seq, end, payload, ts)
        prev, current = conn.traverse(seq)
        conn.push_between(prev, current, p, p2)
        conn.pages += num
        if (0 < self.MaxBufferedPagesPerConnection <= conn.pages) or \
                (0 < self.MaxBufferedPagesTotal <= self.used):
            self.addNextFromConn(conn)

    def pagesFromTCP(self, seq, end, payload, ts):
        """:734-756: the payload cut into pages of 1900 bytes."""
        first = current = self._page(ts)
        num = 1
        while True:
            length = min(len(payload), PAGE_BYTES)
            current.r.Bytes = payload[:length]
            current.seq = seq
            payload = payload[length:]
            if not payload:
                break
            seq = add(seq, length)
            current.next = self._page(ts)
            current.next.prev = current
            current = current.next
            num += 1
        current.r.End = end
        return first, current, num

    def addNextFromConn(self, conn):
        """:760-780."""
        f = conn.first
        if conn.nextSeq == INVALID_SEQUENCE:
            f.r.Skip = -1
        else:
            diff = difference(conn.nextSeq, f.seq)
            if diff > 0:
                f.r.Skip = diff
        f.r.Bytes, conn.nextSeq = byte_span(conn.nextSeq, f.seq, f.r.Bytes)
        self.ret.append(f.r)
        self.used -= 1
        if conn.first is conn.last:
            conn.first = conn.last = None
        else:
            conn.first = f.next
            conn.first.prev = None
        conn.pages -= 1

    def _page(self, ts):
        self.used += 1
        return _Page(ts)


class RecordingFactory:
    """A StreamFactory whose streams keep every Reassembled call (as lists of
    (Bytes, Skip, Start, End)) under the connection's key; `completed` counts
    ReassemblyComplete per key."""

    def __init__(self):
        self.calls = {}
        self.completed = {}

    def New(self, key):
        fac = self

        class _Stream:
            def Reassembled(self, rs):
                fac.calls.setdefault(key, []).append([r.as_tuple() for r in rs])

            def ReassemblyComplete(self):
                fac.completed[key] = fac.completed.get(key, 0) + 1
        return _Stream()


def NewAssembler(factory, max_pages_per_connection: int = 0) -> Assembler:
    return Assembler(StreamPool(factory), MaxBufferedPagesPerConnection=max_pages_per_connection)
