"""TEST INFRASTRUCTURE ONLY: the oracle of the TCP stream assembly (gpd_tcp_assemble,
include/gpd_tcpstream.h).  tests/tcpassembly_ref.py restates tcpassembly's Assembler and is pinned
by assembly_test.go's vectors (tests/golden/tcpassembly_vectors.json).  This file subclasses it
and adds what the end of a batch needs:

  skipFlush        tcpassembly/assembly.go:645-657
  the drain        `for conn.first != nil && !conn.closed { skipFlush(conn) }`: FlushWithOptions
                   (:235-266) with T later than every packet and CloseAll false, :247-254
  FlushAll's close `for !conn.closed { skipFlush(conn) }` (:276-287)

The reference has no flush tests, so this part is a cited restatement, not a pinned one (two
hand-checked cases are literals in tests/test_tcpstream.py).

From hand-off records (SEG_DTYPE, GROUP_DTYPE of tests/tcpseg_ref.py) and the packets' bytes it
builds the arrays the device must give byte for byte: records, streams, bytes, state.  Every key
gets an assembler of its own, as connections do not depend on each other without
MaxBufferedPagesTotal.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import tcpassembly_ref as TA

REASM_DTYPE = np.dtype([("packet", "<u4"), ("src_off", "<u4"), ("len", "<u4"), ("skip", "<i4"),
                        ("stream_off", "<u8"), ("call", "<u4"), ("flags", "<u2"), ("reserved", "<u2")])
STREAM_DTYPE = np.dtype([("flow_id", "<u4"), ("first_rec", "<u4"), ("nrec", "<u4"), ("ncalls", "<u4"),
                         ("byte_off", "<u8"), ("nbytes", "<u8"), ("completed", "<u4"), ("open", "<u4"),
                         ("next_seq", "<u4"), ("reserved", "<u4")])
CONN_DTYPE = np.dtype([("next_seq", "<u4"), ("flags", "<u4")])
R_START, R_END, R_FLUSHED = 1, 2, 4
UNGROUPED = 0xFFFFFFFF


class Span:
    """Payload bytes that remember where they lie: packet index and offset in the packet.  Has
    what the restated assembler asks of a payload: len, truth, slicing, bytes()."""
    __slots__ = ("pkt", "off", "data")

    def __init__(self, pkt, off, data):
        self.pkt, self.off, self.data = pkt, off, data

    def __len__(self):
        return len(self.data)

    def __getitem__(self, s):
        start = s.indices(len(self.data))[0]
        return Span(self.pkt, self.off + start, self.data[s])

    def __bytes__(self):
        return bytes(self.data)


class FlushingAssembler(TA.Assembler):
    flushing = False

    def AssembleSegment(self, key, rec, pkt, ts=0.0):
        po, pl = int(rec["payload_off"]), int(rec["payload_len"])
        self.AssembleWithTimestamp(key, int(rec["seq"]), int(rec["flags"]),
                                   Span(int(rec["packet"]), po, bytes(pkt[po:po + pl])), ts)

    def skipFlush(self, conn):
        """:645-657."""
        if conn.first is None:
            self.closeConnection(conn)
            return
        self.ret = []
        self.addNextFromConn(conn)
        self.addContiguous(conn)
        self.sendToConnection(conn)

    def Drain(self):
        """FlushWithOptions{T: later than every packet, CloseAll: false} (:235-266): for every
        connection, `for conn.first != nil { skipFlush; if conn.closed break }` (:247-254)."""
        self.flushing = True
        for conn in list(self.connPool.conns.values()):
            while conn.first is not None and not conn.closed:
                self.skipFlush(conn)
        self.flushing = False

    def FlushAll(self):
        """:276-287."""
        conns = list(self.connPool.conns.values())
        for conn in conns:
            while not conn.closed:
                self.skipFlush(conn)
        return len(conns)


class _Events:
    """The StreamFactory and Stream of one key: what was called, in order."""

    def __init__(self):
        self.asm = None
        self.news = 0
        self.calls = []      # (flushed, [(packet, src_off, len, skip, start, end, bytes)])
        self.completed = 0
        self.order = []      # "new" | ("call", index) | "complete"

    def New(self, key):
        self.news += 1
        self.order.append("new")
        return self

    def Reassembled(self, rs):
        call = []
        for r in rs:
            b = r.Bytes
            data = bytes(b)
            off = b.off if isinstance(b, Span) and len(data) else 0  # (no Bytes[0]: zero)
            skip = min(int(r.Skip), 0x7FFFFFFF)  # (the record's skip is 32 bits wide, saturated)
            call.append((int(r.Seen), off, len(data), skip, bool(r.Start), bool(r.End), data))
        self.order.append(("call", len(self.calls)))
        self.calls.append((self.asm.flushing, call))

    def ReassemblyComplete(self):
        self.completed += 1
        self.order.append("complete")


Expected = namedtuple("Expected", "recs streams bytes state nrecs nstreams nbytes ncalls events")


def assemble(segs, groups, packet, max_pages=0, close_all=False, state=None) -> Expected:
    """The expected output of gpd_tcp_assemble.  segs, groups: the grouped hand-off; packet(i):
    packet i's bytes; state: CONN_DTYPE array indexed by flow id, or None.  Returns the arrays,
    the new state (a copy; None without state), the four counts and the per-key events
    {flow_id: _Events}."""
    new_state = None if state is None else state.copy()
    recs, streams, chunks, events = [], [], [], {}
    nbytes = ncalls = 0
    for g in groups:
        key = int(g["flow_id"])
        if key == UNGROUPED:
            continue
        ev = _Events()
        a = FlushingAssembler(TA.StreamPool(ev), MaxBufferedPagesPerConnection=max_pages)
        ev.asm = a
        if state is not None and key < len(state) and int(state[key]["flags"]) & 1:
            conn = a.connPool.getConnection(key, False, -1.0)  # carried over: open, nextSeq known
            conn.nextSeq = int(state[key]["next_seq"])
            ev.news, ev.order = 0, []
        for r in segs[int(g["start"]):int(g["start"]) + int(g["count"])]:
            a.AssembleSegment(key, r, packet(int(r["packet"])), ts=float(r["packet"]))
        a.Drain()
        if close_all:
            a.FlushAll()
        first_rec, byte_off = len(recs), nbytes
        for ci, (flushed, call) in enumerate(ev.calls):
            for (pkt, off, ln, skip, start, end, data) in call:
                fl = (R_START if start else 0) | (R_END if end else 0) | (R_FLUSHED if flushed else 0)
                recs.append((pkt, off, ln, skip, nbytes, ci, fl, 0))
                chunks.append(data)
                nbytes += ln
        ncalls += len(ev.calls)
        conn = a.connPool.conns.get(key)
        is_open = conn is not None
        nseq = int(conn.nextSeq) if is_open else 0
        assert not is_open or (conn.first is None and conn.nextSeq != TA.INVALID_SEQUENCE)
        streams.append((key, first_rec, len(recs) - first_rec, len(ev.calls), byte_off, nbytes - byte_off,
                        ev.completed, int(is_open), nseq, 0))
        if new_state is not None and key < len(new_state):
            new_state[key] = (nseq, int(is_open))
        events[key] = ev
    return Expected(np.array(recs, REASM_DTYPE), np.array(streams, STREAM_DTYPE),
                    np.frombuffer(b"".join(chunks), np.uint8), new_state, len(recs), len(streams), nbytes, ncalls,
                    events)


def call_lists(ev: _Events):
    """The key's Reassembled calls as tests/tcpassembly_ref.RecordingFactory keeps them:
    [[(Bytes, Skip, Start, End), ...], ...]."""
    return [[(d, skip, start, end) for (_, _, _, skip, start, end, d) in call] for _, call in ev.calls]
