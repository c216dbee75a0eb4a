"""TEST INFRASTRUCTURE ONLY: the oracle of the stateful TCP assembler (gpd_tcp_assembler_run,
include/gpd_tcpasm.h).  tests/tcpassembly_ref.py restates tcpassembly's Assembler (pinned by
assembly_test.go's vectors), tests/tcpstream_ref.py adds skipFlush and FlushAll.  This file
subclasses the latter and adds

  FlushWithOptions   tcpassembly/assembly.go:235-266, line by line
  FlushOlderThan     :269-271

and keeps one assembler per key alive across runs, so that the page list (with every page's
Seen), nextSeq and lastSeen outlive a batch exactly as they do in the reference.  The reference
has no flush tests: the flush is pinned by hand-checked literals in tests/test_tcpasm.py.

`Model.run` takes one grouped hand-off (SEG_DTYPE / GROUP_DTYPE records and the packets' bytes)
plus the flush options and returns the arrays the device must give byte for byte.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import tcpassembly_ref as TA
import tcpstream_ref as SR

REASM_DTYPE, STREAM_DTYPE = SR.REASM_DTYPE, SR.STREAM_DTYPE
CONN_INFO_DTYPE = np.dtype([("next_seq", "<u4"), ("flags", "<u4"), ("pages", "<u4"), ("page_bytes", "<u4"),
                            ("last_seen_ns", "<u8")])
R_START, R_END, R_FLUSHED, R_CARRIED = 1, 2, 4, 8
CONN_OPEN, CONN_NOSEQ = 1, 2
NO_PACKET = 0xFFFFFFFF
UNGROUPED = 0xFFFFFFFF


class StatefulAssembler(SR.FlushingAssembler):
    """One reference Assembler.  cur_pkt / run_no say where the segment under assembly comes
    from, so that a delivered page knows its packet and whether it was carried."""
    cur_pkt = 0
    run_no = 0

    def pagesFromTCP(self, seq, end, payload, ts):
        first, last, num = super().pagesFromTCP(seq, end, payload, ts)
        p = first
        while p is not None:
            p.r.pkt, p.r.run = self.cur_pkt, self.run_no
            p = p.next
        return first, last, num

    def FlushWithOptions(self, T, CloseAll):
        """:235-266.  Seen.Before(T) and lastSeen.Before(T) are strict."""
        flushes = closes = 0
        self.flushing = True
        for conn in list(self.connPool.conns.values()):                   # :236, 239
            flushed = False                                               # :240
            if conn.closed:                                               # :242-246
                continue
            while conn.first is not None and conn.first.r.Seen < T:       # :247
                self.skipFlush(conn)                                      # :248
                flushed = True                                            # :249
                if conn.closed:                                           # :250-253
                    closes += 1
                    break
            if CloseAll and not conn.closed and conn.first is None and conn.lastSeen < T:  # :255
                flushed = True                                            # :256
                self.closeConnection(conn)                                # :257
                closes += 1                                               # :258
            if flushed:                                                   # :260-262
                flushes += 1
        self.flushing = False
        return flushes, closes                                            # :265

    def FlushOlderThan(self, t):
        """:269-271."""
        return self.FlushWithOptions(t, True)

    def FlushAll(self):
        self.flushing = True
        n = super().FlushAll()
        self.flushing = False
        return n


class Events:
    """The StreamFactory and Stream of one key: what was called, in order, over all runs."""

    def __init__(self):
        self.asm = None
        self.order = []   # "new" | ("call", [(Bytes, Skip, Start, End, Seen)]) | "complete", over all runs
        self.run_calls = []  # this run: (flushed, [(packet, src_off, len, skip, start, end, carried, seen, data)])
        self.run_completed = 0

    def New(self, key):
        self.order.append("new")
        return self

    def Reassembled(self, rs):
        call, plain = [], []
        for r in rs:
            data = bytes(r.Bytes)
            run = getattr(r, "run", None)
            carried = run is not None and run != self.asm.run_no
            pkt = NO_PACKET if carried else (self.asm.cur_pkt if run is None else r.pkt)
            b = r.Bytes
            off = b.off if isinstance(b, SR.Span) and len(data) and not carried else 0
            skip = min(int(r.Skip), 0x7FFFFFFF)
            call.append((pkt, off, len(data), skip, bool(r.Start), bool(r.End), carried, int(r.Seen), data))
            plain.append((data, skip, bool(r.Start), bool(r.End), int(r.Seen)))
        self.run_calls.append((self.asm.flushing, call))
        self.order.append(("call", plain))

    def ReassemblyComplete(self):
        self.run_completed += 1
        self.order.append("complete")


Expected = namedtuple("Expected", "recs seen_ns streams bytes conns stats out")


class Model:
    """The reference's Assembler + StreamPool for flow ids below id_bound, one assembler per key
    (connections do not depend on each other without MaxBufferedPagesTotal)."""

    def __init__(self, id_bound, max_pages=0):
        self.id_bound, self.max_pages = id_bound, max_pages
        self.keys = {}  # key -> Events
        self.run_no = 0

    def _asm(self, key):
        ev = self.keys.get(key)
        if ev is None:
            ev = self.keys[key] = Events()
            ev.asm = StatefulAssembler(TA.StreamPool(ev), MaxBufferedPagesPerConnection=self.max_pages)
        return ev

    def conn(self, key):
        ev = self.keys.get(key)
        return None if ev is None else ev.asm.connPool.conns.get(key)

    def open_keys(self):
        return sorted(k for k in self.keys if self.conn(k) is not None)

    def info(self, key):
        """The key's (next_seq, flags, pages, page_bytes, last_seen_ns); all zero when it is closed."""
        c = self.conn(key)
        if c is None:
            return (0, 0, 0, 0, 0)
        noseq = c.nextSeq == TA.INVALID_SEQUENCE
        nbytes, p = 0, c.first
        while p is not None:
            nbytes += len(p.r.Bytes)
            p = p.next
        return (0 if noseq else c.nextSeq, CONN_OPEN | (CONN_NOSEQ if noseq else 0), c.pages, nbytes,
                int(max(c.lastSeen, 0)))

    def conns(self):
        out = np.zeros(self.id_bound, CONN_INFO_DTYPE)
        for k in self.keys:
            if self.conn(k) is not None:
                out[k] = self.info(k)
        return out

    def stats(self, conns=None):
        c = self.conns() if conns is None else conns
        return {"connections": int((c["flags"] & CONN_OPEN != 0).sum()),
                "connections_with_pages": int((c["pages"] > 0).sum()), "pages": int(c["pages"].sum()),
                "page_bytes": int(c["page_bytes"].sum())}

    def drive(self, work, packet=None, ts=None, now=0, T=0, close_all=False, flush_all=False):
        """One run over `work`, a list of (key, the key's segment records in order): the keys
        need only be hashable and sortable.  Returns (record rows, their Seen, stream rows with
        the key first, byte chunks, bytes, calls)."""
        self.run_no += 1
        grouped = [k for k, _ in work]
        for k in grouped:
            self._asm(k)
        todo = grouped + [k for k in sorted(self.keys) if k not in set(grouped) and self.conn(k) is not None]
        for k in todo:
            ev = self.keys[k]
            ev.run_calls, ev.run_completed = [], 0
            ev.asm.run_no = self.run_no
        for key, rs in work:
            a = self.keys[key].asm
            for r in rs:
                a.cur_pkt = int(r["packet"])
                t = now if ts is None else int(ts[int(r["packet"])])
                a.AssembleSegment(key, r, packet(int(r["packet"])), ts=t)
        recs, seens, streams, chunks = [], [], [], []
        nbytes = ncalls = 0
        for k in todo:
            ev = self.keys[k]
            ev.asm.FlushWithOptions(T, close_all)
            if flush_all:
                ev.asm.FlushAll()
            if k not in grouped and not ev.run_calls and not ev.run_completed:
                continue
            first_rec, byte_off = len(recs), nbytes
            for ci, (flushed, call) in enumerate(ev.run_calls):
                for (pkt, off, ln, skip, start, end, carried, seen, data) in call:
                    fl = (R_START if start else 0) | (R_END if end else 0) | (R_FLUSHED if flushed else 0) | \
                        (R_CARRIED if carried else 0)
                    recs.append((pkt, off, ln, skip, nbytes, ci, fl, 0))
                    seens.append(seen)
                    chunks.append(data)
                    nbytes += ln
            ncalls += len(ev.run_calls)
            c = self.conn(k)
            if c is None:
                op, nseq, pages = 0, 0, 0
            else:
                noseq = c.nextSeq == TA.INVALID_SEQUENCE
                op, nseq, pages = CONN_OPEN | (CONN_NOSEQ if noseq else 0), 0 if noseq else int(c.nextSeq), c.pages
            streams.append((k, first_rec, len(recs) - first_rec, len(ev.run_calls), byte_off, nbytes - byte_off,
                            ev.run_completed, op, nseq, pages))
        return recs, seens, streams, chunks, nbytes, ncalls

    def run(self, segs=None, groups=None, packet=None, ts=None, now=0, T=0, close_all=False, flush_all=False):
        """One gpd_tcp_assembler_run.  ts: None or a sequence of per-packet timestamps (ns)."""
        work = []
        if groups is not None:
            for g in groups:
                key = int(g["flow_id"])
                if key == UNGROUPED:
                    continue
                assert key < self.id_bound
                work.append((key, segs[int(g["start"]):int(g["start"]) + int(g["count"])]))
        recs, seens, streams, chunks, nbytes, ncalls = self.drive(work, packet, ts, now, T, close_all, flush_all)
        conns = self.conns()
        st = self.stats(conns)
        out = (len(recs), len(streams), nbytes, ncalls, st["connections"], st["pages"], st["page_bytes"], 0)
        return Expected(np.array(recs, REASM_DTYPE), np.array(seens, np.uint64), np.array(streams, STREAM_DTYPE),
                        np.frombuffer(b"".join(chunks), np.uint8), conns, st, out)


def call_lists(ev: Events):
    """The key's Reassembled calls over all runs: [[(Bytes, Skip, Start, End, Seen), ...], ...]."""
    return [o[1] for o in ev.order if isinstance(o, tuple)]


def order_of(ev: Events):
    """"new" / "call" / "complete" in order, over all runs."""
    return [o if isinstance(o, str) else "call" for o in ev.order]
