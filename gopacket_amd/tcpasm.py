"""The stateful TCP assembler: tcpassembly's Assembler + StreamPool as a device object.

`tcpstream.TCPStreams` treats a batch as the reordering horizon and drains at its end.  An
`Assembler` keeps, per flow record, what the reference's `connection` keeps
(tcpassembly/assembly.go:374-383): nextSeq, lastSeen and the out-of-order page list with the
pages' bytes, on the device, from batch to batch.  `AssembleBatch` runs AssembleWithTimestamp
(:533-607) for a grouped hand-off's segments on top of that state, then FlushWithOptions
(:235-266) and, if asked, FlushAll (:276-287) over every connection held;
`FlushOlderThan` / `FlushWithOptions` / `FlushAll` are runs with no segments
(gpd_tcp_assembler_run, include/gpd_tcpasm.h).  Results come in tcpstream's layouts plus
`seen_ns` (Reassembly.Seen as a timestamp); `deliver` replays them into a StreamFactory.

The entry points are bound onto the loaded library here, on first use, from TCPASM_EXPORTS.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np

from . import _lib
from ._lib import GpdBatch, check
from .tcpassembly import GROUP_DTYPE, SEG_DTYPE
from .tcpstream import REASM_DTYPE, STREAM_DTYPE, GpdTcpAsmOpts, Reassembly, R_END, R_START

CONN_INFO_DTYPE = np.dtype([("next_seq", "<u4"), ("flags", "<u4"), ("pages", "<u4"), ("page_bytes", "<u4"),
                            ("last_seen_ns", "<u8")])
assert CONN_INFO_DTYPE.itemsize == 24

CONN_OPEN, CONN_NOSEQ = 1, 2
R_FLUSHED, R_CARRIED = 4, 8
NO_PACKET = 0xFFFFFFFF


class GpdTcpFlush(C.Structure):
    _fields_ = [("before_ns", C.c_uint64), ("close_all", C.c_uint32), ("flush_all", C.c_uint32)]


TCPASM_EXPORTS = {
    # include/gpd_tcpasm.h — name: (restype, argtypes)
    "gpd_tcp_assembler_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(GpdTcpAsmOpts), C.POINTER(C.c_void_p)]),
    "gpd_tcp_assembler_destroy": (None, [C.c_void_p]),
    "gpd_tcp_assembler_run": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.c_uint64, C.POINTER(GpdTcpFlush), C.c_void_p, C.c_uint64,
                                        C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.c_void_p]),
    "gpd_tcp_assembler_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gpd_tcp_assembler_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "gpd_tcp_assembler_conns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}

_bound = False


def tcpasm_lib():
    """The loaded library with the assembler's signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in TCPASM_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


# recs / seen_ns / streams / bytes: uint8 device tensors (seen_ns: int64, the u64 bit patterns);
# open_before: the flow ids open in the object before the run (a host uint32 array), which
# `deliver` needs to know when StreamFactory.New is due.
AsmResult = namedtuple("AsmResult", "recs seen_ns streams bytes nrecs nstreams nbytes ncalls connections pages "
                                    "page_bytes open_before")
HostAsm = namedtuple("HostAsm", "recs seen_ns streams bytes open_before")


class Assembler:
    """tcpassembly.Assembler with its StreamPool, on the device of `parser`, for flow records
    below `id_bound`."""

    def __init__(self, parser, id_bound: int, max_pages_per_connection: int = 0):
        self._parser = parser
        self.device = parser.device
        self.id_bound = int(id_bound)
        h = C.c_void_p()
        opts = GpdTcpAsmOpts(int(max_pages_per_connection), 0)
        check(tcpasm_lib().gpd_tcp_assembler_create(parser.ctx().h, self.id_bound, C.byref(opts), C.byref(h)),
              "gpd_tcp_assembler_create")
        self._h = h

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None and h.value:
            tcpasm_lib().gpd_tcp_assembler_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise ValueError("Assembler is closed")
        return self._h

    def _stream(self, stream):
        from .parser import _torch
        return stream if stream is not None else _torch().cuda.current_stream(self.device)

    def run_raw(self, dbatch, segs, count, groups, ngroups, ts, now, flush, recs, max_recs, seen, streams,
                max_streams, byts, max_bytes, stream=None):
        """gpd_tcp_assembler_run as it is: (rc, out[8]).  flush: (before_ns, close_all, flush_all)."""
        out = (C.c_uint64 * 8)()
        b = dbatch.c_batch() if dbatch is not None else None
        fl = GpdTcpFlush(int(flush[0]), 1 if flush[1] else 0, 1 if flush[2] else 0)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = tcpasm_lib().gpd_tcp_assembler_run(
            self._handle(), C.byref(b) if b is not None else None, p(segs), int(count), p(groups), int(ngroups),
            p(ts), int(now), C.byref(fl), p(recs), int(max_recs), p(seen), p(streams), int(max_streams), p(byts),
            int(max_bytes), out, C.c_void_p(self._stream(stream).cuda_stream))
        return rc, tuple(int(v) for v in out)

    def AssembleBatch(self, dbatch, segs, groups, count: int, ngroups: int, ts=None, now: int = 0,
                      flush_older_than: int = 0, close_all: bool = False, flush_all: bool = False,
                      stream=None) -> AsmResult:
        """One run: the hand-off `segs`, `groups`, `count`, `ngroups` of `dbatch` as TCPSegments
        returned them (flow ids given), `ts` None or an int64 / uint64 device tensor of the
        packets' timestamps in ns (None: every timestamp is `now`), then
        FlushWithOptions{T: flush_older_than, CloseAll: close_all} and, with flush_all, FlushAll.
        A sizing call, the allocation, then the run.  Synchronises `stream`."""
        from .parser import _torch
        torch = _torch()
        dev = torch.device("cuda", self.device)
        count, ngroups = int(count), int(ngroups)
        if count and (segs.numel() < count * SEG_DTYPE.itemsize or groups.numel() < ngroups * GROUP_DTYPE.itemsize):
            raise ValueError("AssembleBatch: segs / groups hold fewer records than count / ngroups")
        if ts is not None and count and ts.numel() * ts.element_size() < 8 * dbatch.n:
            raise ValueError("AssembleBatch: ts holds fewer timestamps than the batch has packets")
        flush = (flush_older_than, close_all, flush_all)
        open_before = self.open_ids()
        head = (dbatch, segs, count, groups, ngroups, ts, now, flush)
        rc, out = self.run_raw(*head, None, 0, None, None, 0, None, 0, stream)
        check(rc, "gpd_tcp_assembler_run")
        nrecs, nstreams, nbytes = out[0], out[1], out[2]
        recs = torch.empty(max(nrecs, 1) * REASM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        seen = torch.empty(max(nrecs, 1), dtype=torch.int64, device=dev)
        streams = torch.empty(max(nstreams, 1) * STREAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        byts = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        rc, out = self.run_raw(*head, recs, nrecs, seen, streams, nstreams, byts, nbytes, stream)
        check(rc, "gpd_tcp_assembler_run")
        return AsmResult(recs[:out[0] * REASM_DTYPE.itemsize], seen[:out[0]], streams[:out[1] * STREAM_DTYPE.itemsize],
                         byts[:out[2]], out[0], out[1], out[2], out[3], out[4], out[5], out[6], open_before)

    def FlushWithOptions(self, T: int, CloseAll: bool, stream=None) -> AsmResult:
        """Assembler.FlushWithOptions (:235-266) over every connection held."""
        return self.AssembleBatch(None, None, None, 0, 0, flush_older_than=T, close_all=CloseAll, stream=stream)

    def FlushOlderThan(self, t: int, stream=None) -> AsmResult:
        """Assembler.FlushOlderThan (:269-271): FlushWithOptions with CloseAll."""
        return self.FlushWithOptions(t, True, stream=stream)

    def FlushAll(self, stream=None) -> AsmResult:
        """Assembler.FlushAll (:276-287)."""
        return self.AssembleBatch(None, None, None, 0, 0, flush_all=True, stream=stream)

    def conns(self, stream=None) -> np.ndarray:
        """CONN_INFO_DTYPE[id_bound]: the connections held, by flow id (all zero: none)."""
        from .parser import _torch
        torch = _torch()
        t = torch.empty(max(self.id_bound, 1) * CONN_INFO_DTYPE.itemsize, dtype=torch.uint8,
                        device=torch.device("cuda", self.device))
        check(tcpasm_lib().gpd_tcp_assembler_conns(self._handle(), C.c_void_p(t.data_ptr()),
                                                   C.c_void_p(self._stream(stream).cuda_stream)),
              "gpd_tcp_assembler_conns")
        return t.cpu().numpy().view(CONN_INFO_DTYPE)[:self.id_bound].copy()

    def open_ids(self) -> np.ndarray:
        """The flow ids of the connections held, ascending."""
        if self.stats()["connections"] == 0:
            return np.zeros(0, np.uint32)
        return np.nonzero(self.conns()["flags"] & CONN_OPEN)[0].astype(np.uint32)

    def stats(self) -> dict:
        out = (C.c_uint64 * 4)()
        check(tcpasm_lib().gpd_tcp_assembler_stats(self._handle(), out), "gpd_tcp_assembler_stats")
        return {"connections": int(out[0]), "connections_with_pages": int(out[1]), "pages": int(out[2]),
                "page_bytes": int(out[3])}

    def reset(self, stream=None) -> None:
        """Drops every connection; call it when the flow table is reset."""
        check(tcpasm_lib().gpd_tcp_assembler_reset(self._handle(), C.c_void_p(self._stream(stream).cuda_stream)),
              "gpd_tcp_assembler_reset")


def NewAssembler(parser, table_or_id_bound, max_pages_per_connection: int = 0) -> Assembler:
    """tcpassembly.NewAssembler(NewStreamPool(...)) for a flow table (or its capacity)."""
    bound = table_or_id_bound if isinstance(table_or_id_bound, int) else table_or_id_bound.Stats()["capacity"]
    return Assembler(parser, int(bound), max_pages_per_connection)


def to_host(result: AsmResult) -> HostAsm:
    """Host copies of an AsmResult: REASM_DTYPE[nrecs], uint64[nrecs], STREAM_DTYPE[nstreams],
    uint8[nbytes] and the open set before the run."""
    recs = result.recs.cpu().numpy().view(REASM_DTYPE).copy()
    seen = result.seen_ns.cpu().numpy().view(np.uint64).copy()
    streams = result.streams.cpu().numpy().view(STREAM_DTYPE).copy()
    if len(recs) != result.nrecs or len(streams) != result.nstreams or len(seen) != result.nrecs:
        raise ValueError("to_host: the tensors hold fewer records than the counts say")
    return HostAsm(recs, seen, streams, result.bytes.cpu().numpy().copy(), np.asarray(result.open_before, np.uint32))


def deliver(result, factory, streams: Optional[dict] = None) -> None:
    """Makes the calls the reference's assembler makes for one run, stream by stream:
    factory.New(flow_id) for a key that was not open in the object before the run (or that
    closed earlier in this run), stream.Reassembled([Reassembly, ...]) per call with
    Reassembly.Seen the timestamp from seen_ns, stream.ReassemblyComplete() after a call whose
    last record has End and for a close made by a flush.  `streams` (flow_id -> stream) is the
    caller's pool across runs: New's results are kept there while the connection is open (None:
    a pool for this call alone, so a connection opened by an earlier run gets a new stream)."""
    h = result if isinstance(result, HostAsm) else to_host(result)
    streams = {} if streams is None else streams
    was_open = set(int(k) for k in h.open_before)
    for s in h.streams:
        key, ended = int(s["flow_id"]), 0
        if key not in was_open:
            streams.pop(key, None)  # (a stale entry of the caller's)
        st = streams.get(key)
        a, b = int(s["first_rec"]), int(s["first_rec"]) + int(s["nrec"])
        recs, seen = h.recs[a:b], h.seen_ns[a:b]
        k = 0
        while k < len(recs):
            e = k
            while e < len(recs) and recs["call"][e] == recs["call"][k]:
                e += 1
            call = []
            for r, t in zip(recs[k:e], seen[k:e]):
                data = h.bytes[int(r["stream_off"]):int(r["stream_off"]) + int(r["len"])].tobytes()
                f = int(r["flags"])
                call.append(Reassembly(data, int(r["skip"]), bool(f & R_START), bool(f & R_END), int(t)))
            if st is None:
                st = streams[key] = factory.New(key)
            st.Reassembled(call)
            if call[-1].End:
                st.ReassemblyComplete()
                streams.pop(key, None)
                st = None
                ended += 1
            k = e
        if int(s["completed"]) > ended:  # closed by a flush with no data left (:255-259, :649-651)
            if st is None:
                st = factory.New(key)  # (opened earlier without the caller's pool seeing it)
            st.ReassemblyComplete()
            streams.pop(key, None)
            st = None
        if st is None and int(s["open"]) & CONN_OPEN and (key not in was_open or int(s["completed"])):
            streams[key] = factory.New(key)  # (created by segments that made no call yet)
