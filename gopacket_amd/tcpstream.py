"""TCP stream assembly: tcpassembly's Reassembly lists for the connections of a batch, on the GPU.

`tcpassembly.TCPSegments` groups a decoded batch's TCP segments by connection key.  `TCPStreams`
takes those groups and runs, per key, what the reference's Assembler runs
(tcpassembly/assembly.go): AssembleWithTimestamp for each segment in order (:533-607), then the
end-of-batch drain `for conn.first != nil && !conn.closed { skipFlush(conn) }` (:645-657,
FlushWithOptions :235-266 with a time later than every packet) and, with close_all, FlushAll's
close (:276-287).  It returns one 32-byte record per Reassembly handed to Stream.Reassembled,
one 48-byte record per connection, and the records' bytes gathered into per-connection streams
(gpd_tcp_assemble, include/gpd_tcpstream.h).  `deliver` replays the host copies into a
StreamFactory (New / Reassembled / ReassemblyComplete), the surface a gopacket user expects.

A batch is the reordering horizon: out-of-order data still buffered at the end of the batch is
flushed with Skip set, it does not wait for the next batch.  An open connection is carried to
the next batch by an 8-byte state record per flow record (`NewConnState`).

The entry point is bound onto the loaded library here, on first use, from TCPSTREAM_EXPORTS: it
lives in its own header and is not part of _lib.EXPORTS.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np

from . import _lib
from ._lib import GpdBatch, check
from .tcpassembly import GROUP_DTYPE, SEG_DTYPE, TCP_UNGROUPED

REASM_DTYPE = np.dtype([("packet", "<u4"), ("src_off", "<u4"), ("len", "<u4"), ("skip", "<i4"),
                        ("stream_off", "<u8"), ("call", "<u4"), ("flags", "<u2"), ("reserved", "<u2")])
STREAM_DTYPE = np.dtype([("flow_id", "<u4"), ("first_rec", "<u4"), ("nrec", "<u4"), ("ncalls", "<u4"),
                         ("byte_off", "<u8"), ("nbytes", "<u8"), ("completed", "<u4"), ("open", "<u4"),
                         ("next_seq", "<u4"), ("reserved", "<u4")])
CONN_DTYPE = np.dtype([("next_seq", "<u4"), ("flags", "<u4")])
assert REASM_DTYPE.itemsize == 32 and STREAM_DTYPE.itemsize == 48 and CONN_DTYPE.itemsize == 8

R_START, R_END, R_FLUSHED = 1, 2, 4
CONN_OPEN = 1
PAGE_BYTES = 1900


class GpdTcpAsmOpts(C.Structure):
    _fields_ = [("max_pages_per_connection", C.c_uint32), ("close_all", C.c_uint32)]


TCPSTREAM_EXPORTS = {
    # include/gpd_tcpstream.h — name: (restype, argtypes)
    "gpd_tcp_assemble": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_uint32, C.POINTER(GpdTcpAsmOpts), C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
}

_bound = False


def tcpstream_lib():
    """The loaded library with the assembly's signature bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in TCPSTREAM_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


StreamResult = namedtuple("StreamResult", "recs streams bytes nrecs nstreams nbytes ncalls")


def _call(parser, dbatch, segs, count, groups, ngroups, state, id_bound, max_pages, close_all, recs, max_recs,
          streams, byts, max_bytes, stream):
    out = (C.c_uint64 * 4)()
    b = dbatch.c_batch()
    opts = GpdTcpAsmOpts(int(max_pages), 1 if close_all else 0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = tcpstream_lib().gpd_tcp_assemble(parser.ctx().h, C.byref(b), p(segs), count, p(groups), ngroups, p(state),
                                          id_bound, C.byref(opts), p(recs), max_recs, p(streams), p(byts),
                                          max_bytes, out, C.c_void_p(stream.cuda_stream))
    return rc, tuple(int(v) for v in out)


def NewConnState(table_or_id_bound, device=0):
    """The zeroed connection state for a flow table (or its capacity): one 8-byte record per flow
    record, as a uint8 device tensor.  Zero it again when the table is reset."""
    from .parser import _torch
    torch = _torch()
    bound = table_or_id_bound if isinstance(table_or_id_bound, int) else table_or_id_bound.Stats()["capacity"]
    return torch.zeros(max(int(bound), 1) * CONN_DTYPE.itemsize, dtype=torch.uint8,
                       device=torch.device("cuda", device))


def TCPStreams(parser, dbatch, segs, groups, count: int, ngroups: int, state=None, max_pages_per_connection: int = 0,
               close_all: bool = False, gather: bool = True, max_recs: Optional[int] = None,
               max_bytes: Optional[int] = None, stream=None) -> StreamResult:
    """The stream assembly of a grouped hand-off: `segs`, `groups`, `count`, `ngroups` as
    TCPSegments(parser, dbatch, dres, flow_id=...) returned them for `dbatch`.  Returns
    StreamResult(recs, streams, bytes, nrecs, nstreams, nbytes, ncalls): uint8 device tensors of
    nrecs x 32-byte records (REASM_DTYPE), nstreams x 48-byte records (STREAM_DTYPE) and the
    nbytes gathered stream bytes (None with gather=False: the payloads are then read in place
    through `packet` and `src_off`).  Synchronises `stream`.

    state (NewConnState) carries the open connections from batch to batch; None: every group
    starts with no connection.  max_recs / max_bytes None size the arrays with a first call;
    otherwise they are capacities, and the call raises (GPD_ERR_INVALID) when more is needed:
    nothing is written then, `state` included."""
    from .parser import _torch
    torch = _torch()
    dev = torch.device("cuda", parser.device)
    s = stream if stream is not None else torch.cuda.current_stream(parser.device)
    count, ngroups = int(count), int(ngroups)
    if segs.numel() < count * SEG_DTYPE.itemsize or groups.numel() < ngroups * GROUP_DTYPE.itemsize:
        raise ValueError("TCPStreams: segs / groups hold fewer records than count / ngroups")
    bound = 0
    if state is not None:
        bound = min(state.numel() * state.element_size() // CONN_DTYPE.itemsize, 0xFFFFFFFF)
    args = (parser, dbatch, segs, count, groups, ngroups, state, bound, max_pages_per_connection, close_all)
    if max_recs is None or (gather and max_bytes is None):
        rc, out = _call(*args, None, 0, None, None, 0, s)
        check(rc, "gpd_tcp_assemble")
        max_recs = out[0] if max_recs is None else int(max_recs)
        max_bytes = out[2] if max_bytes is None else int(max_bytes)
    max_recs = int(max_recs)
    max_bytes = int(max_bytes) if gather else 0
    recs = torch.empty(max(max_recs, 1) * REASM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    streams = torch.empty(max(ngroups, 1) * STREAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    byts = torch.empty(max(max_bytes, 16), dtype=torch.uint8, device=dev) if gather else None
    rc, out = _call(*args, recs, max_recs, streams, byts, max_bytes, s)
    check(rc, "gpd_tcp_assemble")
    nrecs, nstreams, nbytes, ncalls = out
    return StreamResult(recs[:nrecs * REASM_DTYPE.itemsize], streams[:nstreams * STREAM_DTYPE.itemsize],
                        byts[:nbytes] if gather else None, nrecs, nstreams, nbytes, ncalls)


HostStreams = namedtuple("HostStreams", "recs streams bytes")


def streams_to_host(result: StreamResult) -> HostStreams:
    """Host copies of a StreamResult: REASM_DTYPE[nrecs], STREAM_DTYPE[nstreams] and the bytes
    (uint8[nbytes], or None when nothing was gathered)."""
    recs = result.recs.cpu().numpy().view(REASM_DTYPE).copy()
    streams = result.streams.cpu().numpy().view(STREAM_DTYPE).copy()
    if len(recs) != result.nrecs or len(streams) != result.nstreams:
        raise ValueError("streams_to_host: the tensors hold fewer records than the counts say")
    byts = None if result.bytes is None else result.bytes.cpu().numpy().copy()
    return HostStreams(recs, streams, byts)


class Reassembly:
    """tcpassembly.Reassembly (:71-85).  Seen is the index of the packet the bytes come from (its
    timestamp is the caller's to look up)."""
    __slots__ = ("Bytes", "Skip", "Start", "End", "Seen")

    def __init__(self, Bytes, Skip, Start, End, Seen):
        self.Bytes, self.Skip, self.Start, self.End, self.Seen = Bytes, Skip, Start, End, Seen

    def as_tuple(self):
        return (bytes(self.Bytes), self.Skip, self.Start, self.End)


def deliver(result, factory, payload=None, streams=None) -> None:
    """Walks the host copies (a HostStreams, or a StreamResult, which is copied first) and makes
    the calls the reference's assembler makes, stream by stream: factory.New(flow_id) for a key
    whose stream has calls or completions, stream.Reassembled([Reassembly, ...]) per call and
    stream.ReassemblyComplete() after a call whose last record has End, plus the close_all one.

    `streams` (a dict flow_id -> stream) keeps the streams of connections that stay open from one
    batch to the next, as the reference's pool does: New is called only for keys not in it, and a
    completed key leaves it.  payload(rec) supplies the bytes when nothing was gathered."""
    h = result if isinstance(result, HostStreams) else streams_to_host(result)
    live = {} if streams is None else streams
    for s in h.streams:
        key, ended = int(s["flow_id"]), 0
        if int(s["ncalls"]) == 0 and int(s["completed"]) == 0:
            continue
        st = live.get(key)
        recs = h.recs[int(s["first_rec"]):int(s["first_rec"]) + int(s["nrec"])]
        k = 0
        while k < len(recs):
            e = k
            while e < len(recs) and recs["call"][e] == recs["call"][k]:
                e += 1
            call = []
            for r in recs[k:e]:
                if h.bytes is not None:
                    b = h.bytes[int(r["stream_off"]):int(r["stream_off"]) + int(r["len"])].tobytes()
                else:
                    b = payload(r)
                f = int(r["flags"])
                call.append(Reassembly(b, int(r["skip"]), bool(f & R_START), bool(f & R_END), int(r["packet"])))
            if st is None:
                st = live[key] = factory.New(key)
            st.Reassembled(call)
            if call[-1].End:
                st.ReassemblyComplete()
                live.pop(key, None)
                st = None
                ended += 1
            k = e
        if int(s["completed"]) > ended:  # the close of a connection that was still open (FlushAll)
            if st is None:
                st = factory.New(key)  # (carried from an earlier batch by `state` without its stream)
            st.ReassemblyComplete()
            live.pop(key, None)
