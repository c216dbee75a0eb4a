"""tcpassembly hand-off: the TCP segments of a decoded batch, grouped by connection key, on the GPU.

The reference's application calls Assembler.AssembleWithTimestamp(netFlow, &tcp, ts) for every
packet (tcpassembly/assembly.go:533-607).  That call ignores a packet that carries neither
SYN/FIN/RST nor payload (:535), looks the connection up under key{netFlow, t.TransportFlow()}
(:543) and hands Seq, the flags and t.Payload to the connection's stateful insert.  `TCPSegments`
runs the ignore rule and reads those fields for every packet of an HBM-resident batch the parser
just decoded (gpd_tcp_segments, include/gpd_tcpassembly.h).  Given the flow ids of
`FlowTable.Insert` — the key's record index — it also groups the segments by key with a stable
device sort, so that several assemblers can each take whole connections and still see each
connection's packets in capture order.  The assembler's state stays with the caller.

The entry point is bound onto the loaded library here, on first use, from TCPSEG_EXPORTS: it
lives in its own header and is not part of _lib.EXPORTS.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import GpdBatch, GpdResult, check

SEG_DTYPE = np.dtype([("packet", "<u4"), ("flow_id", "<u4"), ("seq", "<u4"), ("ack", "<u4"),
                      ("payload_off", "<u4"), ("payload_len", "<u4"), ("tcp_off", "<u2"), ("flags", "<u2"),
                      ("lookup_only", "u1"), ("reserved", "u1", (3,))])
GROUP_DTYPE = np.dtype([("flow_id", "<u4"), ("start", "<u4"), ("count", "<u4"), ("first_packet", "<u4")])
assert SEG_DTYPE.itemsize == 32 and GROUP_DTYPE.itemsize == 16

TCP_UNGROUPED = 0xFFFFFFFF
# flags bits (header bytes 12..13 & 0x1FF)
TCP_FIN, TCP_SYN, TCP_RST, TCP_PSH, TCP_ACK, TCP_URG, TCP_ECE, TCP_CWR, TCP_NS = (1 << b for b in range(9))
# pairs one workgroup of the sort's scatter ranks (gpd_radix_sort.h kSortTile)
SORT_TILE = 8192

TCPSEG_EXPORTS = {
    # include/gpd_tcpassembly.h — name: (restype, argtypes)
    "gpd_tcp_segments": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.POINTER(GpdResult), C.c_void_p,
                                   C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]),
}

_bound = False


def tcpseg_lib():
    """The loaded library with the hand-off's signature bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in TCPSEG_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


def _call(parser, dbatch, dres, fid, id_bound, segs, groups, m, stream):
    cnt, ng, un = C.c_uint64(), C.c_uint64(), C.c_uint64()
    b, r = dbatch.c_batch(), dres.c_result()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = tcpseg_lib().gpd_tcp_segments(parser.ctx().h, C.byref(b), C.byref(r), p(fid), id_bound, p(segs),
                                       p(groups), m, C.byref(cnt), C.byref(ng), C.byref(un),
                                       C.c_void_p(stream.cuda_stream))
    return rc, int(cnt.value), int(ng.value), int(un.value)


def TCPSegments(parser, dbatch, dres, flow_id=None, table=None, max_out: Optional[int] = None, stream=None,
                id_bound: Optional[int] = None):
    """The segment hand-off of a batch `parser` decoded into `dres` (hdr_off required).  Returns
    (segs, groups, count, ngroups, ungrouped): uint8 device tensors of count x 32-byte and
    ngroups x 16-byte records (SEG_DTYPE, GROUP_DTYPE).  Synchronises `stream`.

    flow_id None: the segments in packet order, no groups.  flow_id (the int32 device tensor of
    FlowTable.Insert for this batch) with `table` (the FlowTable; or id_bound, its capacity):
    the segments ordered by flow id and, within one id, by packet; ids at or above the capacity
    (FLOW_FULL, FLOW_COLLISION-flagged, FLOW_NONE) form the last group, TCP_UNGROUPED, in packet
    order.  max_out None sizes the arrays with a first call; otherwise it is their capacity, and
    the call raises (GPD_ERR_INVALID) when the hand-off has more segments."""
    from .parser import _torch
    torch = _torch()
    if dres.hdr_off is None:
        raise ValueError("TCPSegments needs a DeviceResult with hdr_off")
    dev = torch.device("cuda", parser.device)
    s = stream if stream is not None else torch.cuda.current_stream(parser.device)
    fid, bound = None, 0
    if flow_id is not None:
        if flow_id.numel() != dbatch.n or flow_id.element_size() != 4:
            raise ValueError("TCPSegments: flow_id must hold one 32-bit id per packet")
        if id_bound is None:
            if table is None:
                raise ValueError("TCPSegments: flow_id needs the FlowTable (or id_bound)")
            id_bound = table.Stats(s)["capacity"]
        fid, bound = flow_id.contiguous(), min(int(id_bound), 0xFFFFFFFF)
    if max_out is None:
        rc, m, _, _ = _call(parser, dbatch, dres, fid, bound, None, None, 0, s)
        check(rc, "gpd_tcp_segments")
    else:
        m = int(max_out)
    segs = torch.empty(max(m, 1) * SEG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    groups = torch.empty(max(m, 1) * GROUP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    # (a max_out of 0 given by the caller is a capacity like any other, not the sizing call: the
    # arrays go in, and segments that do not fit raise)
    sizing = m == 0 and max_out is None
    rc, cnt, ng, un = _call(parser, dbatch, dres, fid, bound, None if sizing else segs, None if sizing else groups,
                            m, s)
    check(rc, "gpd_tcp_segments")
    return segs[:cnt * SEG_DTYPE.itemsize], groups[:ng * GROUP_DTYPE.itemsize], cnt, ng, un


def segments_to_host(segs, count: int) -> np.ndarray:
    """SEG_DTYPE[count] copy of TCPSegments' records; raises when `segs` holds fewer (an
    assembler fed only the first records would report gaps that are not in the capture)."""
    k = segs.numel() // SEG_DTYPE.itemsize
    if k < count:
        raise ValueError(f"segments_to_host: {count} segments, `segs` holds {k}; "
                         f"call TCPSegments with a larger max_out")
    return segs[:count * SEG_DTYPE.itemsize].cpu().numpy().view(SEG_DTYPE).copy()


def groups_to_host(groups, ngroups: int) -> np.ndarray:
    """GROUP_DTYPE[ngroups] copy of TCPSegments' group records."""
    k = groups.numel() // GROUP_DTYPE.itemsize
    if k < ngroups:
        raise ValueError(f"groups_to_host: {ngroups} groups, `groups` holds {k}")
    return groups[:ngroups * GROUP_DTYPE.itemsize].cpu().numpy().view(GROUP_DTYPE).copy()
