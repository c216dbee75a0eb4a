"""TCP connection tracking: reassembly's bidirectional connection, packet direction and
TCPSimpleFSM for a decoded batch, on the GPU.

The flow table is directional, as tcpassembly's keys are.  The reference's newer assembler,
`reassembly`, pairs a key with its Reverse() into one connection (StreamPool.getHalf,
reassembly/memory.go:169-206), gives each packet a TCPFlowDirection, and offers TCPSimpleFSM
(reassembly/tcpcheck.go:119-246) for Stream.Accept to drop what a real stack would reject.  A
`ConnTracker` does the three for every TCP packet of an HBM-resident batch that `FlowTable.Insert`
just keyed, and keeps one FSM per connection on the device from batch to batch
(gpd_tcp_tracker_run, include/gpd_tcptrack.h).  The verdict byte's accept bit is a keep mask for
`pcapwrite.select` and both writers (`keep_mask`).

The entry points are bound onto the loaded library here, on first use, from TCPTRACK_EXPORTS.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import GpdBatch, GpdResult, check

# tcpcheck.go:131-138
TCPStateClosed, TCPStateSynSent, TCPStateEstablished, TCPStateCloseWait, TCPStateLastAck, TCPStateReset = range(6)
_STATE_NAMES = ("Closed", "SynSent", "Established", "CloseWait", "LastAck", "Reset")
# the direction bit of a verdict (reassembly/tcpassembly.go TCPFlowDirection: false = client to server)
TCPDirClientToServer, TCPDirServerToClient = 0, 1

V_ACCEPT, V_DIR, V_STATE_SHIFT, V_STATE_MASK, V_FSM_DIR = 0x01, 0x02, 2, 0x1C, 0x20
UNTRACKED = 0xFF
C_STATE_MASK, C_FSM_DIR = 0x07, 0x08
FLOW_NONE = 0xFFFFFFFF
# packets one workgroup of the scan takes (gpd_tcptrack.hip kTrkTile), and tiles the aggregate
# scan takes between barriers (kAggRound)
SCAN_TILE = 2048
AGG_ROUND = 256


class GpdTcpTrackOpts(C.Structure):
    _fields_ = [("support_missing_establishment", C.c_uint32), ("reserved", C.c_uint32)]


TCPTRACK_EXPORTS = {
    # include/gpd_tcptrack.h — name: (restype, argtypes)
    "gpd_tcp_tracker_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GpdTcpTrackOpts), C.POINTER(C.c_void_p)]),
    "gpd_tcp_tracker_destroy": (None, [C.c_void_p]),
    "gpd_tcp_tracker_run": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.POINTER(GpdResult), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "gpd_tcp_tracker_states": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpd_tcp_tracker_forget": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "gpd_tcp_tracker_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
}

_bound = False


def tcptrack_lib():
    """The loaded library with the tracker's signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in TCPTRACK_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


# verdict: uint8 device tensor [n]; conn_id: int32 device tensor [n] (the u32 bit patterns) or None
TrackResult = namedtuple("TrackResult", "verdict conn_id tracked accepted rejected connections")


def state_name(state: int) -> str:
    """TCPSimpleFSM.String() (tcpcheck.go:148-164) for a state number."""
    return _STATE_NAMES[state] if 0 <= int(state) < len(_STATE_NAMES) else "?"


def verdict_state(v):
    """The state after, from a verdict byte (or an array of them; meaningless for UNTRACKED)."""
    return (np.asarray(v) & V_STATE_MASK) >> V_STATE_SHIFT


class ConnTracker:
    """One TCPSimpleFSM per connection of `table`, on the device of `parser`."""

    def __init__(self, parser, table, support_missing_establishment: bool = False):
        self._parser = parser
        self._table = table  # (kept alive: the object reads its records)
        self.device = parser.device
        self.support_missing_establishment = bool(support_missing_establishment)
        self._h = None
        h = C.c_void_p()
        opts = GpdTcpTrackOpts(1 if support_missing_establishment else 0, 0)
        check(tcptrack_lib().gpd_tcp_tracker_create(parser.ctx().h, table.h, C.byref(opts), C.byref(h)),
              "gpd_tcp_tracker_create")
        self._h = h
        self.id_bound = int(table.Stats()["capacity"])

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None and h.value:
            tcptrack_lib().gpd_tcp_tracker_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise ValueError("ConnTracker is closed")
        return self._h

    def _stream(self, stream):
        from .parser import _torch
        return stream if stream is not None else _torch().cuda.current_stream(self.device)

    def TrackBatch(self, dbatch, dres, flow_id, want_conn_id: bool = False, stream=None) -> TrackResult:
        """The verdicts of a batch `parser` decoded into `dres` (hdr_off required) and
        `FlowTable.Insert` keyed into `flow_id` (its int32 device tensor), on the same stream.
        Insert's index_base must grow from batch to batch.  Synchronises `stream`."""
        from .parser import _torch
        torch = _torch()
        if dres.hdr_off is None:
            raise ValueError("TrackBatch needs a DeviceResult with hdr_off")
        if flow_id.numel() != dbatch.n or flow_id.element_size() != 4:
            raise ValueError("TrackBatch: flow_id must hold one 32-bit id per packet")
        dev = torch.device("cuda", self.device)
        n = dbatch.n
        fid = flow_id.contiguous()
        verdict = torch.empty(n, dtype=torch.uint8, device=dev)
        conn = torch.empty(n, dtype=torch.int32, device=dev) if want_conn_id else None
        out = (C.c_uint64 * 4)()
        b, r = dbatch.c_batch(), dres.c_result()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        check(tcptrack_lib().gpd_tcp_tracker_run(self._handle(), C.byref(b), C.byref(r), p(fid), p(verdict), p(conn),
                                                 out, C.c_void_p(self._stream(stream).cuda_stream)),
              "gpd_tcp_tracker_run")
        return TrackResult(verdict, conn, int(out[0]), int(out[1]), int(out[2]), int(out[3]))

    def states(self, stream=None) -> np.ndarray:
        """uint8[id_bound]: the carried byte of every flow record (state in bits 0..2, t.dir in
        bit 3; only a connection's own record carries it)."""
        from .parser import _torch
        torch = _torch()
        s = self._stream(stream)
        t = torch.empty(max(self.id_bound, 1), dtype=torch.uint8, device=torch.device("cuda", self.device))
        check(tcptrack_lib().gpd_tcp_tracker_states(self._handle(), C.c_void_p(t.data_ptr()), C.c_void_p(s.cuda_stream)),
              "gpd_tcp_tracker_states")
        s.synchronize()
        return t.cpu().numpy()[:self.id_bound].copy()

    def forget(self, ids, stream=None) -> None:
        """Returns the connections `ids` (a device tensor or an array of connection ids) to the
        fresh state."""
        from .parser import _torch
        torch = _torch()
        if isinstance(ids, torch.Tensor):
            if ids.element_size() != 4:
                raise ValueError("forget: ids must be 32-bit")
            t = ids.contiguous().to(torch.device("cuda", self.device))
        else:
            a = np.ascontiguousarray(np.asarray(ids, np.uint32))
            t = torch.from_numpy(a.view(np.int32)).to(torch.device("cuda", self.device))
        if t.numel() == 0:
            return
        s = self._stream(stream)
        check(tcptrack_lib().gpd_tcp_tracker_forget(self._handle(), C.c_void_p(t.data_ptr()), t.numel(),
                                                    C.c_void_p(s.cuda_stream)), "gpd_tcp_tracker_forget")
        s.synchronize()  # (t may be released on return)

    def reset(self, stream=None) -> None:
        """Every connection back to the fresh state; call it when the flow table is reset."""
        check(tcptrack_lib().gpd_tcp_tracker_reset(self._handle(), C.c_void_p(self._stream(stream).cuda_stream)),
              "gpd_tcp_tracker_reset")


def NewConnTracker(parser, table, support_missing_establishment: bool = False) -> ConnTracker:
    """A StreamPool of connections over `table` (a FlowTable), each with
    NewTCPSimpleFSM(TCPSimpleFSMOptions{SupportMissingEstablishment})."""
    return ConnTracker(parser, table, support_missing_establishment)


def keep_mask(result: TrackResult, untracked: bool = True):
    """The uint8 device mask `pcapwrite.select` / `write_device` take: 1 for the packets the FSM
    accepted and, with `untracked`, for those it does not track (UDP, undecodable, no record)."""
    v = result.verdict
    keep = (v & V_ACCEPT).bool() & (v != UNTRACKED)
    if untracked:
        keep = keep | (v == UNTRACKED)
    return keep.to(v.dtype)
