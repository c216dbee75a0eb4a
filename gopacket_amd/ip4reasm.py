"""IPv4 defragmentation: ip4defrag's datagrams rebuilt on the GPU.

`defrag.IPv4Fragments` hands over the packets of a decoded batch that
IPv4Defragmenter.DefragIPv4WithTimestamp (ip4defrag/defrag.go:86-135) does not return untouched.
`NewIPv4Defragmenter(parser)` is the stateful rest on the device (include/gpd_ip4reasm.h):
`DefragBatch` reports per hand-off record what that call would have returned, as if it were made
for the records in order (fragmentList.insert :216-273, build :278-328, the 8,192-fragment flush
:120-125), keeps the unfinished fragment lists from batch to batch in device memory, and returns
the reassembled datagrams as a DeviceBatch the parser decodes with first layer IPv4:

    out, n = IPv4Fragments(parser, dbatch, dres)
    d = NewIPv4Defragmenter(parser)
    res = d.DefragBatch(dbatch, out, n, ts=ts_ns)        # DefragResult
    ip4 = DecodingLayerParser(LayerTypeIPv4, ...)         # same decoders
    ip4.decode_device(res.batch, DeviceResult(res.batch.n))

A datagram's bytes are the completing fragment's header (options included) with Flags and
FragOffset zeroed, the total length and the header checksum set, then the payload; the record
keeps build's own values (Length = Highest, Checksum = 0 in the reference's struct).

The entry points are bound onto the loaded library here, on first use, from IP4REASM_EXPORTS:
they live in their own header and are not part of _lib.EXPORTS.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np

from . import _lib
from ._lib import GpdBatch, check
from .defrag import FRAG_DTYPE, frag_error

OUTCOME_DTYPE = np.dtype([("what", "<u4"), ("datagram", "<u4")])
DGRAM_DTYPE = np.dtype([("packet", "<u4"), ("frag", "<u4"), ("byte_off", "<u8"), ("payload_len", "<u4"),
                        ("nfrags", "<u4"), ("length", "<u2"), ("id", "<u2"), ("ihl", "u1"), ("protocol", "u1"),
                        ("flags", "<u2")])
assert OUTCOME_DTYPE.itemsize == 8 and DGRAM_DTYPE.itemsize == 32

FILED, COMPLETE, REJECTED, UNCHANGED, HOLE, INVALID, LIST_FULL = range(7)
D_SHORT_SLICE = 1
MAX_LIST_LEN = 8192

# the errors DefragIPv4WithTimestamp returns (defrag.go:122-124, 295, 303), by outcome
OUTCOME_ERRORS = {
    HOLE: "defrag: building - hole found",
    INVALID: "defrag: building - invalid fragment",
    LIST_FULL: "defrag: Fragment List hits its maximumsize(%d), without success. Flushing the list" % MAX_LIST_LEN,
}


def outcome_error(what: int, rec=None) -> Optional[str]:
    """The error text of an outcome (None for FILED, COMPLETE and UNCHANGED); REJECTED needs the
    hand-off record, whose verdict has securityChecks' text."""
    what = int(what)
    if what == REJECTED:
        return frag_error(rec) if rec is not None else "defrag: rejected by securityChecks"
    return OUTCOME_ERRORS.get(what)


IP4REASM_EXPORTS = {
    # include/gpd_ip4reasm.h — name: (restype, argtypes)
    "gpd_ip4_defrag_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "gpd_ip4_defrag_destroy": (None, [C.c_void_p]),
    "gpd_ip4_defrag_run": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]),
    "gpd_ip4_defrag_discard": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "gpd_ip4_defrag_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
}

_bound = False


def ip4reasm_lib():
    """The loaded library with the defragmenter's signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in IP4REASM_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


DefragResult = namedtuple("DefragResult", "outcomes dgrams batch ndgrams noutcomes nbytes nlists")
HostDefrag = namedtuple("HostDefrag", "outcomes dgrams offset caplen bytes")


class IPv4Defragmenter:
    """ip4defrag.IPv4Defragmenter on the device of `parser`: the fragment lists of the running
    datagrams live in device memory between DefragBatch calls."""

    def __init__(self, parser):
        self._parser = parser
        self.device = parser.device
        h = C.c_void_p()
        check(ip4reasm_lib().gpd_ip4_defrag_create(parser.ctx().h, C.byref(h)), "gpd_ip4_defrag_create")
        self._h = h

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None and h.value:
            ip4reasm_lib().gpd_ip4_defrag_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise ValueError("IPv4Defragmenter: closed")
        return self._h

    def _run(self, dbatch, frags, count, ts, now, outcomes, dgrams, max_dgrams, offset, caplen, byts, max_bytes, s):
        out = (C.c_uint64 * 4)()
        b = dbatch.c_batch()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = ip4reasm_lib().gpd_ip4_defrag_run(self._handle(), C.byref(b), p(frags), count, p(ts), int(now),
                                               p(outcomes), p(dgrams), max_dgrams, p(offset), p(caplen), p(byts),
                                               max_bytes, out, C.c_void_p(s.cuda_stream))
        return rc, tuple(int(v) for v in out)

    def DefragBatch(self, dbatch, frags, count: int, ts=None, now: int = 0, gather: bool = True,
                    max_dgrams: Optional[int] = None, max_bytes: Optional[int] = None, stream=None) -> DefragResult:
        """DefragIPv4WithTimestamp for the hand-off `frags`, `count` as IPv4Fragments(parser,
        dbatch, dres) returned them for `dbatch` (complete: a hand-off cut short by max_out is
        refused).  ts: None, or a device tensor of dbatch.n uint64 nanosecond timestamps (int64
        bits are taken as they are); without it every fragment's LastSeen is `now`.

        Returns DefragResult(outcomes, dgrams, batch, ndgrams, noutcomes, nbytes, nlists): uint8
        device tensors of count x 8-byte outcomes (OUTCOME_DTYPE) and ndgrams x 32-byte datagram
        records (DGRAM_DTYPE), and the datagrams as a DeviceBatch (None with gather=False).
        max_dgrams / max_bytes None size the arrays with a first call; otherwise they are
        capacities, and the call raises (GPD_ERR_INVALID) when more is needed: nothing is
        written then and the carried lists are unchanged.  Synchronises `stream`."""
        from .parser import DeviceBatch, _torch
        torch = _torch()
        dev = torch.device("cuda", self.device)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        count = int(count)
        if count and frags.numel() * frags.element_size() < count * FRAG_DTYPE.itemsize:
            raise ValueError(f"DefragBatch: {count} fragments, `frags` holds fewer; a partial hand-off would "
                             f"report holes or never complete the datagrams")
        if ts is not None and ts.numel() * ts.element_size() < dbatch.n * 8:
            raise ValueError("DefragBatch: ts holds fewer than dbatch.n timestamps")
        args = (dbatch, frags if count else None, count, ts, now)
        if max_dgrams is None or (gather and max_bytes is None):
            rc, out = self._run(*args, None, None, 0, None, None, None, 0, s)
            check(rc, "gpd_ip4_defrag_run")
            max_dgrams = out[0] if max_dgrams is None else int(max_dgrams)
            max_bytes = out[2] if max_bytes is None else int(max_bytes)
        max_dgrams = int(max_dgrams)
        max_bytes = int(max_bytes) if gather else 0
        outcomes = torch.empty(max(count, 2) * OUTCOME_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        dgrams = torch.empty(max(max_dgrams, 1) * DGRAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        desc = byts = offset = caplen = None
        if gather:
            m = max((max_dgrams + 15) // 16 * 16, 16)  # caplen[] right behind offset[] (DeviceBatch)
            desc = torch.zeros(2 * m, dtype=torch.int32, device=dev)
            offset, caplen = desc[:m], desc[m:]
            byts = torch.empty((max(max_bytes, 1) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        rc, out = self._run(*args, outcomes, dgrams, max_dgrams, offset, caplen, byts, max_bytes, s)
        check(rc, "gpd_ip4_defrag_run")
        nd, no, nb, nl = out
        batch = None
        if gather:
            batch = DeviceBatch.from_tensors(byts, nb, offset[:nd], caplen[:nd], device=self.device)
        return DefragResult(outcomes[:no * OUTCOME_DTYPE.itemsize], dgrams[:nd * DGRAM_DTYPE.itemsize], batch,
                            nd, no, nb, nl)

    def DiscardOlderThan(self, t: int) -> int:
        """DiscardOlderThan (defrag.go:140-151): drops the lists last touched before `t`
        (nanoseconds, the clock of DefragBatch's ts / now); returns their count."""
        n = C.c_uint64()
        check(ip4reasm_lib().gpd_ip4_defrag_discard(self._handle(), int(t), C.byref(n)), "gpd_ip4_defrag_discard")
        return int(n.value)

    def stats(self) -> dict:
        """The lists, fragments and payload bytes currently held."""
        out = (C.c_uint64 * 3)()
        check(ip4reasm_lib().gpd_ip4_defrag_stats(self._handle(), out), "gpd_ip4_defrag_stats")
        return {"lists": int(out[0]), "fragments": int(out[1]), "bytes": int(out[2])}


def NewIPv4Defragmenter(parser) -> IPv4Defragmenter:
    """NewIPv4Defragmenter (defrag.go:353-357) on the parser's device."""
    return IPv4Defragmenter(parser)


def defrag_to_host(result: DefragResult) -> HostDefrag:
    """Host copies of a DefragResult: OUTCOME_DTYPE[noutcomes], DGRAM_DTYPE[ndgrams], and the
    datagram batch's offset, caplen (uint32) and bytes (uint8[nbytes]); None without a batch."""
    outcomes = result.outcomes.cpu().numpy().view(OUTCOME_DTYPE).copy()
    dgrams = result.dgrams.cpu().numpy().view(DGRAM_DTYPE).copy()
    if len(outcomes) != result.noutcomes or len(dgrams) != result.ndgrams:
        raise ValueError("defrag_to_host: the tensors hold fewer records than the counts say")
    if result.batch is None:
        return HostDefrag(outcomes, dgrams, None, None, None)
    b = result.batch
    return HostDefrag(outcomes, dgrams, b.offset.cpu().numpy().view(np.uint32).copy(),
                      b.caplen.cpu().numpy().view(np.uint32).copy(), b.data[:result.nbytes].cpu().numpy().copy())
