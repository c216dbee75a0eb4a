"""TEST INFRASTRUCTURE ONLY: the oracle of the IPv4 defragmentation (gpd_ip4_defrag_run,
include/gpd_ip4reasm.h).  oracle/ip4defrag_ref.py restates ip4defrag's IPv4Defragmenter and is
pinned by defrag_test.go's fixtures (tests/golden/defrag_vectors.json); this module drives it,
unchanged, over hand-off records in packet order across batches and derives what the entry
point returns: the outcome per record, the datagram records, the datagrams' bytes under the
header rule of include/gpd_ip4reasm.h, and the SHORT_SLICE flag.

The only addition to the restated defragmenter is a fragment list that remembers what its last
build did (the list's length, and whether a slice started past its payload's end): build itself
is the oracle's.
"""
import os
import struct
import sys
from collections import namedtuple

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ip4defrag_ref as R  # noqa: E402
from gopacket_amd.defrag import FRAG_DTYPE, FRAG_INSERT, FRAG_WHOLE  # noqa: E402

OUTCOME_DTYPE = np.dtype([("what", "<u4"), ("datagram", "<u4")])
DGRAM_DTYPE = np.dtype([("packet", "<u4"), ("frag", "<u4"), ("byte_off", "<u8"), ("payload_len", "<u4"),
                        ("nfrags", "<u4"), ("length", "<u2"), ("id", "<u2"), ("ihl", "u1"), ("protocol", "u1"),
                        ("flags", "<u2")])
FILED, COMPLETE, REJECTED, UNCHANGED, HOLE, INVALID, LIST_FULL = range(7)
D_SHORT_SLICE = 1

ERR_WHAT = {"defrag: building - hole found": HOLE, "defrag: building - invalid fragment": INVALID}


class TracedList(R.FragmentList):
    """fragmentList whose build also notes the list's length and the slices Go would panic on."""

    def build(self, f):
        out, err = super().build(f)
        if out is not None:
            short, cur = False, 0
            for e in self.frags:  # the offsets of build's loop (defrag.go:283-306), nothing else
                off8 = (e.frag_offset * 8) & 0xFFFF
                if off8 == cur:
                    cur = (cur + e.length - 20) & 0xFFFF
                else:
                    short |= ((cur - off8) & 0xFFFF) > len(e.payload)
                    cur = (cur + off8) & 0xFFFF
            out.nfrags, out.short = len(self.frags), short
        return out, err


def ip_checksum(h: bytes) -> int:
    s = sum(struct.unpack(">%dH" % (len(h) // 2), h))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def datagram_bytes(header: bytes, payload: bytes) -> bytes:
    """The completing fragment's header bytes with the three patches, then the payload."""
    h = bytearray(header)
    total = len(h) + len(payload)
    h[2:4] = struct.pack(">H", total if total <= 65535 else 0)
    h[6:8] = b"\0\0"
    h[10:12] = b"\0\0"
    h[10:12] = struct.pack(">H", ip_checksum(bytes(h)))
    return bytes(h) + payload


RefResult = namedtuple("RefResult", "outcomes dgrams offset caplen bytes payloads")


class RefDefragmenter:
    """The restated IPv4Defragmenter fed batch by batch."""

    def __init__(self):
        self.d = R.NewIPv4Defragmenter()

    def run(self, batch, frags, ts=None, now=0) -> RefResult:
        """frags: FRAG_DTYPE records of `batch` (a PacketBatch) in packet order; ts: None or
        per-packet timestamps."""
        outcomes = np.zeros(len(frags), OUTCOME_DTYPE)
        dg, chunks, payloads, pos = [], [], [], 0
        for i, rec in enumerate(frags):
            pk = int(rec["packet"])
            o0 = int(batch.offset[pk])
            packet = bytes(batch.data[o0:o0 + int(batch.caplen[pk])])
            v = int(rec["verdict"])
            if v == FRAG_INSERT:
                key = (bytes(rec["src"]), bytes(rec["dst"]), int(rec["id"]))
                if key not in self.d.ip_flows:
                    self.d.ip_flows[key] = TracedList()  # (what the call would create, traced)
            t = now if ts is None else int(ts[pk])
            out, err = self.d.DefragIPv4WithTimestamp(rec, packet, t)
            if v == FRAG_WHOLE:
                assert out == "unchanged"
                outcomes[i]["what"] = UNCHANGED
            elif v != FRAG_INSERT:
                assert err is not None
                outcomes[i]["what"] = REJECTED
            elif out is not None:
                net, ihl = int(rec["net_off"]), int(rec["ihl"])
                header = packet[net:net + 4 * ihl]
                r = np.zeros((), DGRAM_DTYPE)
                r["packet"], r["frag"], r["byte_off"], r["payload_len"] = pk, i, pos, len(out.payload)
                r["nfrags"], r["length"], r["id"], r["ihl"] = out.nfrags, out.length, out.ident, out.ihl
                r["protocol"], r["flags"] = header[9], D_SHORT_SLICE if out.short else 0
                outcomes[i] = (COMPLETE, len(dg))
                dg.append(r)
                b = datagram_bytes(header, out.payload)
                chunks.append(b)
                payloads.append(out.payload)
                pos += len(b)
            elif err is None:
                outcomes[i]["what"] = FILED
            elif err in ERR_WHAT:
                outcomes[i]["what"] = ERR_WHAT[err]
            else:
                assert err.startswith("defrag: Fragment List hits its maximum"), err
                outcomes[i]["what"] = LIST_FULL
        dgrams = np.array(dg, DGRAM_DTYPE) if dg else np.zeros(0, DGRAM_DTYPE)
        return RefResult(outcomes, dgrams, dgrams["byte_off"].astype(np.uint32),
                         np.array([len(c) for c in chunks], np.uint32),
                         np.frombuffer(b"".join(chunks), np.uint8), payloads)

    def discard(self, t) -> int:
        return self.d.DiscardOlderThan(t)

    def stats(self) -> dict:
        fl = self.d.ip_flows.values()
        return {"lists": len(fl), "fragments": sum(len(x.frags) for x in fl),
                "bytes": sum(len(e.payload) for x in fl for e in x.frags)}
