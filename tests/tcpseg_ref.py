"""TEST INFRASTRUCTURE ONLY: CPU restatement of the tcpassembly hand-off (gpd_tcp_segments,
include/gpd_tcpassembly.h), from the oracle's results and the packet bytes.

For every packet the application calls Assembler.AssembleWithTimestamp(netFlow, &tcp, ts)
(tcpassembly/assembly.go:533-607) with the parser's TCP object as DecodeLayers left it.  The
hand-off lists the packets that call does not ignore (:535), with what it reads:

  * candidates are the packets the flow table keys (a network and a transport endpoint type in
    the status word, both header offsets below 0xFFFF) whose transport type is TCPPort (4);
  * t.Payload is the TCP object's Payload range of the oracle's ext record (obj[5]) — whatever
    the IPv4/IPv6 length trimming, Ethernet padding, a cut capture or TCP options made of it;
  * Seq, Ack and the flag bits are read where the header offsets word says t's fields were read;
  * !SYN && !FIN && !RST && len(Payload) == 0 is dropped (:535); lookup_only is getConnection's
    `end` argument, !SYN && len(Payload) == 0 (:550-551).

Grouping is numpy's stable argsort over min(flow_id, id_bound); nothing here shares code with the
kernels.
"""
from __future__ import annotations

import numpy as np

OBJ_TCP = 5
FIN, SYN, RST = 1, 2, 4
FLOW_NONE = 0xFFFFFFFF
UNGROUPED = 0xFFFFFFFF

SEG_DTYPE = np.dtype([("packet", "<u4"), ("flow_id", "<u4"), ("seq", "<u4"), ("ack", "<u4"),
                      ("payload_off", "<u4"), ("payload_len", "<u4"), ("tcp_off", "<u2"), ("flags", "<u2"),
                      ("lookup_only", "u1"), ("reserved", "u1", (3,))])
GROUP_DTYPE = np.dtype([("flow_id", "<u4"), ("start", "<u4"), ("count", "<u4"), ("first_packet", "<u4")])


def segments(batch, res, flow_id=None) -> np.ndarray:
    """SEG_DTYPE records in packet order for an oracle BatchResult decoded with ext records."""
    if res.ext is None or res.hdr_off is None:
        raise ValueError("the segment oracle reads the TCP object from ext records and hdr_off")
    st = res.status.astype(np.uint32)
    ho = res.hdr_off.astype(np.uint32)
    cand = (((st >> 20) & 15) != 0) & (((st >> 24) & 15) == 4) & ((ho & 0xFFFF) != 0xFFFF) & ((ho >> 16) != 0xFFFF)
    cand &= ((res.ext["obj_valid"].astype(np.uint32) >> OBJ_TCP) & 1) == 1
    out = []
    for i in np.nonzero(cand)[0]:
        i = int(i)
        o = res.ext["obj"][i, OBJ_TCP]
        p = batch.packet(i)
        to = int(ho[i] >> 16)
        flags = ((int(p[to + 12]) << 8) | int(p[to + 13])) & 0x1FF
        plen = int(o["payload_len"])
        if not flags & (SYN | FIN | RST) and plen == 0:
            continue
        r = np.zeros((), SEG_DTYPE)
        r["packet"] = i
        r["flow_id"] = FLOW_NONE if flow_id is None else int(flow_id[i])
        r["seq"] = int.from_bytes(bytes(p[to + 4:to + 8]), "big")
        r["ack"] = int.from_bytes(bytes(p[to + 8:to + 12]), "big")
        r["payload_off"] = int(o["payload_off"])
        r["payload_len"] = plen
        r["tcp_off"] = int(o["contents_off"]) & 0xFFFF
        r["flags"] = flags
        r["lookup_only"] = int(not flags & SYN and plen == 0)
        out.append(r)
    return np.array(out, SEG_DTYPE) if out else np.zeros(0, SEG_DTYPE)


def group(segs: np.ndarray, id_bound: int):
    """(segs ordered by min(flow_id, id_bound) then packet, GROUP_DTYPE groups, ungrouped)."""
    key = np.minimum(segs["flow_id"].astype(np.uint64), np.uint64(id_bound))
    order = np.argsort(key, kind="stable")
    s, k = segs[order], key[order]
    if not len(s):
        return s, np.zeros(0, GROUP_DTYPE), 0
    heads = np.nonzero(np.concatenate(([True], k[1:] != k[:-1])))[0]
    g = np.zeros(len(heads), GROUP_DTYPE)
    g["start"] = heads
    g["count"] = np.diff(np.concatenate((heads, [len(s)])))
    g["first_packet"] = s["packet"][heads]
    un = k[heads] >= id_bound
    g["flow_id"] = np.where(un, UNGROUPED, k[heads]).astype(np.uint32)
    return s, g, int(g["count"][-1]) if un[-1] else 0


def hand_off(batch, res, flow_id=None, id_bound=0):
    """What gpd_tcp_segments returns: (segs, groups, count, ngroups, ungrouped)."""
    s = segments(batch, res, flow_id)
    if flow_id is None:
        return s, np.zeros(0, GROUP_DTYPE), len(s), 0, 0
    s, g, un = group(s, id_bound)
    return s, g, len(s), len(g), un
