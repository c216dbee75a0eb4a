"""Shared inputs of the stateful assembler's tests (tests/test_tcpasm.py, tests/test_tcpasm_gpu.py):
a crafted hand-off (tests/tcpstream_cases.crafted) cut at packet indices into batches of their
own, and the text forms the host walk program reads and writes."""
from __future__ import annotations

import numpy as np

import tcpseg_ref as TS
from gopacket_amd.batch import PacketBatch


def regroup(segs):
    """GROUP_DTYPE records for segs[] ordered by flow id, then packet."""
    grp, at = [], 0
    ids = segs["flow_id"]
    while at < len(segs):
        e = at
        while e < len(segs) and ids[e] == ids[at]:
            e += 1
        grp.append((int(ids[at]), at, e - at, int(segs["packet"][at])))
        at = e
    return np.array(grp, TS.GROUP_DTYPE)


def cut(batch, segs, lo, hi):
    """Packets [lo, hi) of a crafted whole as a batch of their own, with their hand-off:
    (batch, segs, groups), packet indices counted from lo."""
    sel = segs[(segs["packet"] >= lo) & (segs["packet"] < hi)].copy()
    sel["packet"] -= lo
    sub = PacketBatch.from_packets([bytes(batch.packet(i)) for i in range(lo, hi)])
    return sub, sel, regroup(sel)


def cut_all(batch, segs, cuts):
    """cut() for consecutive ranges: cuts = [0, a, b, ..., n]."""
    return [cut(batch, segs, cuts[k], cuts[k + 1]) for k in range(len(cuts) - 1)]


def set_payloads(batch, segs, payloads):
    """Writes payloads[k] over the payload of segs[k] in the batch's data (crafted() fills at
    random)."""
    for r, p in zip(segs, payloads):
        at = int(batch.offset[int(r["packet"])]) + int(r["payload_off"])
        batch.data[at:at + len(p)] = np.frombuffer(bytes(p), np.uint8)
