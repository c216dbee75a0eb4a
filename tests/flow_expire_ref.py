"""TEST INFRASTRUCTURE ONLY: the model of a flow table whose records can leave
(include/gpd_flow_expire.h).  A dict pool on top of oracle/flow_ref.py's group(): StreamPool's
map with remove (tcpassembly/assembly.go:659-676) and the idle test of FlushOlderThan
(conn.lastSeen.Before(t)), in packet sequence numbers.  Slot indices are not modelled, only
relations: which keys are in the pool, with which counters; a key that comes back after its
removal is a new record with fresh counters."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import flow_ref  # noqa: E402


def reverse_key(k: bytes) -> bytes:
    """The key of the other direction, in flow_ref.flow_keys' 40-byte layout."""
    return k[16:32] + k[0:16] + k[34:36] + k[32:34] + k[36:40]


class Pool:
    def __init__(self):
        self.flows = {}  # key bytes -> {first, last, packets, bytes}

    def insert(self, batch, res, index_base: int = 0):
        """The pool after the batch; returns each packet's key (None without one)."""
        add, per_packet = flow_ref.group(batch, res, index_base)
        self.merge(add)
        return per_packet

    def merge(self, add: dict) -> None:
        for k, f in add.items():
            g = self.flows.get(k)
            if g is None:
                self.flows[k] = dict(f)
            else:
                g["first"] = min(g["first"], f["first"])
                g["last"] = max(g["last"], f["last"])
                g["packets"] += f["packets"]
                g["bytes"] += f["bytes"]

    def remove(self, keys) -> None:
        """StreamPool.remove; keys not in the pool are ignored."""
        for k in keys:
            self.flows.pop(k, None)

    def expire(self, cutoff: int, held=(), pairs: bool = False):
        """Removes every key with last < cutoff that is not in `held`; with `pairs`, only if its
        reverse qualifies as well (a missing reverse, or a key that is its own reverse, is a
        complete pair).  Returns the removed keys."""
        held = set(held)
        cand = {k for k, f in self.flows.items() if f["last"] < cutoff and k not in held}
        if pairs:
            cand = {k for k in cand if reverse_key(k) not in self.flows or reverse_key(k) in cand}
        self.remove(cand)
        return cand

    def __len__(self):
        return len(self.flows)


def same_as_export(pool: Pool, recs) -> bool:
    """An Export() equals the pool key by key (first, last, packets, bytes)."""
    got = {flow_ref.record_key(r): {f: int(r[f]) for f in ("first", "last", "packets", "bytes")} for r in recs}
    return len(got) == len(recs) and got == pool.flows


def key_of(src: int, dst: int, sport: int, dport: int, tp: int = 4) -> bytes:
    """The 40-byte key of an IPv4 TCP (tp 4) or UDP (5) packet from its addresses and ports."""
    k = np.zeros(40, np.uint8)
    k[0:4] = np.frombuffer(int(src).to_bytes(4, "big"), np.uint8)
    k[16:20] = np.frombuffer(int(dst).to_bytes(4, "big"), np.uint8)
    k[32:34] = np.frombuffer(int(sport).to_bytes(2, "big"), np.uint8)
    k[34:36] = np.frombuffer(int(dport).to_bytes(2, "big"), np.uint8)
    k[36], k[37], k[38] = 1, tp, 4
    return k.tobytes()
