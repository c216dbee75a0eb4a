"""TEST INFRASTRUCTURE: reference and harness helpers for the flow-sharding tests
(tests/test_flow_shard.py on the CPU, tests/test_flow_shard_gpu.py on the GPU).

The reference of record is oracle/flow_ref.py; what is here restates it without per-packet
Python loops (the multi-sweep cases hold about a million packets), adds the owner rule of
include/gpd_flow.h, and simulates the all-to-all of key records in one process with tensor
slicing.  Nothing here imports gopacket_amd.flows: that module is code under test.
"""
from __future__ import annotations

import numpy as np

KEY_BYTES = 40   # flow_ref.flow_keys' layout: src[16], dst[16], ports[4], net type, tp type, addr len, 0
KEY_WORDS = 8    # a 64-byte gpd_flow_key as int64 words; word 6 is `seq`, word 7 `fp`
SEQ_WORD = 6
# The 64-byte key record read as sixteen uint32 words.
W_KEY, W_CAPLEN, W_OWNER, W_SEQ_LO, W_SEQ_HI, W_FP_LO, W_FP_HI = slice(0, 10), 10, 11, 12, 13, 14, 15


def owner_ref(net_hash, tp_hash, nparts: int) -> np.ndarray:
    """owner = ((net ^ tp) >> 32) * nparts >> 32 (include/gpd_flow.h), from the oracle's hashes.
    The high half is below 2^32 and nparts at most 1024, so the product fits uint64 exactly."""
    x = np.bitwise_xor(np.asarray(net_hash).astype(np.uint64), np.asarray(tp_hash).astype(np.uint64))
    hi = x // np.uint64(1 << 32)
    return ((hi * np.uint64(int(nparts))) // np.uint64(1 << 32)).astype(np.int64)


def owner_ref_ints(net_hash, tp_hash, nparts: int) -> list:
    """The same rule in Python ints (unbounded), one packet at a time: pins owner_ref."""
    return [(((int(a) ^ int(b)) >> 32) * int(nparts)) >> 32 for a, b in zip(net_hash, tp_hash)]


def keys_vec(batch, res):
    """flow_ref.flow_keys without the per-packet loop: (keyed mask, key bytes u8[n, 40])."""
    n = batch.n
    st = res.status.astype(np.uint32)
    ho = res.hdr_off.astype(np.uint32)
    nt = ((st >> 20) & 15).astype(np.int64)
    tt = ((st >> 24) & 15).astype(np.int64)
    no = (ho & 0xFFFF).astype(np.int64)
    to = (ho >> 16).astype(np.int64)
    keyed = (nt != 0) & (tt != 0) & (no != 0xFFFF) & (to != 0xFFFF)
    keys = np.zeros((n, KEY_BYTES), np.uint8)
    idx = np.nonzero(keyed)[0]
    if len(idx) == 0:
        return keyed, keys
    data = batch.data
    off = batch.offset[idx].astype(np.int64)
    v4 = nt[idx] == 1
    alen = np.where(v4, 4, 16)
    s0 = off + no[idx] + np.where(v4, 12, 8)
    col = np.arange(16, dtype=np.int64)
    used = col[None, :] < alen[:, None]
    top = data.shape[0] - 1  # (masked columns may point past the buffer: clamp, then zero)
    src = data[np.minimum(s0[:, None] + col, top)]
    dst = data[np.minimum((s0 + alen)[:, None] + col, top)]
    sub = np.zeros((len(idx), KEY_BYTES), np.uint8)
    sub[:, 0:16] = np.where(used, src, 0)
    sub[:, 16:32] = np.where(used, dst, 0)
    sub[:, 32:36] = data[(off + to[idx])[:, None] + col[None, :4]]
    sub[:, 36] = nt[idx]
    sub[:, 37] = tt[idx]
    sub[:, 38] = alen
    keys[idx] = sub
    return keyed, keys


def group_vec(keys, keyed, caplen, seq):
    """flow_ref.group without the per-packet loop.  `seq` is each packet's sequence number.
    Returns a dict: `keys` u8[m, 40] (the distinct keys, sorted), `first`, `last`, `packets`,
    `bytes` (int64/uint64[m]) and `label` int64[n]: each packet's row in `keys`, -1 unkeyed."""
    keyed = np.asarray(keyed, bool)
    seq = np.asarray(seq).astype(np.uint64)
    idx = np.nonzero(keyed)[0]
    label = np.full(len(keyed), -1, np.int64)
    if len(idx) == 0:
        z = np.zeros(0, np.uint64)
        return {"keys": np.zeros((0, KEY_BYTES), np.uint8), "first": z, "last": z.copy(),
                "packets": z.copy(), "bytes": z.copy(), "label": label}
    # np.unique(axis=0) sorts 40-byte rows by comparison (8 s for a million packets), so the
    # packets are first labelled exactly by refining over the key's five 64-bit words (1-D
    # sorts), and the row-wise unique runs over one packet per label.
    sub = np.ascontiguousarray(keys[idx])
    words = sub.view("<u8").reshape(len(idx), KEY_BYTES // 8)
    lab = np.zeros(len(idx), np.int64)
    for c in range(words.shape[1]):
        cu, ci = np.unique(words[:, c], return_inverse=True)
        _, rep, lab = np.unique(lab * len(cu) + np.asarray(ci).reshape(-1), return_index=True,
                                return_inverse=True)
        lab = np.asarray(lab).reshape(-1).astype(np.int64)
    uk, inv = np.unique(sub[rep], axis=0, return_inverse=True)
    assert len(uk) == len(rep)
    inv = np.asarray(inv).reshape(-1).astype(np.int64)[lab]
    m = len(uk)
    first = np.full(m, np.iinfo(np.uint64).max, np.uint64)
    last = np.zeros(m, np.uint64)
    np.minimum.at(first, inv, seq[idx])
    np.maximum.at(last, inv, seq[idx])
    packets = np.bincount(inv, minlength=m).astype(np.uint64)
    # (float64 weights: exact while a flow's bytes stay below 2^53)
    nbytes = np.bincount(inv, weights=np.asarray(caplen)[idx].astype(np.float64), minlength=m).astype(np.uint64)
    label[idx] = inv
    return {"keys": uk, "first": first, "last": last, "packets": packets, "bytes": nbytes, "label": label}


def group_as_dict(g) -> dict:
    """group_vec's result in flow_ref.group's form: key bytes -> {first, last, packets, bytes}."""
    return {g["keys"][j].tobytes(): {"first": int(g["first"][j]), "last": int(g["last"][j]),
                                     "packets": int(g["packets"][j]), "bytes": int(g["bytes"][j])}
            for j in range(len(g["keys"]))}


def record_rows(part, key_words, caplen, owner, seq) -> np.ndarray:
    """Key records as uint32 rows [m, 15]: the partition a record sits in, then its key words,
    caplen, owner and seq (low, high) — sorted, so that two multisets compare with array_equal."""
    seq = np.asarray(seq).astype(np.uint64)
    m = len(seq)
    rows = np.zeros((m, 15), np.uint32)
    rows[:, 0] = part
    rows[:, 1:11] = key_words
    rows[:, 11] = caplen
    rows[:, 12] = owner
    rows[:, 13] = (seq & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rows[:, 14] = (seq >> np.uint64(32)).astype(np.uint32)
    order = np.lexsort(tuple(rows[:, c] for c in range(14, -1, -1)))
    return rows[order]


def expected_partition(keyed, keys, caplen, seq, owner, nparts: int):
    """What gpd_flow_keys must emit: (sorted record rows of every partition, see record_rows;
    the records per owner, int64[nparts]).  Rows [sum(counts[:p]), sum(counts[:p + 1])) are
    partition p's multiset of (key[40], caplen, owner, seq)."""
    idx = np.nonzero(np.asarray(keyed, bool))[0]
    own = np.asarray(owner)[idx].astype(np.int64)
    assert len(idx) == 0 or (own.min() >= 0 and own.max() < nparts)
    counts = np.bincount(own, minlength=nparts).astype(np.int64)
    kw = np.ascontiguousarray(keys[idx]).view("<u4").reshape(len(idx), 10)
    rows = record_rows(own, kw, np.asarray(caplen)[idx], own, np.asarray(seq)[idx])
    return rows, counts


def emitted_rows(kr16: np.ndarray, counts) -> np.ndarray:
    """The records gpd_flow_keys wrote (uint32[m, 16] words of the 64-byte records, in the
    order written) as record_rows, the partition taken from where each record sits."""
    part = np.repeat(np.arange(len(counts), dtype=np.int64), np.asarray(counts, np.int64))
    seq = kr16[:, W_SEQ_LO].astype(np.uint64) | (kr16[:, W_SEQ_HI].astype(np.uint64) << np.uint64(32))
    return record_rows(part, kr16[:, W_KEY], kr16[:, W_CAPLEN], kr16[:, W_OWNER], seq)


# ---------------------------------------------------------------- test material
def golden_mut_batch(per_case: int = 200, seed: int = 5):
    """The golden packets and `per_case` two-byte mutations of each (the `golden_mut` recipe of
    tests/test_flow.py): decode errors, truncated headers and keys read near a packet's end."""
    import golden_cases as G
    from gopacket_amd.batch import PacketBatch
    pk = [G.case_bytes(c) for c in G.load()["cases"]]
    rng = np.random.default_rng(seed)
    for p in list(pk):
        for _ in range(per_case):
            a = np.frombuffer(p[:512], np.uint8).copy()
            pos = rng.integers(0, min(len(a), 80), size=2)
            a[pos] = rng.integers(0, 256, size=2, dtype=np.uint8)
            pk.append(a.tobytes())
    return PacketBatch.from_packets(pk)


def concat_batches(batches):
    """Several PacketBatches as one (packet order kept; 16-byte aligned starts)."""
    from gopacket_amd.batch import PacketBatch
    return PacketBatch.from_packets([b.packet(i) for b in batches for i in range(b.n)])


# ---------------------------------------------------------------- the simulated exchange
def sim_exchange(keys_by_sender, counts_by_sender, order=None):
    """What flows.exchange_keys does over a process group, in one process.  keys_by_sender[s] is
    sender s's key records [m_s, ...] grouped by owner, counts_by_sender[s][p] its records for
    owner p.  Returns (recv, route): recv[p] is the concatenation of every sender's partition p
    in the sender order `order` (default ascending); route[p] lists (sender, records) in that
    order, for sim_return."""
    import torch
    senders = list(range(len(keys_by_sender)))
    order = senders if order is None else list(order)
    assert sorted(order) == senders
    nparts = len(counts_by_sender[0])
    starts = []
    for s in senders:
        c = [int(x) for x in counts_by_sender[s]]
        assert len(c) == nparts and sum(c) <= keys_by_sender[s].shape[0]
        starts.append(np.concatenate([[0], np.cumsum(c)]).astype(np.int64))
    recv, route = [], []
    for p in range(nparts):
        pieces = [keys_by_sender[s][int(starts[s][p]):int(starts[s][p + 1])] for s in order]
        recv.append(torch.cat(pieces, dim=0))
        route.append([(s, int(starts[s][p + 1] - starts[s][p])) for s in order])
    return recv, route


def sim_return(ids_by_owner, route, counts_by_sender):
    """What flows.return_ids does: ids_by_owner[p][j] is owner p's id for recv[p][j]; returns per
    sender the ids of its records in the order it sent them (grouped by owner, as its keys)."""
    import torch
    nsend, nparts = len(counts_by_sender), len(route)
    pieces = [[None] * nparts for _ in range(nsend)]
    for p in range(nparts):
        at = 0
        for s, c in route[p]:
            pieces[s][p] = ids_by_owner[p][at:at + c]
            at += c
        assert at <= ids_by_owner[p].shape[0]
    return [torch.cat(pieces[s], dim=0) for s in range(nsend)]


# ---------------------------------------------------------------- exported records, by key
def rec_keys(recs) -> np.ndarray:
    """Key bytes u8[m, 40] of exported gpd_flow_rec records, in flow_ref.record_key's layout."""
    k = np.zeros((len(recs), KEY_BYTES), np.uint8)
    k[:, 0:16] = recs["src"]
    k[:, 16:32] = recs["dst"]
    k[:, 32:34] = recs["sport"]
    k[:, 34:36] = recs["dport"]
    k[:, 36] = recs["net_type"]
    k[:, 37] = recs["tp_type"]
    k[:, 38] = recs["addr_len"]
    return k


def rows_in(ref_keys: np.ndarray, keys: np.ndarray) -> np.ndarray:
    """For each row of `keys` (u8[m, 40]) its row in `ref_keys` (distinct rows), -1 if absent.
    One dictionary lookup per row: meant for records (thousands), not packets."""
    at = {ref_keys[j].tobytes(): j for j in range(len(ref_keys))}
    return np.array([at.get(keys[j].tobytes(), -1) for j in range(len(keys))], np.int64)
