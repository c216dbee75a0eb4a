"""Flow-affine sharding (gpd_flow_keys / gpd_flow_insert_keys / gpd_flow_key_ids, DESIGN §5b,
§8(e)) on the GPU against the restatement (oracle/flow_ref.py through tests/flow_shard_ref.py):
the three-pass partition alone, W ranks simulated in one process, mixed use of one table, the
test hooks on the key-record path, grid-stride loops of more than one sweep, and the epoch tag
wrapping after 255 inserts."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import flow_shard_ref as R
import golden_cases as G
import oracle_ref as O
from conftest import ROOT
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.batch import PacketBatch
from test_flow import _burst_batch, _decode_dev, _hot_batch

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import flow_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = 0xFFF
BASE = (1 << 40) + 5
NONE, FULL, COLLISION = 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000
PATTERN = 0xA5
MAX_PARTS = 1024


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    return P.NewDecodingLayerParser(L.LayerTypeEthernet, *[P.DECODER_BY_NAME[k]() for k in P.DECODER_BY_NAME])


# ---------------------------------------------------------------- material
@functools.lru_cache(maxsize=None)
def _unkeyed_frames():
    """Golden frames without a network + transport pair (ARP, truncated headers, ...)."""
    batch = PacketBatch.from_packets([G.case_bytes(c) for c in G.load()["cases"]])
    keyed, _ = R.keys_vec(batch, O.decode(batch, L.LayerTypeEthernet, ALL, 0, ext=False))
    frames = [batch.packet(int(i)) for i in np.nonzero(~keyed)[0]]
    assert len(frames) >= 2
    return frames


@functools.lru_cache(maxsize=None)
def _part_source():
    """20,000+ packets: stretches of the mixed batch (every packet its own flow), an unkeyed
    frame, a stretch of bursts (runs of one flow), and so on."""
    mixed, burst, unk = synth.make_mixed(8400), _burst_batch(12000, 200, 7), _unkeyed_frames()
    out, i, j, u = [], 0, 0, 0
    while len(out) < 20040:
        out += [mixed.packet(k) for k in range(i, i + 37)]
        out.append(unk[u % len(unk)])
        out += [burst.packet(k) for k in range(j, j + 53)]
        i, j, u = i + 37, j + 53, u + 1
    return PacketBatch.from_packets(out)


def _with_unkeyed(batch, every):
    """The batch with an unkeyed frame after every `every` packets."""
    unk, out = _unkeyed_frames(), []
    for i in range(batch.n):
        out.append(batch.packet(i))
        if i % every == every - 1:
            out.append(unk[(i // every) % len(unk)])
    return PacketBatch.from_packets(out)


def _decode_checked(parser, batch, records=False):
    """Decode on the device and with the oracle; status and hdr_off must agree, so that a flow
    failure is not a decode failure in disguise.  Returns (db, dr, oracle result, keyed, keys)."""
    import torch
    from gopacket_amd import parser as P
    if records:
        db, dr = P.DeviceBatch(batch, 0), P.DeviceResult(batch.n, 0, records=True)
        parser.decode_device(db, dr)
    else:
        db, dr = _decode_dev(parser, batch)
    torch.cuda.synchronize()
    res = dr.to_host()
    ref = O.decode(batch, L.LayerTypeEthernet, parser.decoders, 0, ext=False, nthreads=8)
    assert np.array_equal(res.status, ref.status) and np.array_equal(res.hdr_off, ref.hdr_off)
    keyed, keys = R.keys_vec(batch, ref)
    return db, dr, ref, keyed, keys


# ---------------------------------------------------------------- the C-ABI calls
def _flow_keys(ft, db, dr, nparts, base, slack=4):
    """gpd_flow_keys into a pattern-filled tensor of n + slack records.  Returns (rc, the uint8
    tensor, the counts)."""
    import torch
    from gopacket_amd import flows as FL
    kt = torch.full(((db.n + slack) * 64,), PATTERN, dtype=torch.uint8, device="cuda")
    counts = (C.c_uint64 * max(nparts, 1))()
    b, r = db.c_batch(), dr.c_result()
    rc = FL.lib.gpd_flow_keys(ft.h, C.byref(b), C.byref(r), nparts, base, C.c_void_p(kt.data_ptr()),
                              counts, ft._stream(None))
    return rc, kt, [int(c) for c in counts]


def _words(kt, m):
    """The first m key records of a uint8 key tensor as int64 [m, 8] (a view)."""
    import torch
    return kt[:m * 64].view(torch.int64).view(m, R.KEY_WORDS)


def _insert_keys(ft, recs):
    """gpd_flow_insert_keys of an int64 [m, 8] tensor.  Returns the ids (int32 tensor [m])."""
    import torch
    from gopacket_amd import flows as FL
    recs = recs.contiguous()
    m = int(recs.shape[0])
    ids = torch.full((m + 8,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    FL.check(FL.lib.gpd_flow_insert_keys(ft.h, C.c_void_p(recs.data_ptr()), m, C.c_void_p(ids.data_ptr()),
                                         ft._stream(None)), "gpd_flow_insert_keys")
    return ids[:m], ids[m:]


def _key_ids(ft, recs, m, ids, base, n, guard=64):
    """gpd_flow_key_ids.  Returns (owner int32[n], flow_id uint32[n]) on the host; the guard
    elements after the n results must stay as they were."""
    import torch
    from gopacket_amd import flows as FL
    owner = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    fid = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    FL.check(FL.lib.gpd_flow_key_ids(ft.h, C.c_void_p(recs.data_ptr()), m, C.c_void_p(ids.data_ptr()), base, n,
                                     C.c_void_p(owner.data_ptr()), C.c_void_p(fid.data_ptr()),
                                     ft._stream(None)), "gpd_flow_key_ids")
    torch.cuda.synchronize()
    o, f = owner.cpu().numpy(), fid.cpu().numpy()
    assert (o[n:] == 0x5A5A5A5A).all() and (f[n:] == 0x5A5A5A5A).all(), "writes past the n results"
    return o[:n], f[:n].view(np.uint32)


def _host16(recs):
    """Key records (int64 [m, 8] tensor) on the host as uint32 [m, 16]."""
    return np.ascontiguousarray(recs.cpu().numpy()).view("<u4").reshape(-1, 16)


def _seq_of(kr16):
    return kr16[:, R.W_SEQ_LO].astype(np.uint64) | (kr16[:, R.W_SEQ_HI].astype(np.uint64) << np.uint64(32))


# ---------------------------------------------------------------- checks by key
def _check_export(recs, g, whole=True):
    """Exported records against the reference rows of their keys.  Returns each record's row."""
    row = R.rows_in(g["keys"], R.rec_keys(recs))
    assert (row >= 0).all(), "a record whose key the reference does not hold"
    assert len(set(row.tolist())) == len(row), "two records with one key"
    if whole:
        assert len(recs) == len(g["keys"]), "one record per distinct key"
    for f in ("first", "last", "packets", "bytes"):
        bad = np.nonzero(recs[f].astype(np.uint64) != g[f][row].astype(np.uint64))[0]
        assert len(bad) == 0, f"{f}: record {bad[0]} holds {recs[f][bad[0]]}, the reference {g[f][row][bad[0]]}"
    assert (recs["first"][1:] >= recs["first"][:-1]).all(), "export ordered by first"
    assert (recs["fp"] != 0).all()
    return row


def _check_ids(fid, label, idx, row):
    """Every item with a key (label >= 0: its row in the reference) carries the index of the
    record that holds its key; every other item GPD_FLOW_NONE.  idx / row: the exported
    records' indices and reference rows."""
    fid = np.asarray(fid).view(np.uint32)
    label = np.asarray(label)
    has = label >= 0
    assert (fid[~has] == NONE).all(), "GPD_FLOW_NONE exactly where no key"
    assert (fid[has] < COLLISION).all(), "a keyed item without a record (none, full or collision)"
    order = np.argsort(idx)
    sidx = idx[order].astype(np.int64)
    pos = np.minimum(np.searchsorted(sidx, fid[has].astype(np.int64)), len(sidx) - 1)
    assert (sidx[pos] == fid[has]).all(), "a flow id that names no exported record"
    assert (row[order][pos] == label[has]).all(), "a flow id that names another key's record"


def _check_stats(ft, flows, packets, no_key):
    st = ft.Stats()
    assert (st["flows"], st["packets"], st["no_key"]) == (flows, packets, no_key), st
    assert st["collisions"] == 0 and st["full"] == 0, st


def _scaled(g, times, last_add):
    """The reference after the same items went in `times` times, the last time `last_add` later."""
    return {**g, "packets": g["packets"] * np.uint64(times), "bytes": g["bytes"] * np.uint64(times),
            "last": g["last"] + np.uint64(last_add)}


# ---------------------------------------------------------------- a. the partition alone
_NS = (1, 63, 64, 65, 255, 256, 257, 1000, 20000)
_PS = (1, 2, 3, 7, 64, 1000, 1024)
_PART_CASES = sorted((n, p) for n in _NS for p in _PS if n in (257, 20000) or p in (3, 1024))


def _check_partition(ft, batch, db, dr, ref, keyed, keys, nparts, base):
    rc, kt, counts = _flow_keys(ft, db, dr, nparts, base)
    assert rc == 0
    n = batch.n
    own = R.owner_ref(ref.net_hash, ref.tp_hash, nparts)
    rows, want = R.expected_partition(keyed, keys, batch.caplen, base + np.arange(n, dtype=np.uint64), own, nparts)
    assert counts == want.tolist(), "part_count per owner"
    m = sum(counts)
    assert m == int(keyed.sum())
    host = kt.cpu().numpy()
    assert (host[m * 64:] == PATTERN).all(), "bytes past the sum(part_count) records were written"
    kr16 = host[:m * 64].view("<u4").reshape(m, 16)
    assert np.array_equal(kr16[:, R.W_OWNER], np.repeat(np.arange(nparts), counts)), \
        "a record's owner is the partition it sits in"
    assert np.array_equal(R.emitted_rows(kr16, counts), rows), "partition p's records are the reference's for owner p"
    fp = kr16[:, R.W_FP_LO].astype(np.uint64) | (kr16[:, R.W_FP_HI].astype(np.uint64) << np.uint64(32))
    assert (fp != 0).all() and (fp < (1 << 56)).all()
    if m:
        uk, inv = np.unique(kr16[:, R.W_KEY], axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        lo, hi = np.full(len(uk), ~np.uint64(0)), np.zeros(len(uk), np.uint64)
        np.minimum.at(lo, inv, fp)
        np.maximum.at(hi, inv, fp)
        assert np.array_equal(lo, hi), "one key, two fingerprints"
        assert len(np.unique(lo)) == len(uk), "two keys of this batch share a 56-bit fingerprint"
    return kt, counts


@pytest.mark.parametrize("n,nparts", _PART_CASES)
def test_partition_matches_reference(parser, n, nparts):
    """gpd_flow_keys at wave (64) and workgroup (256) edges and with 1 to GPD_FLOW_MAX_PARTS
    owners, from the SoA results and from the gpd_record form."""
    from gopacket_amd import flows as FL
    src = _part_source()
    lo = 0 if n == 20000 else 36  # (36: one packet of the mixed stretch, an unkeyed frame, then bursts)
    batch = src.slice(lo, lo + n)
    assert batch.n == n
    ft = FL.NewFlowTable(parser, 64)
    for records in (False, True):
        db, dr, ref, keyed, keys = _decode_checked(parser, batch, records)
        assert n < 63 or 0 < int(keyed.sum()) < n
        _check_partition(ft, batch, db, dr, ref, keyed, keys, nparts, BASE)
    st = ft.Stats()
    assert st["flows"] == 0 and st["packets"] == 0, "gpd_flow_keys leaves the table alone"


# ---------------------------------------------------------------- b. degenerate partitions
@pytest.mark.parametrize("nparts", [7, 1024])
def test_partition_one_flow_one_owner(parser, nparts):
    from gopacket_amd import flows as FL
    one = synth.make_mixed(3).packet(1)
    batch = PacketBatch.from_packets([one] * 700)
    db, dr, ref, keyed, keys = _decode_checked(parser, batch)
    assert keyed.all()
    ft = FL.NewFlowTable(parser, 64)
    _, counts = _check_partition(ft, batch, db, dr, ref, keyed, keys, nparts, BASE)
    assert sorted(counts)[-1] == 700 and sum(counts) == 700


def test_partition_without_keys_and_empty_calls(parser):
    import torch
    from gopacket_amd import flows as FL
    unk = _unkeyed_frames()
    batch = PacketBatch.from_packets([unk[i % len(unk)] for i in range(300)])
    db, dr, ref, keyed, keys = _decode_checked(parser, batch)
    assert not keyed.any()
    ft = FL.NewFlowTable(parser, 64)
    for nparts in (1, 3, 1024):
        _, counts = _check_partition(ft, batch, db, dr, ref, keyed, keys, nparts, BASE)
        assert counts == [0] * nparts
    recs = torch.zeros((1, R.KEY_WORDS), dtype=torch.int64, device="cuda")
    ids, guard = _insert_keys(ft, recs[:0])
    ids1 = torch.zeros(1, dtype=torch.int32, device="cuda")
    owner, fid = _key_ids(ft, recs, 0, ids1, BASE, batch.n)
    assert (owner == -1).all() and (fid == NONE).all()
    assert (guard.cpu().numpy() == -0x5A5A5A5B).all()
    _check_stats(ft, 0, 0, 0)
    assert len(ft.Export()[0]) == 0


def test_partition_of_an_empty_batch(parser):
    """n = 0: every count 0, nothing written; a DeviceBatch / DeviceResult of no packets holds
    null arrays, which an empty call must accept (it reads nothing)."""
    import torch
    from gopacket_amd import flows as FL
    from gopacket_amd import parser as P
    src = _part_source()
    batch = src.slice(5, 5)
    assert batch.n == 0
    db, dr = P.DeviceBatch(batch, 0), P.DeviceResult(0, 0)
    ft = FL.NewFlowTable(parser, 64)
    for nparts in (1, 3, 1024):
        rc, kt, counts = _flow_keys(ft, db, dr, nparts, BASE)
        assert rc == 0 and counts == [0] * nparts
        assert (kt.cpu().numpy() == PATTERN).all()
    fid = ft.Insert(db, dr, index_base=7)
    assert fid.numel() == 0
    st = FL.ShardedFlowTable(parser, 64)
    owner, fid = st.Insert(db, dr, index_base=7)
    torch.cuda.synchronize()
    assert owner.numel() == 0 and fid.numel() == 0
    _check_stats(ft, 0, 0, 0)
    _check_stats(st.table, 0, 0, 0)


@pytest.mark.parametrize("nparts", [0, MAX_PARTS + 1])
def test_partition_refuses_nparts_out_of_range(parser, nparts):
    from gopacket_amd import _lib
    from gopacket_amd import flows as FL
    batch = _part_source().slice(0, 100)
    db, dr = _decode_dev(parser, batch)
    ft = FL.NewFlowTable(parser, 64)
    rc, kt, _ = _flow_keys(ft, db, dr, nparts, BASE)
    assert rc == _lib.GPD_ERR_INVALID
    assert (kt.cpu().numpy() == PATTERN).all()


# ---------------------------------------------------------------- c. W simulated ranks
G0 = (1 << 33) + 11  # sequence number of the whole material's first packet


@functools.lru_cache(maxsize=None)
def _sender_material():
    """Three senders' batches (consecutive thirds of one capture, each with its own index_base)
    and the reference over the whole: flow_ref.group, and the same as arrays (group_vec)."""
    parts = [_hot_batch(4000, 400, 6), _with_unkeyed(synth.make_mixed(3900, seed=0x5EED0200), 39),
             _burst_batch(4000, 100, 8)]
    bases = [G0, G0 + parts[0].n, G0 + parts[0].n + parts[1].n]
    full = R.concat_batches(parts)
    ref = O.decode(full, L.LayerTypeEthernet, ALL, 0, ext=False, nthreads=8)
    keyed, keys = R.keys_vec(full, ref)
    g = R.group_vec(keys, keyed, full.caplen, G0 + np.arange(full.n, dtype=np.uint64))
    flows_ref, _ = F.group(full, ref, index_base=G0)
    assert R.group_as_dict(g) == flows_ref and 0 < int((~keyed).sum())
    for a in (keyed, keys, g["label"], ref.net_hash, ref.tp_hash):
        a.setflags(write=False)
    return parts, bases, ref, keyed, g


def _sender_keys(parser, batch, base, nparts, ft=None):
    """One sender's part of a round: decode (checked), gpd_flow_keys.  Returns a dict."""
    from gopacket_amd import flows as FL
    db, dr, ref, keyed, keys = _decode_checked(parser, batch)
    ft = ft or FL.NewFlowTable(parser, 64)  # (the sender's table: its scratch holds the counts)
    rc, kt, counts = _flow_keys(ft, db, dr, nparts, base)
    assert rc == 0 and sum(counts) == int(keyed.sum())
    return {"ft": ft, "n": batch.n, "base": base, "kt": kt, "counts": counts, "m": sum(counts),
            "recs": _words(kt, sum(counts)), "keyed": keyed, "keys": keys, "ref": ref}


def _exchange_insert_return(snd, tables, order, each):
    """The exchange, the owners' inserts and the ids' way back, for senders `snd` (from
    _sender_keys) and one table per owner.  each: one gpd_flow_insert_keys call per (owner,
    sender) in the order given, not one per owner over the concatenation.  Returns per sender
    (owner, flow_id) host arrays, and per owner (received records, their ids)."""
    import torch
    recv, route = R.sim_exchange([s["recs"] for s in snd], [s["counts"] for s in snd], order)
    ids, held = [], []
    for p, ft in enumerate(tables):
        if each:
            pieces, at = [], 0
            for _, c in route[p]:
                got, guard = _insert_keys(ft, recv[p][at:at + c])
                pieces.append(got)
                held.append(guard)
                at += c
            ids.append(torch.cat(pieces))
        else:
            got, guard = _insert_keys(ft, recv[p])
            ids.append(got)
            held.append(guard)
    torch.cuda.synchronize()
    assert all((h.cpu().numpy() == -0x5A5A5A5B).all() for h in held), "ids written past the records"
    back = R.sim_return(ids, route, [s["counts"] for s in snd])
    out = []
    for s, b in zip(snd, back):
        b = torch.cat([b, b.new_zeros(1)])  # (never an empty allocation)
        out.append(_key_ids(s["ft"], s["recs"] if s["m"] else b, s["m"], b, s["base"], s["n"]))
    return out, list(zip(recv, ids))


def _check_sharded(tables, owner, fid, keyed, label, own_ref, g):
    """What test_sharded_flow_table_two_ranks asserts: each packet's (owner, id) names the record
    holding its key; no key on two tables; the union of the exports is the reference."""
    assert np.array_equal(owner, np.where(keyed, own_ref, -1)), "owner per packet"
    seen = np.zeros(len(g["keys"]), bool)
    for p, ft in enumerate(tables):
        recs, idx = ft.Export()
        row = _check_export(recs, g, whole=False)
        assert not seen[row].any(), "a flow on two tables"
        seen[row] = True
        mine = owner == p
        _check_ids(fid[mine], label[mine], idx, row)
        st = ft.Stats()
        assert st["collisions"] == 0 and st["full"] == 0 and st["no_key"] == 0
        assert st["flows"] == len(recs) and st["packets"] == int(mine.sum())
    assert (fid[~keyed] == NONE).all()
    assert seen.all(), "a flow of the reference on no table"


@pytest.mark.parametrize("each", [False, True], ids=["one_insert", "insert_per_sender"])
@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("W", [1, 2, 3, 7])
def test_sharded_tables_in_one_process(parser, W, order, each):
    """S = 3 senders, W owners, one FlowTable per owner; the exchange is simulated with tensor
    slicing (tests/flow_shard_ref.py).  With the senders' partitions inserted in descending
    order `first` must still fall (key records: no bound on earlier sequence numbers)."""
    from gopacket_amd import flows as FL
    parts, bases, ref, keyed, g = _sender_material()
    snd = [_sender_keys(parser, b, base, W) for b, base in zip(parts, bases)]
    tables = [FL.NewFlowTable(parser, 1 << 14) for _ in range(W)]
    out, _ = _exchange_insert_return(snd, tables, [0, 1, 2] if order == "ascending" else [2, 1, 0], each)
    owner = np.concatenate([o for o, _ in out])
    fid = np.concatenate([f for _, f in out])
    own_ref = R.owner_ref(ref.net_hash, ref.tp_hash, W)
    _check_sharded(tables, owner, fid, keyed, g["label"], own_ref, g)
    if W > 1:
        assert len(set(owner[keyed].tolist())) == W


def test_sharded_flow_table_single_rank_path(parser):
    """ShardedFlowTable without a process group (its `single` path) against a plain
    FlowTable.Insert of the same batches: record for record, by key."""
    import torch
    from gopacket_amd import flows as FL
    parts, bases, ref, keyed, g = _sender_material()
    st, ft = FL.ShardedFlowTable(parser, 1 << 14), FL.NewFlowTable(parser, 1 << 14)
    assert st.single and st.world == 1 and st.rank == 0
    owners, fids, plain = [], [], []
    for b, base in zip(parts, bases):
        db, dr, *_ = _decode_checked(parser, b)
        o, f = st.Insert(db, dr, index_base=base)
        plain.append(ft.Insert(db, dr, index_base=base).cpu().numpy().view(np.uint32))
        owners.append(o.cpu().numpy())
        fids.append(f.cpu().numpy().view(np.uint32))
    torch.cuda.synchronize()
    owner, fid = np.concatenate(owners), np.concatenate(fids)
    _check_sharded([st.table], owner, fid, keyed, g["label"], np.zeros(len(keyed), np.int64), g)
    recs_s, idx_s = st.Export()
    recs_p, idx_p = ft.Export()
    row_s, row_p = _check_export(recs_s, g), _check_export(recs_p, g)
    _check_ids(np.concatenate(plain), g["label"], idx_p, row_p)
    a, b = recs_s[np.argsort(row_s)], recs_p[np.argsort(row_p)]
    for f in ("fp", "src", "dst", "sport", "dport", "net_type", "tp_type", "addr_len", "first", "last",
              "packets", "bytes"):
        assert np.array_equal(a[f], b[f]), f
    assert {k: v for k, v in st.Stats().items() if k != "no_key"} == \
        {k: v for k, v in ft.Stats().items() if k != "no_key"}
    assert ft.Stats()["no_key"] == int((~keyed).sum())


# ---------------------------------------------------------------- d. mixed use of one table
def test_packets_and_key_records_into_one_table(parser):
    """gpd_flow_insert at base 10,000, then key records (W = 1), then gpd_flow_insert at base 0,
    below everything before: once key records went in, the table knows no bound on earlier
    sequence numbers and `first` must still fall.  After Reset the bound is back and exact."""
    import torch
    from gopacket_amd import flows as FL
    a, b, c = (_with_unkeyed(_hot_batch(3000, 300, 21), 50), _burst_batch(2500, 300, 22),
               _with_unkeyed(_hot_batch(2000, 300, 23), 41))
    bases = (10000, 30000, 0)
    ft = FL.NewFlowTable(parser, 1 << 12)
    dec = [_decode_checked(parser, x) for x in (a, b, c)]
    fids = [None] * 3
    fids[0] = ft.Insert(dec[0][0], dec[0][1], index_base=bases[0]).cpu().numpy().view(np.uint32)
    s = _sender_keys(parser, b, bases[1], 1, ft)
    ids, _ = _insert_keys(ft, s["recs"])
    _, fids[1] = _key_ids(ft, s["recs"], s["m"], ids, bases[1], b.n)
    fids[2] = ft.Insert(dec[2][0], dec[2][1], index_base=bases[2]).cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()

    def ref_of(steps):
        keyed = np.concatenate([dec[k][3] for k, _ in steps])
        keys = np.concatenate([dec[k][4] for k, _ in steps])
        cap = np.concatenate([(a, b, c)[k].caplen for k, _ in steps])
        seq = np.concatenate([base + np.arange((a, b, c)[k].n, dtype=np.uint64) for k, base in steps])
        return keyed, R.group_vec(keys, keyed, cap, seq)

    keyed, g = ref_of([(0, bases[0]), (1, bases[1]), (2, bases[2])])
    assert int(g["packets"].max()) > 3 and int((g["first"] < 2000).sum()) > 100
    recs, idx = ft.Export()
    row = _check_export(recs, g)
    _check_ids(np.concatenate(fids), g["label"], idx, row)
    _check_stats(ft, len(g["keys"]), int(keyed.sum()), int((~dec[0][3]).sum() + (~dec[2][3]).sum()))
    ft.Reset()
    assert ft.Stats()["flows"] == 0
    f0 = ft.Insert(dec[0][0], dec[0][1], index_base=0).cpu().numpy().view(np.uint32)
    f2 = ft.Insert(dec[2][0], dec[2][1], index_base=a.n).cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    keyed, g = ref_of([(0, 0), (2, a.n)])
    recs, idx = ft.Export()
    row = _check_export(recs, g)
    _check_ids(np.concatenate([f0, f2]), g["label"], idx, row)
    _check_stats(ft, len(g["keys"]), int(keyed.sum()), int((~keyed).sum()))


# ---------------------------------------------------------------- e. gpd_flow_key_ids bounds
def test_key_ids_ignores_records_outside_the_batch(parser):
    """Key records whose sequence number lies below index_base or at / above index_base + n name
    no packet of the batch: they change nothing, and every other packet still gets its id."""
    import torch
    from gopacket_amd import flows as FL
    n, base = 1000, BASE
    batch = _part_source().slice(100, 100 + n)
    s = _sender_keys(parser, batch, base, 3)
    m = s["m"]
    ids = torch.arange(m, dtype=torch.int32, device="cuda") * 7 + 1
    kr = _host16(s["recs"])
    seq = _seq_of(kr)
    want_owner, want_fid = np.full(n, -1, np.int32), np.full(n, NONE, np.uint32)
    want_owner[(seq - base).astype(np.int64)] = kr[:, R.W_OWNER]
    want_fid[(seq - base).astype(np.int64)] = np.arange(m) * 7 + 1
    assert np.array_equal(want_owner >= 0, s["keyed"])
    owner, fid = _key_ids(s["ft"], s["recs"], m, ids, base, n)
    assert np.array_equal(owner, want_owner) and np.array_equal(fid, want_fid)
    # move some records out of the batch: just below, far below, zero, just above, far above
    out = np.array([base - 1, base - (1 << 20), 0, base + n, base + n + 5, (1 << 63) + 9, (1 << 64) - 1], np.uint64)
    pick = np.random.default_rng(4).choice(m, size=5 * len(out), replace=False)
    moved = seq.copy()
    moved[pick] = np.tile(out, 5)
    kr2 = kr.copy()
    kr2[:, R.W_SEQ_LO] = (moved & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    kr2[:, R.W_SEQ_HI] = (moved >> np.uint64(32)).astype(np.uint32)
    recs2 = torch.from_numpy(kr2.view(np.int64).reshape(m, R.KEY_WORDS)).cuda()
    lost = (seq[pick] - base).astype(np.int64)
    want_owner[lost], want_fid[lost] = -1, NONE
    owner, fid = _key_ids(s["ft"], recs2, m, ids, base, n)
    assert np.array_equal(owner, want_owner) and np.array_equal(fid, want_fid)


# ---------------------------------------------------------------- f. the test hooks
def test_fingerprint_collisions_on_the_key_record_path(parser):
    """Fingerprints cut to 3 bits on two owner tables: a key record whose key differs from its
    record's stored key carries GPD_FLOW_COLLISION, every other does not, the counter counts
    exactly the flagged ones and each record's counters cover every key record on it."""
    from gopacket_amd import flows as FL
    batch = synth.make_mixed(6000, 0x5EED0300)
    W = 2
    s = _sender_keys(parser, batch, BASE, W)
    tables = [FL.NewFlowTable(parser, 1 << 12) for _ in range(W)]
    for ft in tables:
        ft._test_fingerprint_bits(3)
    out, got = _exchange_insert_return([s], tables, [0], False)
    owner, fid = out[0]
    flagged_packets = 0
    for p, (ft, (recv, ids)) in enumerate(zip(tables, got)):
        kr = _host16(recv)
        ids = ids.cpu().numpy().view(np.uint32)
        assert len(kr) == s["counts"][p] > 0 and (kr[:, R.W_OWNER] == p).all()
        rec_of, flagged = ids & 0x7FFFFFFF, (ids & COLLISION) != 0
        recs, idx = ft.Export()
        st = ft.Stats()
        assert st["flows"] == len(recs) <= 8 and st["full"] == 0 and st["packets"] == len(kr)
        stored = {int(ix): k.tobytes() for ix, k in zip(idx, R.rec_keys(recs))}
        mine = kr[:, R.W_KEY].copy().view(np.uint8)
        for j in range(len(kr)):
            assert flagged[j] == (mine[j].tobytes() != stored[int(rec_of[j])])
        assert st["collisions"] == int(flagged.sum()) > 0
        seq = _seq_of(kr)
        for r, ix in zip(recs, idx):
            on = rec_of == ix
            assert int(r["packets"]) == int(on.sum()) > 0
            assert int(r["bytes"]) == int(kr[on, R.W_CAPLEN].astype(np.int64).sum())
            assert (int(r["first"]), int(r["last"])) == (int(seq[on].min()), int(seq[on].max()))
        # the flags reach the packets through gpd_flow_key_ids unchanged
        at = (seq - BASE).astype(np.int64)
        assert np.array_equal(fid[at], ids) and (owner[at] == p).all()
        flagged_packets += int(flagged.sum())
    assert int(((fid != NONE) & ((fid & COLLISION) != 0)).sum()) == flagged_packets


def test_counter_spills_on_the_key_record_path(parser):
    """The packed counter word split at 7 bits: nearly every add of key records carries; the
    same records inserted four times over leave exact counters."""
    from gopacket_amd import flows as FL
    batch = R.concat_batches([_hot_batch(4000, 300, 11), _burst_batch(4000, 200, 12)])
    s = _sender_keys(parser, batch, BASE, 1)
    g = R.group_vec(s["keys"], s["keyed"], batch.caplen, BASE + np.arange(batch.n, dtype=np.uint64))
    ft = FL.NewFlowTable(parser, 1 << 12)
    ft._test_counter_bits(7)
    label = g["label"][(_seq_of(_host16(s["recs"])) - BASE).astype(np.int64)]
    for k in range(1, 5):
        ids, _ = _insert_keys(ft, s["recs"])
        recs, idx = ft.Export()
        row = _check_export(recs, _scaled(g, k, 0))
        _check_ids(ids.cpu().numpy(), label, idx, row)
    assert int(g["packets"].max()) * 4 > 128 and int(g["bytes"].max()) * 4 > (1 << 7)
    _check_stats(ft, len(g["keys"]), 4 * s["m"], 0)


# ---------------------------------------------------------------- g. more than one sweep
@pytest.fixture(scope="module")
def swept(parser):
    """A batch of two sweeps of the capped grid (8 workgroups per CU, 256 packets each) plus 257
    packets: 8,000 packets tiled through offset[] / caplen[] over one copy of their bytes, so
    the same flows recur in later sweeps of one launch.  Decoded once; the reference is the
    oracle's decode of the 8,000, tiled, through keys_vec and group_vec."""
    import torch
    from gopacket_amd import parser as P
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweep = 8 * cus * 256
    n = 2 * sweep + 257
    small = R.concat_batches([synth.make_mixed(5950), PacketBatch.from_packets(_unkeyed_frames() * 25),
                              _burst_batch(2000, 100, 5)])
    nb = small.n
    reps = -(-n // nb)
    big = PacketBatch.from_arrays(small.data, np.tile(small.offset, reps)[:n], np.tile(small.caplen, reps)[:n],
                                  small.data_len)
    assert big.n == n and n > 2 * sweep
    db, dr = P.DeviceBatch(big, 0), P.DeviceResult(n, 0)
    parser.decode_device(db, dr)
    torch.cuda.synchronize()
    res = dr.to_host()
    ref = O.decode(small, L.LayerTypeEthernet, parser.decoders, 0, ext=False, nthreads=8)
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n]
    assert np.array_equal(res.status, tile(ref.status)) and np.array_equal(res.hdr_off, tile(ref.hdr_off))
    keyed, keys = R.keys_vec(small, ref)
    keyed_n, keys_n = tile(keyed), tile(keys)
    g = R.group_vec(keys_n, keyed_n, big.caplen, BASE + np.arange(n, dtype=np.uint64))
    assert 0 < int((~keyed).sum()) and int(g["packets"].min()) >= reps - 1
    return {"n": n, "db": db, "dr": dr, "keyed": keyed_n, "g": g, "reps": reps,
            "net": tile(ref.net_hash), "tp": tile(ref.tp_hash)}


def test_insert_over_several_sweeps(parser, swept):
    """gpd_flow_insert of more than two sweeps into an empty table (records claimed in an
    earlier sweep of the same launch are left to the verify launch), then the same batch at the
    next base (existing flows, updated in the insert, over several sweeps)."""
    import torch
    from gopacket_amd import flows as FL
    n, g, keyed = swept["n"], swept["g"], swept["keyed"]
    ft = FL.NewFlowTable(parser, 1 << 14)
    nk = int(keyed.sum())
    for k in (1, 2):
        fid = ft.Insert(swept["db"], swept["dr"], index_base=BASE + (k - 1) * n)
        torch.cuda.synchronize()
        recs, idx = ft.Export()
        row = _check_export(recs, _scaled(g, k, (k - 1) * n))
        _check_ids(fid.cpu().numpy(), g["label"], idx, row)
        _check_stats(ft, len(g["keys"]), k * nk, k * (n - nk))


@pytest.mark.parametrize("nparts", [1, 3, 1024])
def test_partition_over_several_sweeps(parser, swept, nparts):
    """gpd_flow_keys of more than two sweeps: the LDS counters and the scatter cursors carry over
    the loop iterations.  Per-owner counts and the sorted sequence numbers per owner; at one
    owner the records then go into a table (gpd_flow_insert_keys over several sweeps)."""
    import torch
    from gopacket_amd import flows as FL
    n, g, keyed = swept["n"], swept["g"], swept["keyed"]
    ft = FL.NewFlowTable(parser, 1 << 14)
    rc, kt, counts = _flow_keys(ft, swept["db"], swept["dr"], nparts, BASE)
    assert rc == 0
    own = R.owner_ref(swept["net"], swept["tp"], nparts)
    at = np.nonzero(keyed)[0]
    assert counts == np.bincount(own[at], minlength=nparts).tolist()
    m = sum(counts)
    assert m == len(at)
    recs = _words(kt, m)
    assert (kt[m * 64:].cpu().numpy() == PATTERN).all()
    part = np.repeat(np.arange(nparts), counts)
    assert np.array_equal(recs[:, 5].cpu().numpy() >> 32, part), "owner = the partition a record sits in"
    seq = recs[:, R.SEQ_WORD].cpu().numpy().view(np.uint64)
    got = seq[np.lexsort((seq, part))]
    want = (BASE + at.astype(np.uint64))[np.lexsort((at, own[at]))]
    assert np.array_equal(got, want), "the sorted sequence numbers of every owner"
    if nparts == 1:
        ids, guard = _insert_keys(ft, recs)
        torch.cuda.synchronize()
        assert (guard.cpu().numpy() == -0x5A5A5A5B).all()
        ex, idx = ft.Export()
        row = _check_export(ex, g)
        _check_ids(ids.cpu().numpy(), g["label"][(seq - BASE).astype(np.int64)], idx, row)
        _check_stats(ft, len(g["keys"]), m, 0)
        owner, fid = _key_ids(ft, recs, m, ids, BASE, n)
        assert np.array_equal(owner, np.where(keyed, 0, -1))
        _check_ids(fid, g["label"], idx, row)


# ---------------------------------------------------------------- h. the epoch tag wraps
def _wrap_batch():
    """192 packets over about 40 flows: single packets, short runs, one run across a wave
    boundary, unkeyed frames between."""
    pool = synth.make_mixed(40, 0x5EED0400)
    unk = _unkeyed_frames()
    rng = np.random.default_rng(21)
    out = []
    for f in range(pool.n):
        out += [pool.packet(f)] * int(rng.choice([1, 1, 2, 3]))
        if f % 6 == 2:
            out.append(unk[f % len(unk)])
        if f == 13:
            out += [pool.packet(4)] * 70
    while len(out) < 192:
        out.append(pool.packet(int(rng.integers(0, pool.n))))
    return PacketBatch.from_packets(out[:192])


def test_epoch_tag_wraps_after_255_inserts(parser):
    """300 inserts of one batch into one table, as packets and as key records: at the 256th call
    the records claimed by the first carry the call's own epoch tag and are left to the verify
    launch.  Records, stats and every call's ids are exact; a key keeps its record."""
    import torch
    from gopacket_amd import flows as FL
    calls = 300
    batch = _wrap_batch()
    n = batch.n
    db, dr, ref, keyed, keys = _decode_checked(parser, batch)
    g = R.group_vec(keys, keyed, batch.caplen, np.arange(n, dtype=np.uint64))
    assert 30 <= len(g["keys"]) <= 45 and 0 < int((~keyed).sum()) < n
    want = _scaled(g, calls, (calls - 1) * n)
    nk = int(keyed.sum())
    named = [c - 1 for c in (1, 255, 256, 257, 300)]
    # as packets
    ft = FL.NewFlowTable(parser, 256)
    fids = torch.stack([ft.Insert(db, dr, index_base=c * n) for c in range(calls)]).cpu().numpy().view(np.uint32)
    recs, idx = ft.Export()
    row = _check_export(recs, want)
    for c in named:
        _check_ids(fids[c], g["label"], idx, row)
    assert (fids == fids[0]).all(), "a key keeps its record"
    _check_stats(ft, len(g["keys"]), calls * nk, calls * (n - nk))
    # as key records
    s = _sender_keys(parser, batch, 0, 1)
    label = g["label"][_seq_of(_host16(s["recs"])).astype(np.int64)]
    ft2 = FL.NewFlowTable(parser, 256)
    ids = []
    for c in range(calls):
        kc = s["recs"].clone()
        kc[:, R.SEQ_WORD] += c * n
        ids.append(_insert_keys(ft2, kc)[0])
    ids = torch.stack(ids).cpu().numpy().view(np.uint32)
    recs, idx = ft2.Export()
    row = _check_export(recs, want)
    for c in named:
        _check_ids(ids[c], label, idx, row)
    assert (ids == ids[0]).all(), "a key keeps its record"
    _check_stats(ft2, len(g["keys"]), calls * nk, 0)


# ---------------------------------------------------------------- i. a short export
@pytest.mark.parametrize("max_flows", [1, 10, 299])
def test_export_fewer_records_than_flows(parser, max_flows):
    from gopacket_amd import flows as FL
    batch = _hot_batch(5000, 300, 31)
    db, dr, ref, keyed, keys = _decode_checked(parser, batch)
    g = R.group_vec(keys, keyed, batch.caplen, BASE + np.arange(batch.n, dtype=np.uint64))
    assert len(g["keys"]) >= 300
    ft = FL.NewFlowTable(parser, 1 << 11)
    ft.Insert(db, dr, index_base=BASE)
    recs, idx = ft.Export(max_flows)
    assert len(recs) == len(idx) == max_flows
    _check_export(recs, g, whole=False)  # distinct keys, each the reference's record, sorted by first
    assert len(set(idx.tolist())) == max_flows
