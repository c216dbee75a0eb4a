"""The helpers of the flow-sharding tests (tests/flow_shard_ref.py) against what they restate:
oracle/flow_ref.py, the owner rule of include/gpd_flow.h and the all-to-all of key records.
CPU only; the GPU cases that use them are in tests/test_flow_shard_gpu.py."""
import os
import sys

import numpy as np
import pytest

import flow_shard_ref as R
import oracle_ref as O
from conftest import ROOT
from gopacket_amd import layers as L
from gopacket_amd import synth
from test_flow import _burst_batch

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import flow_ref as F  # noqa: E402

ALL = 0xFFF


def _batch(kind):
    if kind == "mixed":
        return synth.make_mixed(3000)
    if kind == "golden_mut":
        return R.golden_mut_batch()
    return _burst_batch(3000)


@pytest.mark.parametrize("kind", ["mixed", "golden_mut", "burst"])
def test_keys_vec_and_group_vec_match_flow_ref(kind):
    batch = _batch(kind)
    res = O.decode(batch, L.LayerTypeEthernet, ALL, 0, ext=False)
    keyed_ref, keys_ref = F.flow_keys(batch, res)
    keyed, keys = R.keys_vec(batch, res)
    assert np.array_equal(keyed, keyed_ref) and np.array_equal(keys, keys_ref)
    assert 0 < int(keyed.sum()) and (kind != "golden_mut" or int(keyed.sum()) < batch.n)
    base = (1 << 40) + 5
    flows_ref, per_ref = F.group(batch, res, index_base=base)
    g = R.group_vec(keys, keyed, batch.caplen, base + np.arange(batch.n, dtype=np.uint64))
    assert R.group_as_dict(g) == flows_ref
    assert len(np.unique(g["keys"], axis=0)) == len(g["keys"]) == len(flows_ref)
    for i, k in enumerate(per_ref):
        assert (g["label"][i] == -1) if k is None else (g["keys"][g["label"][i]].tobytes() == k)


def test_group_vec_without_keys():
    g = R.group_vec(np.zeros((5, 40), np.uint8), np.zeros(5, bool), np.ones(5, np.uint32), np.arange(5))
    assert len(g["keys"]) == 0 and (g["label"] == -1).all() and R.group_as_dict(g) == {}


@pytest.mark.parametrize("nparts", [1, 2, 3, 7, 64, 1000, 1024])
def test_owner_ref_matches_flow_owner(nparts):
    from gopacket_amd import flows as FL
    batch = synth.make_mixed(3000)
    res = O.decode(batch, L.LayerTypeEthernet, ALL, 0, ext=False)
    own = R.owner_ref(res.net_hash, res.tp_hash, nparts)
    assert own.tolist() == R.owner_ref_ints(res.net_hash, res.tp_hash, nparts)
    assert np.array_equal(own, FL.flow_owner(res.net_hash, res.tp_hash, nparts).astype(np.int64))
    assert own.min() >= 0 and own.max() < nparts
    keyed, _ = R.keys_vec(batch, res)
    hit = len(set(own[keyed].tolist()))
    if nparts == 1:
        assert hit == 1
    if nparts == 1024:
        assert hit > 1, f"nparts = 1024: the mixed batch's keyed packets hit {hit} distinct owners"
        # the rule reads the high half of the hash: the low half gives other owners
        x = res.net_hash ^ res.tp_hash
        low = ((x & np.uint64(0xFFFFFFFF)) * np.uint64(nparts)) >> np.uint64(32)
        assert (low.astype(np.int64) != own)[keyed].any()


def test_owner_ref_extremes():
    top = np.array([0xFFFFFFFFFFFFFFFF, 0, 0x00000000FFFFFFFF, 0x8000000000000000], np.uint64)
    zero = np.zeros(4, np.uint64)
    assert R.owner_ref(top, zero, 1024).tolist() == [1023, 0, 0, 512]
    assert R.owner_ref(top, top, 7).tolist() == [0, 0, 0, 0]
    assert R.owner_ref(top, zero, 3).tolist() == R.owner_ref_ints(top, zero, 3) == [2, 0, 0, 1]


def test_expected_partition_counts_and_rows():
    batch = _burst_batch(700, 60, 2)
    res = O.decode(batch, L.LayerTypeEthernet, ALL, 0, ext=False)
    keyed, keys = R.keys_vec(batch, res)
    seq = 1000 + np.arange(batch.n, dtype=np.uint64)
    own = R.owner_ref(res.net_hash, res.tp_hash, 7)
    rows, counts = R.expected_partition(keyed, keys, batch.caplen, seq, own, 7)
    assert int(counts.sum()) == int(keyed.sum()) == len(rows)
    assert counts.tolist() == [int(((own == p) & keyed).sum()) for p in range(7)]
    assert np.array_equal(rows[:, 0], np.repeat(np.arange(7), counts)) and np.array_equal(rows[:, 0], rows[:, 12])
    # the emitted form of the same records, shuffled inside each partition, is the same multiset
    rng = np.random.default_rng(1)
    kr = np.zeros((len(rows), 16), np.uint32)
    kr[:, 0:14] = rows[:, 1:15]
    at = 0
    for c in counts:
        kr[at:at + c] = kr[at:at + c][rng.permutation(int(c))]
        at += int(c)
    assert np.array_equal(R.emitted_rows(kr, counts), rows)
    kr[3, R.W_CAPLEN] ^= 1
    assert not np.array_equal(R.emitted_rows(kr, counts), rows)


@pytest.mark.parametrize("order", [None, [2, 1, 0, 3], [3, 0, 2, 1]])
def test_simulated_exchange_round_trips(order):
    """Every record carries (sender, position at the sender); the owners' ids encode (owner,
    position at the owner); ids returned through the exchange land on the records they were
    assigned for.  Random counts, zero-count partitions and an idle sender included."""
    import torch
    rng = np.random.default_rng(11)
    S, W = 4, 5
    counts = rng.integers(0, 40, size=(S, W))
    counts[rng.random((S, W)) < 0.3] = 0
    counts[1, :] = 0      # a sender with nothing to send
    counts[:, 2] = 0      # an owner that receives nothing
    keys = []
    for s in range(S):
        m = int(counts[s].sum())
        k = torch.zeros((m + 3, R.KEY_WORDS), dtype=torch.int64)  # (slack past the records, as in->n gives)
        k[:m, 0] = s
        k[:m, 1] = torch.arange(m)
        k[:m, 2] = torch.from_numpy(np.repeat(np.arange(W), counts[s]))
        k[m:] = -1
        keys.append(k)
    recv, route = R.sim_exchange(keys, counts, order)
    assert len(recv) == W
    ids = []
    for p in range(W):
        assert recv[p].shape == (int(counts[:, p].sum()), R.KEY_WORDS)
        assert (recv[p][:, 2] == p).all(), "only partition p's records reach owner p"
        snd = recv[p][:, 0].tolist()
        want = [s for s in (order or range(S)) for _ in range(int(counts[s, p]))]
        assert snd == want, "senders concatenated in the chosen order"
        ids.append((p << 20) + torch.arange(recv[p].shape[0]))
    back = R.sim_return(ids, route, counts)
    for s in range(S):
        m = int(counts[s].sum())
        assert back[s].shape == (m,)
        for j in range(m):
            p, at = int(back[s][j]) >> 20, int(back[s][j]) & 0xFFFFF
            assert p == int(keys[s][j, 2])
            assert recv[p][at, 0] == s and recv[p][at, 1] == j, "the id names the record it was assigned for"
