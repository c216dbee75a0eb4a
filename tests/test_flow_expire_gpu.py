"""Flow expiry on the GPU (gpd_flow_remove / gpd_flow_expire / gpd_flow_load,
include/gpd_flow_expire.h): minimal Eth/IPv4/TCP frames through parser and flow table, records
removed and their slots reused, against the model (tests/flow_expire_ref.py).  After every step the
export equals the model key by key, the counts agree, live keys keep their ids and distinct live
keys have distinct ids."""
import json
import os

import numpy as np
import pytest

import flow_expire_ref as ER
import oracle_ref as O
from conftest import ROOT
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.batch import PacketBatch
from tcptrack_cases import ACK, FIN, PSH, SYN, UDP, Packets, frames

pytestmark = pytest.mark.gpu

FULL, NONE = 0xFFFFFFFE, 0xFFFFFFFF
SRV = 0xC0A80001


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    return p


def client(j):
    """Key j as (src, dst, sport, dport): client j to the one server."""
    return (0x0A000000 + j, SRV, 1024 + j % 60000, 80)


def packets(keys, flags=ACK):
    pk = Packets()
    for k in keys:
        pk.add(k[0], k[1], k[2], k[3], flags)
    return pk


def mkey(k):
    return ER.key_of(*k)


class Rig:
    """A flow table beside its model, the packets' sequence numbers counted on.  keys_path: the
    packets go in as key records (gpd_flow_keys, gpd_flow_insert_keys, gpd_flow_key_ids)."""

    def __init__(self, parser, capacity, keys_path=False):
        from gopacket_amd import flows as FL
        self.parser = parser
        self.sharded = FL.ShardedFlowTable(parser, capacity) if keys_path else None
        self.table = self.sharded.table if keys_path else FL.NewFlowTable(parser, capacity)
        self.cap = self.table.Stats()["capacity"]
        self.pool, self.base, self.id_of, self.full = ER.Pool(), 0, {}, 0

    def insert(self, pk, model_hi=None):
        """One batch; the packets from model_hi on are expected to find the table full.  Returns
        the ids (uint32)."""
        from gopacket_amd import parser as P
        batch = pk.batch()
        db, dr = P.DeviceBatch(batch, 0), P.DeviceResult(batch.n, 0)
        self.parser.decode_device(db, dr)
        if self.sharded is not None:
            owner, ids = self.sharded.Insert(db, dr, index_base=self.base)
            assert (owner.cpu().numpy() == 0).all()
        else:
            ids = self.table.Insert(db, dr, index_base=self.base)
        ids = ids.cpu().numpy().view(np.uint32)
        hi = batch.n if model_hi is None else model_hi
        mb = pk.batch(0, hi)
        per = self.pool.insert(mb, O.decode(mb, L.LayerTypeEthernet, 0xFFF, ext=False), self.base)
        for i, k in enumerate(per):
            assert k is not None and ids[i] < self.cap, (i, hex(ids[i]))
            assert self.id_of.setdefault(k, int(ids[i])) == int(ids[i]), "a live key keeps its id"
        assert (ids[hi:] == FULL).all()
        self.full += batch.n - hi
        self.base += batch.n
        self.check()
        return ids

    def check(self):
        """Export, Stats and Load against the model; returns the tombstone count."""
        from gopacket_amd import flowexpire as FE
        recs, idx = self.table.Export()
        assert ER.same_as_export(self.pool, recs)
        assert {ER.flow_ref.record_key(r): int(ix) for r, ix in zip(recs, idx)} == self.id_of
        assert len(set(self.id_of.values())) == len(self.id_of), "distinct live keys, distinct ids"
        st = self.table.Stats()
        assert (st["flows"], st["full"], st["collisions"]) == (len(self.pool), self.full, 0)
        used, tombs = FE.Load(self.table)
        assert used == len(self.pool) and used + tombs <= self.cap
        return tombs

    def hold_mask(self, held):
        import torch
        m = np.zeros(self.cap, np.uint8)
        m[[self.id_of[mkey(k)] for k in held]] = 1
        return torch.from_numpy(m).cuda()

    def expire(self, cutoff, held=(), pairs=False):
        """Expire on the device and in the model: the same keys leave, ids ascending.  Returns
        (the removed ids, the tombstone count)."""
        from gopacket_amd import flowexpire as FE
        ids, n = FE.Expire(self.table, cutoff, self.hold_mask(held) if held else None, pairs)
        got = ids.cpu().numpy().view(np.uint32)
        gone = self.pool.expire(cutoff, [mkey(k) for k in held], pairs)
        assert n == len(gone) == len(got) and list(got) == sorted(self.id_of[k] for k in gone)
        for k in gone:
            del self.id_of[k]
        return got, self.check()

    def remove(self, ids, keys):
        """Remove `ids` on the device, `keys` (their keys) in the model."""
        from gopacket_amd import flowexpire as FE
        FE.Remove(self.table, np.asarray(ids, np.uint32))
        self.pool.remove(mkey(k) for k in keys)
        for k in keys:
            self.id_of.pop(mkey(k), None)
        return self.check()


PATHS = pytest.mark.parametrize("keys_path", [False, True], ids=["packets", "key_records"])


# ---------------------------------------------------------------- 1. chains survive removal
@PATHS
def test_chains_survive_removal(parser, keys_path):
    """256 slots, 192 keys: clusters are certain.  The older half is expired; packets of the rest
    find their records through the tombstones: same ids, no record created."""
    rig = Rig(parser, 256, keys_path)
    old, young = [client(j) for j in range(96)], [client(j) for j in range(96, 192)]
    rig.insert(packets(old))
    ids_young = rig.insert(packets(young))
    displaced = sum(1 for r, ix in zip(*rig.table.Export()) if int(r["fp"]) & 255 != int(ix))
    assert displaced > 20  # keys that sit behind other keys on their chains
    gone, tombs = rig.expire(96)
    assert len(gone) == 96 and 0 < tombs < 96  # some runs end at a record, some were swept
    again = rig.insert(packets(young[::-1] + young))  # (Rig.insert: every key keeps its id)
    assert np.array_equal(again[96:], ids_young) and rig.table.Stats()["flows"] == 96
    gone, tombs2 = rig.expire(96)  # nothing is idle any more
    assert len(gone) == 0 and tombs2 == tombs and len(rig.pool) == 96


# ---------------------------------------------------------------- 2. reuse
@PATHS
def test_reuse_of_a_full_table(parser, keys_path):
    """64 slots, all taken; 32 expire and 32 new keys take their place with no empty slot to end
    a chain on; one key more finds the table full."""
    rig = Rig(parser, 64, keys_path)
    rig.insert(packets([client(j) for j in range(32)]))
    rig.insert(packets([client(j) for j in range(32, 64)]))
    assert len(rig.pool) == 64 and rig.check() == 0
    gone, tombs = rig.expire(32)
    assert len(gone) == 32 and tombs == 32  # no empty slot: nothing to sweep
    rig.insert(packets([client(j) for j in range(100, 132)]))
    assert rig.table.Stats()["full"] == 0 and len(rig.pool) == 64 and rig.check() == 0
    # one more new key, after packets of keys that are there: GPD_FLOW_FULL for it alone
    ids = rig.insert(packets([client(40), client(101), client(999)]), model_hi=2)
    assert ids[2] == FULL and rig.table.Stats()["full"] == 1
    # and everything leaves: the slots equal a reset table's
    gone, tombs = rig.expire(1 << 40)
    assert len(gone) == 64 and tombs == 0 and rig.table.Export()[0].size == 0
    ids = rig.insert(packets([client(j) for j in range(64)]))
    assert sorted(ids) == list(range(64))


# ---------------------------------------------------------------- 3. the race
@PATHS
@pytest.mark.parametrize("bursts", [False, True], ids=["shuffled", "bursts"])
def test_new_keys_race_for_tombstones(parser, keys_path, bursts):
    """A table with tombstones; one batch of 4096 packets carries 64 new keys, each 64 times:
    shuffled across waves and workgroups, or in bursts of neighbouring lanes.  Exactly 64 records
    appear, one id per key, counters exact (Rig.insert checks all of it)."""
    rig = Rig(parser, 256, keys_path)
    rig.insert(packets([client(j) for j in range(96)]))
    rig.insert(packets([client(j) for j in range(96, 192)]))
    gone, tombs = rig.expire(96)
    assert tombs > 0
    rng = np.random.default_rng(5)
    new = [client(1000 + j) for j in range(64)]
    if bursts:
        runs = [j for j in range(64) for _ in range(8)]  # 8 bursts of 8 packets per key
        order = np.repeat(np.array(runs)[rng.permutation(len(runs))], 8)
    else:
        order = rng.permutation(np.repeat(np.arange(64), 64))
    assert len(order) == 4096
    ids = rig.insert(packets([new[int(j)] for j in order]))
    assert len(set(ids.tolist())) == 64 and len(rig.pool) == 96 + 64
    assert all(f["packets"] == 64 for k, f in rig.pool.flows.items() if k in {mkey(x) for x in new})
    assert rig.check() < tombs  # tombstones were claimed


# ---------------------------------------------------------------- 4. the sweep
NCAND = 16384


@pytest.fixture(scope="module")
def homes(parser):
    """The fingerprints of NCAND candidate keys, from a probe insert into a scratch table: a key's
    home slot in a table of 2^k slots is its fingerprint's low k bits."""
    rig = Rig(parser, 1 << 16)
    rig.insert(packets([client(5000 + j) for j in range(NCAND)]))
    recs, _ = rig.table.Export()
    fp = {ER.flow_ref.record_key(r): int(r["fp"]) for r in recs}
    return [fp[mkey(client(5000 + j))] for j in range(NCAND)]


def key_at(homes, slot, mask, used):
    """A candidate key, not used yet, whose home slot is `slot`."""
    for j, fp in enumerate(homes):
        if fp & mask == slot and j not in used:
            used.add(j)
            return client(5000 + j)
    raise AssertionError(f"no candidate for slot {slot}")


@PATHS
def test_sweep_clears_runs_that_end_at_an_empty_slot(parser, homes, keys_path):
    """Keys placed by their home slots: a run of 70 tombstones and one across the table end, both
    ending at an empty slot, vanish; a run that ends at a record stays and is used again."""
    rig, used = Rig(parser, 1024, keys_path), set()
    at = lambda s: key_at(homes, s, 1023, used)
    long_run = list(range(100, 170))                        # 70 slots, then an empty one
    wrap_run = list(range(1015, 1024)) + list(range(0, 6))  # across the table end, then an empty one
    kept_run = list(range(300, 310))                        # ends at the record in slot 310
    idle = [at(s) for s in long_run + wrap_run + kept_run]
    ids = rig.insert(packets(idle))
    assert list(ids) == long_run + wrap_run + kept_run      # every key sits in its home slot
    stay = at(310)
    assert rig.insert(packets([stay]))[0] == 310
    gone, tombs = rig.expire(len(idle))
    assert len(gone) == len(idle) and tombs == len(kept_run)  # both other runs vanished
    # the run that stayed is used again: a new key whose home is inside it takes its home
    k303 = at(303)
    assert rig.insert(packets([k303]))[0] == 303 and rig.check() == 9
    # a new key whose home is the record's slot meets no tombstone on its chain: it goes behind the record
    k310 = at(310)
    assert rig.insert(packets([k310]))[0] == 311
    # with 311 and 310 removed the tombstones 304..311 end at an empty slot and vanish; 300..302 stay behind 303
    assert rig.remove([311, 310], [k310, stay]) == 3
    # expire everything: the table is a reset one, and a fresh insert behaves as on one
    gone, tombs = rig.expire(1 << 40)
    from gopacket_amd import flowexpire as FE
    assert list(gone) == [303] and FE.Load(rig.table) == (0, 0)
    again = rig.insert(packets(idle))
    assert list(again) == long_run + wrap_run + kept_run


# ---------------------------------------------------------------- 5. hold, pairs, the capacity rule
@PATHS
def test_hold_pairs_and_the_capacity_rule(parser, keys_path):
    from gopacket_amd import flowexpire as FE
    A, B, C_, D = 0x0A000001, 0x0A000002, 0x0A000003, 0x0A000004
    c, s = (A, B, 1000, 80), (B, A, 80, 1000)          # client half idle, server half recent
    lone, own = (A, C_, 5, 6), (D, D, 7, 7)            # no reverse; its own reverse
    c2, s2 = (C_, D, 2000, 80), (D, C_, 80, 2000)      # both halves idle
    rig = Rig(parser, 256, keys_path)
    rig.insert(packets([s, c, s, lone, own, own, c2, s2] + [client(j) for j in range(40)]))
    rig.insert(packets([s]))
    cutoff = rig.base - 1
    before = rig.table.Export()
    # the sizing call changes nothing; one id too few removes nothing and says how many
    rc, count = FE.expire_raw(rig.table, cutoff, None, FE.EXPIRE_PAIRS, None, 0)
    assert (rc, count) == (0, 44) and rig.check() == 0
    import torch
    small = torch.full((43,), -1, dtype=torch.int32, device="cuda")
    rc, count = FE.expire_raw(rig.table, cutoff, None, FE.EXPIRE_PAIRS, small, 43)
    assert rc != 0 and count == 44 and (small == -1).all() and rig.check() == 0
    after = rig.table.Export()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # last_below = 0 and a cutoff at the oldest `last` (c's only packet is number 1) remove nothing: strict
    assert len(rig.expire(0)[0]) == 0 and len(rig.expire(1)[0]) == 0 and len(rig.expire(1, pairs=True)[0]) == 0
    # pairs: neither half of the half-idle connection leaves; a held record stays, and holds its peer
    gone, _ = rig.expire(cutoff, held=[s2, client(7)], pairs=True)
    assert len(gone) == 41 and {mkey(c), mkey(s), mkey(c2), mkey(s2), mkey(client(7))} == set(rig.pool.flows)
    assert list(gone) == sorted(gone)
    # without pairs the idle half leaves alone
    gone, _ = rig.expire(cutoff, held=[s2, client(7)])
    assert len(gone) == 2 and set(rig.pool.flows) == {mkey(s), mkey(s2), mkey(client(7))}
    # Remove: duplicates, ids past the capacity, ids of empty slots and of slots already removed
    id7 = rig.id_of[mkey(client(7))]
    empty = next(i for i in range(256) if i not in rig.id_of.values())
    rig.remove([id7, id7, 256, 5000, FULL, NONE, empty, id7], [client(7)])
    rig.remove([id7, empty], [])
    assert set(rig.pool.flows) == {mkey(s), mkey(s2)}
    rig.insert(packets([client(7), c, s]))  # they come back as new records


# ---------------------------------------------------------------- 7. with the consumers
@pytest.mark.parametrize("server_first", [False, True])
def test_tracker_accepts_the_tuple_again_after_expiry(parser, server_first):
    """A connection runs to Established, is expired with pairs and forgotten; the same 4-tuple
    comes again: its SYN is accepted from Closed, whichever side sends it."""
    from gopacket_amd import flowexpire as FE
    from gopacket_amd import parser as P
    from gopacket_amd import tcptrack as M
    from gopacket_amd.flows import NewFlowTable
    table = NewFlowTable(parser, 64)
    tracker = M.NewConnTracker(parser, table)
    c, s = (0x0A000001, 0x0A000002, 1000, 80), (0x0A000002, 0x0A000001, 80, 1000)
    base = 0

    def run(pk):
        nonlocal base
        b = pk.batch()
        db, dr = P.DeviceBatch(b, 0), P.DeviceResult(b.n, 0)
        parser.decode_device(db, dr)
        ids = table.Insert(db, dr, index_base=base)
        base += b.n
        r = tracker.TrackBatch(db, dr, ids, want_conn_id=True)
        return r.verdict.cpu().numpy(), r.conn_id.cpu().numpy().view(np.uint32), ids.cpu().numpy().view(np.uint32)

    hs = Packets()
    hs.add(*c, SYN)
    hs.add(*s, SYN | ACK)
    hs.add(*c, ACK)
    v, conn, ids = run(hs)
    assert (v & 1).all() and (int(v[2]) >> 2) & 7 == M.TCPStateEstablished and list((v >> 1) & 1) == [0, 1, 0]
    assert tracker.states()[conn[0]] & 7 == M.TCPStateEstablished
    # without the expiry the tuple's next SYN meets the old connection: Established, the old directions
    v2, _, _ = run(packets([s if server_first else c], SYN))
    assert v2[0] == (1 | (2 if server_first else 0) | (M.TCPStateEstablished << 2))
    gone, n = FE.Expire(table, base, pairs=True)
    assert n == 2 and sorted(gone.cpu().numpy().view(np.uint32)) == sorted(set(ids.tolist()))
    tracker.forget(gone)
    assert FE.Load(table) == (0, 0) and tracker.states().sum() == 0
    v3, conn3, ids3 = run(packets([s if server_first else c], SYN))
    assert v3[0] == (1 | (M.TCPStateSynSent << 2))  # accepted, client to server, SynSent
    assert conn3[0] == ids3[0]
    tracker.close()


def test_assembler_hold_keeps_a_connection_with_pages(parser):
    """A connection with a buffered out-of-order page is held; it delivers with Skip = 0 when the
    gap fills in a later batch; once closed it expires."""
    from gopacket_amd import flowexpire as FE
    from gopacket_amd import parser as P
    from gopacket_amd import tcpasm as M
    from gopacket_amd import tcpassembly as T
    from gopacket_amd.flows import NewFlowTable
    from tcpseg_cases import A4, B4
    table = NewFlowTable(parser, 64)
    asm = M.NewAssembler(parser, table)
    calls, pool, base = [], {}, 0

    class Fac:
        def New(self, key):
            class St:
                def Reassembled(self, rs):
                    calls.extend(r.as_tuple() for r in rs)

                def ReassemblyComplete(self):
                    calls.append("complete")
            return St()

    def run(fr):
        nonlocal base
        db = P.DeviceBatch(PacketBatch.from_packets(fr), 0)
        d = P.DeviceResult(db.n, 0)
        parser.decode_device(db, d)
        ids = table.Insert(db, d, index_base=base)
        base += db.n
        dsegs, dgroups, count, ngroups, ungrouped = T.TCPSegments(parser, db, d, flow_id=ids, table=table)
        assert ungrouped == 0
        M.deliver(asm.AssembleBatch(db, dsegs, dgroups, count, ngroups), Fac(), pool)
        return ids.cpu().numpy().view(np.uint32)

    tcp = lambda seq, fl, pay=b"": synth.tcp_frame(A4, B4, 5000, 80, seq, ack=1, flags=fl, payload=pay)
    udp = frames([0x0A000009], [SRV], [53], [53], [ACK], [UDP]).packet(0)
    ids = run([tcp(1000, SYN), tcp(1001, PSH | ACK, b"a" * 10), tcp(1021, PSH | ACK, b"c" * 10), udp])
    cid = int(ids[0])
    got = lambda: [x for x in calls if x != "complete"]
    assert asm.conns()[cid]["pages"] == 1 and b"".join(r[0] for r in got()) == b"a" * 10 and got()[0][2]
    assert "complete" not in calls
    hold = FE.assembler_hold(asm)
    assert hold.element_size() == 1 and hold.numel() == 64 and hold.is_cuda
    assert hold.cpu().numpy().nonzero()[0].tolist() == [cid]
    gone, n = FE.Expire(table, base, hold=hold)          # everything is idle; the held record stays
    assert n == 1 and int(gone[0]) == int(ids[3]) and FE.Load(table)[0] == 1
    ids2 = run([tcp(1011, PSH | ACK, b"b" * 10), tcp(1031, FIN | ACK)])
    assert (ids2 == cid).all()                           # the record kept its id
    assert b"".join(r[0] for r in got()) == b"a" * 10 + b"b" * 10 + b"c" * 10  # the page came out behind the gap's bytes
    assert all(r[1] == 0 for r in got()) and [r[2] for r in got()] == [True] + [False] * (len(got()) - 1)
    assert got()[-1][3] and calls[-1] == "complete" and calls.count("complete") == 1
    hold = FE.assembler_hold(asm)
    assert hold.sum().item() == 0 and asm.stats()["connections"] == 0
    gone, n = FE.Expire(table, base, hold=hold)
    assert n == 1 and int(gone[0]) == cid and FE.Load(table) == (0, 0)
    asm.close()


# ---------------------------------------------------------------- 8. a table never removed from
def golden_batch():
    """2,000 packets of 200 keys in bursts, with frames that have no key between them."""
    rng = np.random.default_rng(0xF10E)
    pk = Packets()
    while len(pk) < 2000:
        j = int(rng.integers(200))
        for _ in range(int(rng.integers(1, 12))):
            pk.add(*client(j), ACK, UDP if j % 7 == 0 else 0)
        if rng.random() < 0.2:
            pk.add(*client(j), ACK, 2)  # cut inside the IPv4 header: no key
    return pk


def test_a_table_never_removed_from_equals_the_parent(parser):
    """The ids, stats and export of one batch, recorded before records could leave the table
    (tests/golden/flow_expire_parent.json): the insert of a table without tombstones is the same
    code.  The batch's keys have distinct home slots, so the ids do not depend on timing."""
    from gopacket_amd import parser as P
    from gopacket_amd.flows import NewFlowTable
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "flow_expire_parent.json")))
    b = golden_batch().batch(0, 2000)
    table = NewFlowTable(parser, 1 << 16)
    db, dr = P.DeviceBatch(b, 0), P.DeviceResult(b.n, 0)
    parser.decode_device(db, dr)
    ids = table.Insert(db, dr, index_base=77).cpu().numpy().view(np.uint32)
    recs, idx = table.Export()
    assert ids.tolist() == want["ids"] and table.Stats() == want["stats"]
    assert recs.tobytes().hex() == want["export_hex"] and idx.tolist() == want["export_index"]
    assert (ids == NONE).sum() > 20 and len(recs) > 100
