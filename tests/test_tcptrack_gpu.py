"""TCP connection tracking on the GPU (gpd_tcp_tracker_run, include/gpd_tcptrack.h): real
Eth/IPv4/TCP frames through parser, flow table and tracker; verdicts, connection ids, counts and
carried states compared with the model (tests/tcptrack_ref.py) byte for byte."""
import numpy as np
import pytest

import tcptrack_ref as TR
from gopacket_amd import layers as L
from tcptrack_cases import (ACK, CUT, FIN, LIFE, RST, SYN, UDP, Packets, endpoints, gen_connections, interleaved,
                            size_case)
from test_tcptrack import VEC, vector_accepts, vector_packets

pytestmark = pytest.mark.gpu

FULL, COLLISION, NONE = 0xFFFFFFFE, 0x80000000, 0xFFFFFFFF


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    return p


class Pipe:
    """Parser -> flow table -> tracker, with the packets' sequence numbers counted on."""

    def __init__(self, parser, capacity, sme=False, fingerprint_bits=None):
        from gopacket_amd import tcptrack as M
        from gopacket_amd.flows import NewFlowTable
        self.parser = parser
        self.table = NewFlowTable(parser, capacity)
        if fingerprint_bits:
            self.table._test_fingerprint_bits(fingerprint_bits)
        self.tracker = M.NewConnTracker(parser, self.table, support_missing_establishment=sme)
        self.base = 0

    def run(self, batch, records=False):
        """(verdict u8[n], conn u32[n], counts, flow ids u32[n], the TrackResult, the DeviceBatch)."""
        from gopacket_amd import parser as P
        db = P.DeviceBatch(batch, 0)
        dr = P.DeviceResult(batch.n, 0, records=records)
        self.parser.decode_device(db, dr)
        ids = self.table.Insert(db, dr, index_base=self.base)
        self.base += batch.n
        r = self.tracker.TrackBatch(db, dr, ids, want_conn_id=True)
        return (r.verdict.cpu().numpy(), r.conn_id.cpu().numpy().view(np.uint32),
                (r.tracked, r.accepted, r.rejected, r.connections), ids.cpu().numpy().view(np.uint32), r, db)

    def close(self):
        self.tracker.close()


def check(pipe, model, pk, lo=0, hi=None, records=False):
    """One batch pk[lo:hi] through the device and the model: everything equal.  Packets whose flow
    id is no record are untracked for the model, too.  Returns the verdicts."""
    hi = len(pk) if hi is None else hi
    v, c, counts, fid, _, _ = pipe.run(pk.batch(lo, hi), records=records)
    keys = [k if f < pipe.tracker.id_bound else None for k, f in zip(pk.keys(lo, hi), fid)]
    wv, wc, wcounts = model.track(keys, pk.flags[lo:hi], fid)
    bad = np.nonzero(v != wv)[0]
    assert len(bad) == 0, (len(bad), bad[:8], v[bad[:8]], wv[bad[:8]])
    assert np.array_equal(c, wc) and counts == wcounts
    return v


# ---------------------------------------------------------------- 1. the reference's tests as frames
def test_golden_sequences_as_frames(parser):
    """Every golden sequence on a connection of its own, interleaved step by step in one batch per
    option value: the accept bits are the ones the reference's tests assert."""
    for sme in (False, True):
        seqs = [s for s in VEC["sequences"] if s["support_missing_establishment"] == sme]
        pk, owner = Packets(), []
        for step in range(max(len(s["steps"]) for s in seqs)):
            for j, s in enumerate(seqs):
                if step < len(s["steps"]):
                    (a, b, sp, dp), fl = [x[step] for x in vector_packets(s)]
                    ca, sa = 0x0A000001 + j, 0x0B000001
                    pk.add(ca if a == "a" else sa, sa if a == "a" else ca, sp, dp, fl)
                    owner.append(j)
        pipe, model = Pipe(parser, 256, sme), TR.Model(sme)
        v = check(pipe, model, pk)
        for j, s in enumerate(seqs):
            mine = [bool(v[i] & 1) for i in range(len(pk)) if owner[i] == j]
            assert mine == vector_accepts(s), s["test"]
        assert np.array_equal(pipe.tracker.states(), model.states(256))
        pipe.close()


# ---------------------------------------------------------------- 2. random connections, cut into batches
@pytest.fixture(scope="module")
def randcase():
    pk = interleaved(gen_connections(0x7C01, 300), 0x7C02, noise=0.1)
    assert 4000 < len(pk) < 9000 and pk.kind.count(UDP) > 100 and pk.kind.count(CUT) > 100
    return pk


@pytest.mark.parametrize("sme", [False, True])
def test_random_connections_whole_and_cut(parser, randcase, sme):
    pk, n = randcase, len(randcase)
    got = []
    for cuts in ([0, n], [0, n // 2 + 3, n], [0, n // 3, (2 * n) // 3 + 1, n]):
        pipe, model = Pipe(parser, 2048, sme), TR.Model(sme)
        v = np.concatenate([check(pipe, model, pk, a, b, records=(len(cuts) == 3))
                            for a, b in zip(cuts, cuts[1:])])
        assert np.array_equal(pipe.tracker.states(), model.states(2048))
        got.append(v)
        pipe.close()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])  # the carry, the fixed direction
    t = got[0][got[0] != 0xFF]
    assert set((t >> 2) & 7) == set(range(6)) and set(t & 1) == {0, 1} and set((t >> 1) & 1) == {0, 1}
    assert set((t >> 5) & 1) == {0, 1} and (got[0] == 0xFF).sum() == randcase.kind.count(UDP) + randcase.kind.count(CUT)


# ---------------------------------------------------------------- 3. tile boundaries
def long_script(n):
    """n packets of one connection: lives of LIFE, every 23rd packet a stray SYN+FIN that derails
    the life it falls into."""
    out = []
    for k in range(n):
        fl, srv = LIFE[k % len(LIFE)]
        if k % 23 == 22:
            fl = SYN | FIN
        out.append((fl, srv))
    return out


NBIG, NPAD = 64, 8192  # candidates for the long connections and for the one-packet connections


@pytest.fixture(scope="module")
def probe_ids(parser):
    """The flow records of the candidate keys in a fresh table of 2^16 slots."""
    from gopacket_amd import parser as P
    from gopacket_amd.flows import NewFlowTable
    cand = Packets()
    for j in range(NBIG + NPAD):
        c, s = endpoints(j)
        cand.add(c[0], s[0], c[1], s[1], SYN)
    b = cand.batch()
    db, dr = P.DeviceBatch(b, 0), P.DeviceResult(b.n, 0)
    parser.decode_device(db, dr)
    ids = NewFlowTable(parser, 1 << 16).Insert(db, dr).cpu().numpy().view(np.uint32).astype(np.int64)
    assert (ids < (1 << 16)).all()
    return ids


def place(ids, nbig, npad_before):
    """The tracker orders packets by connection id, a flow record index the test cannot choose.
    A probe insert of candidate keys into a table of the same capacity tells their records: the
    first long connection is the candidate whose record lies nearest three quarters of the table,
    and of the one-packet candidates exactly npad_before with smaller records are taken, and 64
    with larger ones.  Returns (the long connections' endpoint numbers, the pads')."""
    first = int(np.argmin(np.abs(ids[:NBIG] - 3 * (1 << 14))))
    bigs = [first] + [j for j in range(NBIG) if j != first][:nbig - 1]
    big0, pads = ids[first], ids[NBIG:]
    far = np.ones(NPAD, bool)  # (a record displaced by a probe step still sorts on the same side)
    for j in bigs:
        far &= np.abs(pads - ids[j]) > 8
    before = np.nonzero(far & (pads < big0))[0][:npad_before]
    after = np.nonzero(far & (pads > big0))[0][:64]
    assert len(before) == npad_before and len(after) == 64
    return bigs, [NBIG + int(j) for j in list(before) + list(after)]


def run_placed(parser, ids, sizes, npad_before):
    scripts = [long_script(n) for n in sizes]
    bigs, pad_ids = place(ids, len(scripts), npad_before)
    pk = Packets()
    # the long connections' packets round robin, a pad between them while pads last
    at, k = [0] * len(scripts), 0
    while any(a < len(s) for a, s in zip(at, scripts)) or k < len(pad_ids):
        for j, s in enumerate(scripts):
            if at[j] < len(s):
                fl, srv = s[at[j]]
                at[j] += 1
                c, sv = endpoints(bigs[j])
                a, b = (sv, c) if srv else (c, sv)
                pk.add(a[0], b[0], a[1], b[1], fl)
        if k < len(pad_ids):
            c, sv = endpoints(pad_ids[k])
            pk.add(c[0], sv[0], c[1], sv[1], SYN)
            k += 1
    pipe, model = Pipe(parser, 1 << 16), TR.Model()
    v, c, counts, fid, _, _ = pipe.run(pk.batch())
    wv, wc, wcounts = model.track(pk.keys(), pk.flags, fid)
    assert np.array_equal(v, wv) and np.array_equal(c, wc) and counts == wcounts
    assert np.array_equal(pipe.tracker.states(), model.states(1 << 16))
    start = int((c < c[0]).sum())  # where the first long connection begins in the sorted order
    pipe.close()
    return start, v


@pytest.mark.parametrize("which", range(4))
def test_tile_boundaries(parser, probe_ids, which):
    """One connection of T-1, T, T+1 or 2T+1 packets among one-packet connections, placed so that
    its group begins at every lane offset of the first lane, across a wave edge and a tile edge."""
    from gopacket_amd.tcptrack import SCAN_TILE as T
    size = (T - 1, T, T + 1, 2 * T + 1)[which]
    per_wave = T // 4
    for off in list(range(8)) + [per_wave - 3, per_wave, T - 1, T + 5]:
        start, v = run_placed(parser, probe_ids, [size], off)
        assert start == off, (start, off)
        assert (v & 1).sum() > size // 2 and ((v & 1) == 0).sum() > size // 40  # (the model's, too)


def test_tile_boundaries_together_and_alone(parser, probe_ids):
    from gopacket_amd.tcptrack import SCAN_TILE as T
    run_placed(parser, probe_ids, [T - 1, T, T + 1, 2 * T + 1], 37)
    run_placed(parser, probe_ids, [3 * T + 5], 0)  # (alone but for the pads behind it)
    pk = Packets()
    c, s = endpoints(0)
    for fl, srv in long_script(3 * T + 5):
        a, b = (s, c) if srv else (c, s)
        pk.add(a[0], b[0], a[1], b[1], fl)
    pipe, model = Pipe(parser, 64), TR.Model()
    v = check(pipe, model, pk)
    assert len(v) == 3 * T + 5 and np.array_equal(pipe.tracker.states(), model.states(64))
    pipe.close()


# ---------------------------------------------------------------- 4. direction
def test_direction(parser):
    A, B, C, D = 0x0A000001, 0x0A000002, 0x0A000003, 0x0A000004
    pipe, model = Pipe(parser, 256), TR.Model()
    # batch 1: A->B alone; C->D and D->C both first seen here, the server's packet first; a
    # self-reverse key; a connection whose reverse never appears
    b1 = Packets()
    b1.add(A, B, 1000, 80, SYN)
    b1.add(D, C, 80, 2000, SYN | ACK)
    b1.add(C, D, 2000, 80, SYN)
    b1.add(A, A, 7, 7, SYN)
    b1.add(A, A, 7, 7, SYN | ACK)
    b1.add(B, D, 5, 6, SYN)
    b1.add(A, B, 1000, 80, SYN)
    v1 = check(pipe, model, b1)
    assert [int(x >> 1) & 1 for x in v1] == [0, 0, 1, 0, 0, 0, 0]
    # batch 2: the reverse of A->B first appears now; C<->D in the other order; the rest again
    b2 = Packets()
    b2.add(B, A, 80, 1000, SYN | ACK)
    b2.add(A, B, 1000, 80, ACK)
    b2.add(C, D, 2000, 80, ACK)
    b2.add(D, C, 80, 2000, ACK)
    b2.add(A, A, 7, 7, RST)
    b2.add(B, D, 5, 6, ACK)
    v2, c2, counts, fid, _, _ = pipe.run(b2.batch())
    wv, wc, wcounts = model.track(b2.keys(), b2.flags, fid)
    assert np.array_equal(v2, wv) and np.array_equal(c2, wc) and counts == wcounts
    assert [int(x >> 1) & 1 for x in v2] == [1, 0, 1, 0, 0, 0]
    assert c2[0] == c2[1] and c2[0] != fid[0] and c2[1] == fid[1]  # the connection is the first-seen record
    assert c2[2] == c2[3] == fid[3] and c2[4] == fid[4]
    assert (int(v2[1]) >> 2) & 7 == TR.TCPStateEstablished and (int(v2[4]) >> 2) & 7 == TR.TCPStateReset
    assert np.array_equal(pipe.tracker.states(), model.states(256))
    pipe.close()


# ---------------------------------------------------------------- 5. ids that are no record
def test_table_too_small_gives_untracked_packets(parser, randcase):
    pipe, model = Pipe(parser, 64), TR.Model()
    v, c, counts, fid, _, _ = pipe.run(randcase.batch())
    assert (fid == FULL).sum() > 1000
    keys = [k if f < 64 else None for k, f in zip(randcase.keys(), fid)]
    wv, wc, wcounts = model.track(keys, randcase.flags, fid)
    assert np.array_equal(v, wv) and np.array_equal(c, wc) and counts == wcounts
    assert (v[fid >= 64] == 0xFF).all() and (c[fid >= 64] == NONE).all()
    assert counts[0] == (v != 0xFF).sum() and counts[1] + counts[2] == counts[0] and counts[1] == (v[v != 0xFF] & 1).sum()
    assert np.array_equal(pipe.tracker.states(), model.states(64))
    pipe.close()


def test_fingerprint_collisions_give_untracked_packets(parser, randcase):
    """Fingerprints narrowed to 7 bits: most keys share a record with another key and are flagged.
    Such packets are untracked, every other connection matches the model, the counts add up.
    Every connection is opened by one packet in a first batch and answered in later ones: with
    narrowed fingerprints a record's `first` also covers the flagged packets that landed on it in
    the launch that created it (include/gpd_tcptrack.h), so only records created in different
    batches are ordered by their own packets alone."""
    opened, first = set(), Packets()
    for i, k in enumerate(randcase.keys()):
        if k is not None and k not in opened and TR.reverse_key(k) not in opened:
            opened.add(k)
            first.add(k[0], k[1], k[2], k[3], randcase.flags[i])
    assert len(first) == 300
    pipe, model = Pipe(parser, 2048, fingerprint_bits=7), TR.Model()
    n = len(randcase)
    total = 0
    for pk, a, b in ((first, 0, len(first)), (randcase, 0, n // 2), (randcase, n // 2, n)):
        v, c, counts, fid, _, _ = pipe.run(pk.batch(a, b))
        flagged = (fid & COLLISION != 0) & (fid < FULL)
        total += int(flagged.sum())
        keys = [k if f < 2048 else None for k, f in zip(pk.keys(a, b), fid)]
        wv, wc, wcounts = model.track(keys, pk.flags[a:b], fid)
        assert np.array_equal(v, wv) and np.array_equal(c, wc) and counts == wcounts
        assert (v[flagged] == 0xFF).all() and counts[1] + counts[2] == counts[0] == (v != 0xFF).sum()
        assert set((v[v != 0xFF] >> 1) & 1) == ({0} if pk is first else {0, 1})
    assert total > 500
    assert np.array_equal(pipe.tracker.states(), model.states(2048))
    pipe.close()


# ---------------------------------------------------------------- 6. size
def test_size_past_the_first_rounds(parser):
    """The smallest batch that takes the sort's scan and the aggregate scan past their first
    round: 2^16 small connections and one with a quarter of the packets."""
    from gopacket_amd.tcpassembly import SORT_TILE
    from gopacket_amd.tcptrack import AGG_ROUND, SCAN_TILE
    n = max(16384 // 256 * SORT_TILE, AGG_ROUND * SCAN_TILE) + 1  # (16,384 counts a round, 256 per sort tile)
    assert n <= 1 << 22
    batch, keys, fl = size_case(n)
    pipe, model = Pipe(parser, 1 << 18), TR.Model()
    v, c, counts, fid, _, _ = pipe.run(batch)
    assert (fid < (1 << 18)).all()
    wv, wc, wcounts = model.track(keys, fl, fid)
    bad = np.nonzero(v != wv)[0]
    assert len(bad) == 0, (len(bad), bad[:8])
    assert np.array_equal(c, wc) and counts == wcounts and counts[3] == (1 << 16) + 1
    assert (c == c[3]).sum() == n // 4 and counts[0] == n
    assert np.array_equal(pipe.tracker.states(), model.states(1 << 18))
    pipe.close()


def test_tracked_compaction_past_the_first_round(parser):
    """compact_scan (tk_scan_kernel) takes 1,024 blocks of 2,048 packets a round: a batch of one
    block and five packets more, UDP but for every 4,099th packet and the last 3,000, so that the
    second round's blocks hold tracked packets whose places depend on the first round's total."""
    from tcptrack_cases import sparse_case
    n = 1024 * 2048 + 2048 + 5
    i = np.arange(n)
    batch, keys, fl = sparse_case(n, (i % 4099 == 0) | (i >= n - 3000))
    pipe, model = Pipe(parser, 256), TR.Model()
    v, c, counts, fid, _, _ = pipe.run(batch)
    wv, wc, wcounts = model.track(keys, fl, fid)
    bad = np.nonzero(v != wv)[0]
    assert len(bad) == 0, (len(bad), bad[:8])
    assert np.array_equal(c, wc) and counts == wcounts and 3500 < counts[0] < 3600 and counts[3] == 37
    assert np.array_equal(pipe.tracker.states(), model.states(256))
    pipe.close()


# ---------------------------------------------------------------- 7. state management
def test_states_forget_reset(parser, randcase):
    pipe, model = Pipe(parser, 2048), TR.Model()
    n = len(randcase)
    assert pipe.tracker.states().sum() == 0
    check(pipe, model, randcase, 0, n // 2)
    st = pipe.tracker.states()
    assert np.array_equal(st, model.states(2048))
    live = np.nonzero(st)[0]
    assert len(live) > 100
    gone = live[::3]
    pipe.tracker.forget(np.concatenate([gone, [5000, NONE]]).astype(np.uint32))  # (ids past the bound: ignored)
    model.forget(gone)
    st2 = pipe.tracker.states()
    assert np.array_equal(st2, model.states(2048)) and (st2[gone] == 0).all() and st2.sum() < st.sum()
    check(pipe, model, randcase, n // 2, (3 * n) // 4)
    assert np.array_equal(pipe.tracker.states(), model.states(2048))
    pipe.tracker.reset()
    model.reset()
    assert pipe.tracker.states().sum() == 0
    check(pipe, model, randcase, (3 * n) // 4, n)
    assert np.array_equal(pipe.tracker.states(), model.states(2048))
    from gopacket_amd import parser as P
    from gopacket_amd.batch import PacketBatch
    r = pipe.tracker.TrackBatch(P.DeviceBatch(PacketBatch.from_packets([]), 0), P.DeviceResult(0, 0),
                                pipe.table.Insert(P.DeviceBatch(PacketBatch.from_packets([]), 0), P.DeviceResult(0, 0)))
    assert (r.tracked, r.accepted, r.rejected, r.connections) == (0, 0, 0, 0)
    pipe.close()
    with pytest.raises(ValueError):
        pipe.tracker.states()


# ---------------------------------------------------------------- 8. the writers' mask
def test_keep_mask_selects_the_accepted_packets(parser, randcase):
    from gopacket_amd import pcapwrite
    from gopacket_amd import tcptrack as M
    pipe = Pipe(parser, 2048)
    batch = randcase.batch()
    v, _, counts, _, r, db = pipe.run(batch)
    for untracked in (False, True):
        sel, index = pcapwrite.select(parser, db, M.keep_mask(r, untracked=untracked))
        want = np.nonzero(((v & 1) == 1) & (v != 0xFF) | ((v == 0xFF) & untracked))[0]
        assert np.array_equal(index.cpu().numpy(), want) and sel.n == len(want)
        if not untracked:
            assert sel.n == counts[1] and 0 < sel.n < counts[0]
    k = int(want[len(want) // 2])
    off, cap = int(sel.offset[len(want) // 2]), int(sel.caplen[len(want) // 2])
    assert sel.data[off:off + cap].cpu().numpy().tobytes() == batch.packet(k)
    pipe.close()
