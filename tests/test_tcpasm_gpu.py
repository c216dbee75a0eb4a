"""The stateful TCP assembler on the GPU (gpd_tcp_assembler_run, include/gpd_tcpasm.h): records,
seen_ns, streams, bytes, conns(), stats() and out[] compared byte for byte with the oracle
(tests/tcpasm_ref.py: one restated reference assembler per key, alive across runs), run after
run, on hand-offs the device made from real frames and on hand-offs built from segment lists."""
import numpy as np
import pytest

import tcpasm_ref as AR
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.batch import PacketBatch
from tcpasm_cases import cut_all, set_payloads
from tcpseg_cases import A4, ALL, B4
from tcpstream_cases import FIN, SYN, crafted, gen_groups
from test_tcpstream_gpu import Piped, _chain, _frames, _up

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = ALL
    return p


def _same(asm, res, e, what=""):
    from gopacket_amd import tcpasm as M
    h = M.to_host(res)
    got = (res.nrecs, res.nstreams, res.nbytes, res.ncalls, res.connections, res.pages, res.page_bytes, 0)
    assert got == e.out, (what, got, e.out)
    if not np.array_equal(h.recs.view(np.uint8), e.recs.view(np.uint8)):
        k = int(np.nonzero(h.recs != e.recs)[0][0])
        raise AssertionError((what, "record", k, h.recs[max(k - 2, 0):k + 2], e.recs[max(k - 2, 0):k + 2]))
    assert np.array_equal(h.seen_ns, e.seen_ns), (what, "seen")
    if not np.array_equal(h.streams.view(np.uint8), e.streams.view(np.uint8)):
        k = int(np.nonzero(h.streams != e.streams)[0][0])
        raise AssertionError((what, "stream", k, h.streams[k], e.streams[k]))
    if not np.array_equal(h.bytes, e.bytes):
        k = int(np.nonzero(h.bytes != e.bytes)[0][0])
        raise AssertionError((what, "byte", k, h.bytes[max(k - 8, 0):k + 8], e.bytes[max(k - 8, 0):k + 8]))
    conns = asm.conns()
    if not np.array_equal(conns.view(np.uint8), e.conns.view(np.uint8)):
        k = int(np.nonzero(conns != e.conns)[0][0])
        raise AssertionError((what, "conn", k, conns[k], e.conns[k]))
    assert asm.stats() == e.stats, what
    return h


class Pair:
    """A device assembler and the oracle, fed the same runs."""

    def __init__(self, parser, id_bound, max_pages=0):
        from gopacket_amd import tcpasm as M
        self.parser = parser
        self.dev, self.ref = M.NewAssembler(parser, id_bound, max_pages), AR.Model(id_bound, max_pages)

    def feed(self, batch, segs, groups, ts=None, what="", db=None, dsegs=None, dgroups=None, **kw):
        """One hand-off through both; the batch's device buffers are overwritten afterwards.
        kw: now, T, close_all, flush_all.  Returns (device result on the host, oracle's)."""
        import torch
        from gopacket_amd import parser as P
        db = P.DeviceBatch(batch, 0) if db is None else db
        dsegs = _up(segs) if dsegs is None else dsegs
        dgroups = _up(groups) if dgroups is None else dgroups
        dts = None if ts is None else torch.from_numpy(np.asarray(ts, np.int64)).cuda()
        e = self.ref.run(segs, groups, batch.packet, ts=ts, now=kw.get("now", 0), T=kw.get("T", 0),
                         close_all=kw.get("close_all", False), flush_all=kw.get("flush_all", False))
        res = self.dev.AssembleBatch(db, dsegs, dgroups, len(segs), len(groups), ts=dts, now=kw.get("now", 0),
                                     flush_older_than=kw.get("T", 0), close_all=kw.get("close_all", False),
                                     flush_all=kw.get("flush_all", False))
        db.data.fill_(0xEE)  # the caller reuses its buffers: carried pages must not depend on them
        dsegs.fill_(0xEE)
        dgroups.fill_(0xEE)
        torch.cuda.synchronize()
        return _same(self.dev, res, e, what), e

    def flush(self, T=0, close_all=False, flush_all=False, what=""):
        e = self.ref.run(T=T, close_all=close_all, flush_all=flush_all)
        if flush_all and not T:
            res = self.dev.FlushAll()
        else:
            res = self.dev.AssembleBatch(None, None, None, 0, 0, flush_older_than=T, close_all=close_all,
                                         flush_all=flush_all)
        return _same(self.dev, res, e, what), e

    def close(self):
        self.dev.close()


def _key_calls(model, key_of):
    """{connection: call lists over all runs} with the model's flow ids mapped by key_of."""
    return {key_of[k]: AR.call_lists(ev) for k, ev in model.keys.items()}


# ---------------------------------------------------------------- 1. cut-independence
@pytest.fixture(scope="module")
def randframes():
    groups = gen_groups(0x5EED0051, 300)
    frames, owner = _frames(groups, interleave_seed=0x51)
    return frames, owner


def test_cut_independence(parser, randframes):
    """The 300 generated connections of the stream assembly's test as real frames through one
    flow table per cutting: whole, cut in two and cut in three at arbitrary packet indices, T = 0
    throughout and a final FlushAll.  Every run equals the oracle's; per connection the
    concatenated call lists (bytes, Skip, Start, End, Seen) are the same for all three cuttings,
    the whole run being one reference assembler fed everything.  In the cut runs some connection
    gets, in a later batch, the segment that fills a gap an earlier batch left: its carried pages
    come out behind it in the same call with Skip 0."""
    from gopacket_amd.flows import NewFlowTable
    frames, owner = randframes
    n = len(frames)
    stamps = 1000 + 10 * np.arange(n, dtype=np.int64)
    per_cutting, filled = [], 0
    for cuts in ([0, n], [0, 11003, n], [0, 7919, 7919 + 12347, n]):
        table = NewFlowTable(parser, 1 << 12)
        p = Pair(parser, 1 << 12, max_pages=4)
        key_of = {}
        for b in range(len(cuts) - 1):
            c = Piped(parser, frames[cuts[b]:cuts[b + 1]], table)
            assert c.ungrouped == 0
            for r in c.segs:
                key_of[int(r["flow_id"])] = owner[cuts[b] + int(r["packet"])]
            h, e = p.feed(c.batch, c.segs, c.groups, ts=stamps[cuts[b]:cuts[b + 1]], what=(len(cuts), b), db=c.db,
                          dsegs=c.dsegs, dgroups=c.dgroups)
            if b:
                fl = h.recs["flags"]
                sid = np.repeat(np.arange(len(h.streams)), h.streams["nrec"])
                mid = (fl & AR.R_CARRIED != 0) & (fl & AR.R_FLUSHED == 0) & (sid == np.roll(sid, 1))
                mid &= h.recs["call"] == np.roll(h.recs["call"], 1)
                mid &= np.roll(fl, 1) & AR.R_CARRIED == 0  # behind a record of this batch, in its call
                assert (h.recs["skip"][mid] == 0).all()
                filled += int(mid.sum())
        p.flush(flush_all=True, what="FlushAll")
        assert p.dev.stats()["connections"] == 0
        per_cutting.append(_key_calls(p.ref, key_of))
        p.close()
    assert len(per_cutting[0]) == 300 and filled > 0
    assert per_cutting[1] == per_cutting[0] and per_cutting[2] == per_cutting[0]


# ---------------------------------------------------------------- 2. flush by time
def _multi(groups, keys):
    batch, segs, grp = crafted([[(s, f, len(p)) for s, f, p in g] for g in groups], keys=keys, interleave_seed=None)
    set_payloads(batch, segs, [p for g in groups for _, _, p in g])
    return batch, segs, grp


def test_flush_by_time(parser):
    """The hand-checked flush cases of tests/test_tcpasm.py as real runs with timestamps, among
    connections that have no segment in the flushing run (the extra items, in ascending id behind
    the run's groups): Seen == T and lastSeen == T do nothing, T between two pages' Seen sends the
    first run of contiguous pages only, close_all closes drained connections with and without
    pages pending elsewhere, and runs with count == 0."""
    example = [(9, SYN, b""), (15, 0, b"AAAAA"), (20, 0, b"BBBBB"), (30, 0, b"C" * 20)]
    nosyn = [(1001, 0, b"abc"), (1010, 0, b"xyz")]
    idle = [(50, SYN, b"hi"), (53, 0, b"there")]
    late = [(700, SYN, b""), (701, 0, b"q")]
    batch, segs, grp = _multi([idle, example, nosyn, late], keys=[2, 5, 9, 11])
    # packets in capture order: idle 0-1, example 2-5, nosyn 6-7, late 8-9
    ts = [10, 20, 100, 200, 300, 400, 50, 60, 900, 950]
    p = Pair(parser, 16)
    h, e = p.feed(batch, segs, grp, ts=ts, what="fill")
    assert tuple(e.conns[5]) == (10, 1, 3, 30, 400) and tuple(e.conns[9]) == (0, 3, 2, 6, 60)
    assert e.stats == {"connections": 4, "connections_with_pages": 2, "pages": 5, "page_bytes": 36}
    # key 5's first page was seen at 200: not before T.  Key 9's pages (50, 60) are: two calls, two gaps
    h, e = p.flush(T=200, close_all=False, what="Seen == T")
    assert list(h.streams["flow_id"]) == [9] and list(h.recs["skip"]) == [-1, 6] and list(h.seen_ns) == [50, 60]
    assert list(h.recs["call"]) == [0, 1] and tuple(e.conns[5]) == (10, 1, 3, 30, 400)
    # a run with segments for key 11 only; T = 250 flushes keys 5 and 9, close_all closes key 2
    b2, s2, g2 = _multi([[(702, 0, b"rs")]], keys=[11])
    h, e = p.feed(b2, s2, g2, ts=[960], T=250, close_all=True, what="T = 250")
    assert list(h.streams["flow_id"]) == [11, 2, 5, 9] and list(h.streams["completed"]) == [0, 1, 0, 1]
    k5 = h.recs[int(h.streams["first_rec"][2]):][:2]
    assert list(k5["skip"]) == [5, 0] and list(k5["call"]) == [0, 0] and list(k5["packet"]) == [AR.NO_PACKET] * 2
    assert list(k5["flags"]) == [AR.R_FLUSHED | AR.R_CARRIED] * 2
    assert tuple(e.conns[5]) == (25, 1, 1, 20, 400) and not e.conns[2]["flags"] and not e.conns[9]["flags"]
    h, e = p.flush(T=400, close_all=True, what="Seen == T again")
    assert len(h.streams) == 0 and e.out == (0, 0, 0, 0, 2, 1, 20, 0)
    h, e = p.flush(T=401, what="later T")
    assert list(h.recs["skip"]) == [5] and h.bytes.tobytes() == b"C" * 20 and list(h.seen_ns) == [400]
    h, e = p.flush(T=400, close_all=True, what="lastSeen == T")
    assert len(h.streams) == 0 and e.stats["connections"] == 2
    res = p.dev.FlushOlderThan(401)  # closes key 5 (lastSeen 400), not key 11 (960)
    e = p.ref.run(T=401, close_all=True)
    h = _same(p.dev, res, e, "FlushOlderThan")
    assert list(h.streams["flow_id"]) == [5] and list(h.streams["completed"]) == [1] and e.stats["connections"] == 1
    h, e = p.flush(T=1 << 62, close_all=True, what="all")
    assert e.stats["connections"] == 0 and list(h.streams["flow_id"]) == [11]
    h, e = p.flush(T=1 << 62, close_all=True, flush_all=True, what="nothing held")
    assert e.out == (0,) * 8
    p.close()


# ---------------------------------------------------------------- 3. list mechanics across runs
@pytest.mark.parametrize("max_pages", [0, 1, 4])
def test_list_mechanics_across_runs(parser, max_pages):
    """A 4,000-byte segment (3 pages) carried and a later segment landing between its pages; a
    segment before the carried first page that makes the whole list contiguous; a connection with
    no SYN whose SYN never comes; a SYN that arrives after data was carried with NOSEQ; the page
    limit counting carried pages (max_pages 1 and 4)."""
    Z = lambda n, c=0x41: bytes([c]) * n
    runs = [
        [[(99, SYN, b""), (1000, 0, Z(4000))], [(9, SYN, b""), (15, 0, Z(5)), (20, 0, Z(5, 0x42))],
         [(1001, 0, b"abc"), (1010, 0, b"xyz")], [(5001, 0, Z(2500, 0x43))], [(7, 0, Z(3)), (40, 0, Z(3)), (30, 0, Z(3))]],
        [[(2000, 0, Z(100, 0x44)), (5100, 0, Z(10, 0x45))], [(10, 0, Z(5, 0x46))], [(1020, 0, b"more")],
         [(5000, SYN, b"")], [(20, 0, Z(3)), (50, 0, Z(3)), (10, 0, Z(3))]],
        [[(100, 0, Z(900, 0x47))], [(25, FIN, b"")], [(1004, 0, Z(6, 0x48))], [(7501, 0, b"tail")],
         [(60, 0, Z(3)), (13, 0, Z(3))]],
    ]
    p = Pair(parser, 8, max_pages=max_pages)
    for k, groups in enumerate(runs):
        batch, segs, grp = _multi(groups, keys=[0, 1, 3, 4, 6])
        h, e = p.feed(batch, segs, grp, ts=[100 * k + i for i in range(batch.n)], what=k)
        if k == 0 and max_pages == 0:
            assert tuple(e.conns[0])[:4] == (100, 1, 3, 4000) and tuple(e.conns[3])[:4] == (0, 3, 2, 6)
        if k == 1 and max_pages == 0:
            assert tuple(e.conns[0])[:4] == (100, 1, 5, 4110)
            s1 = h.streams[1]  # (10..15) fills: one call, the two carried pages behind it with Skip 0
            r1 = h.recs[int(s1["first_rec"]):int(s1["first_rec"]) + int(s1["nrec"])]
            assert list(r1["skip"]) == [0, 0, 0] and list(r1["flags"]) == [0, AR.R_CARRIED, AR.R_CARRIED]
            s4 = h.streams[3]  # the SYN after carried NOSEQ data: Start, then the carried pages
            r4 = h.recs[int(s4["first_rec"]):int(s4["first_rec"]) + int(s4["nrec"])]
            assert list(r4["flags"]) == [AR.R_START, AR.R_CARRIED, AR.R_CARRIED] and int(s4["open"]) == 1
    h, e = p.flush(flush_all=True, what="FlushAll")
    assert e.stats["connections"] == 0
    p.close()


# ---------------------------------------------------------------- 4. chain-run edges with carry
def _after_carry(n, drain_at, plen=7):
    """Run 1: a SYN at 999 and one out-of-order page; run 2: n in-order segments from 1000 that
    step over the page's bytes.  drain_at = d: segment d of run 2 ends where the page begins, so
    the list drains there; None: the page lies far ahead and never drains."""
    lens = [plen + k % 3 for k in range(n)]
    page_len = 11
    if drain_at is None:
        page_seq = 10_000_000
    else:
        page_seq = 1000 + sum(lens[:drain_at + 1])
    run1 = [(999, SYN, 0), (page_seq, 0, page_len)]
    run2, seq = [], 1000
    for k, ln in enumerate(lens):
        run2.append((seq, 0, ln))
        seq += ln
        if drain_at is not None and k == drain_at:
            seq += page_len
    return run1, run2


def test_chain_run_edges_with_carry(parser):
    """63 to 129 in-order segments behind a carried list that drains at segment 0, 1 and 63 of
    the run (the in-order run of the wave starts right after), and behind one that never drains
    (the run must stay off: every segment takes the step, the page stays)."""
    cases = [(n, d) for n in (63, 64, 65, 128, 129) for d in (0, 1, 63, None) if d is None or d < n]
    first = [_after_carry(n, d)[0] for n, d in cases]
    second = [_after_carry(n, d)[1] for n, d in cases]
    p = Pair(parser, len(cases))
    b1, s1, g1 = crafted(first, interleave_seed=5)
    h, e = p.feed(b1, s1, g1, ts=list(range(b1.n)), what="carry")
    assert e.stats["pages"] == len(cases)
    b2, s2, g2 = crafted(second, interleave_seed=6)
    h, e = p.feed(b2, s2, g2, ts=list(range(1000, 1000 + b2.n)), what="runs")
    for j, (n, d) in enumerate(cases):
        assert int(h.streams["ncalls"][j]) == n and int(h.streams["nrec"][j]) == n + (d is not None)
        assert int(h.streams["reserved"][j]) == (1 if d is None else 0)
    p.flush(flush_all=True, what="FlushAll")
    p.close()


# ---------------------------------------------------------------- 5. gather
def test_gather_alignment_and_sentinels(parser):
    """Carried pages of 1 to 15 bytes (and a duplicate that is trimmed to 0 bytes) in 16
    connections.  Run 2 adds a page far ahead, so every page moves from the old store to the new
    one; run 3 fills each connection's one-byte gap, so all of them move from the store to the
    output, each stream one byte further along: every store offset mod 16 meets every output
    offset mod 16.  64 sentinel bytes behind the counted output bytes stay untouched."""
    import torch
    from gopacket_amd import parser as P
    from gopacket_amd import tcpasm as M
    lens = list(range(1, 16)) * 3
    pages, seq = [], 1001
    for i, ln in enumerate(lens):
        pages.append((seq, 0, ln))
        if i == 3:
            pages.append((seq, 0, ln))  # a retransmit: delivered as 0 bytes
        seq += ln
    nconn = 16
    p = Pair(parser, nconn)
    b1, s1, g1 = crafted([[(999, SYN, 0)] + pages for _ in range(nconn)], interleave_seed=11)
    p.feed(b1, s1, g1, what="pages")
    b2, s2, g2 = crafted([[(5000, 0, 8)] for _ in range(nconn)], interleave_seed=12)
    p.feed(b2, s2, g2, what="store to store")
    # where the pages lie in the store now: the connections in id order, each list in order
    store_off, at = [], 0
    for k in range(nconn):
        q = p.ref.conn(k).first
        while q is not None:
            store_off.append(at)
            at += len(q.r.Bytes)
            q = q.next
    b3, s3, g3 = crafted([[(1000, 0, 1)] for _ in range(nconn)], interleave_seed=13)
    e = p.ref.run(s3, g3, b3.packet)
    carried = e.recs[e.recs["flags"] & AR.R_CARRIED != 0]
    assert len(carried) == nconn * len(pages) and (carried["len"] == 0).sum() == nconn
    left = [o for o, pg in zip(store_off, [pg for _ in range(nconn) for pg in pages + [None]]) if pg is not None]
    pairs = {(int(a) % 16, int(b) % 16) for a, b in zip(left, carried["stream_off"])}
    assert len(pairs) == 256 and set(carried["len"]) == set(range(16))
    db, dsegs, dgroups = P.DeviceBatch(b3, 0), _up(s3), _up(g3)
    recs = torch.zeros(e.out[0] * 32, dtype=torch.uint8, device="cuda")
    seen = torch.zeros(e.out[0], dtype=torch.int64, device="cuda")
    streams = torch.zeros(e.out[1] * 48, dtype=torch.uint8, device="cuda")
    byts = torch.full((e.out[2] + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, out = p.dev.run_raw(db, dsegs, len(s3), dgroups, len(g3), None, 0, (0, False, False), recs, e.out[0], seen,
                            streams, e.out[1], byts, e.out[2])
    assert rc == 0 and out == e.out
    got = byts.cpu().numpy()
    assert np.array_equal(got[:e.out[2]], e.bytes) and (got[e.out[2]:] == 0xA5).all()
    assert np.array_equal(recs.cpu().numpy(), e.recs.view(np.uint8))
    assert np.array_equal(p.dev.conns().view(np.uint8), e.conns.view(np.uint8)) and p.dev.stats() == e.stats
    p.flush(flush_all=True, what="FlushAll")
    p.close()


# ---------------------------------------------------------------- 6. capacity and reset
def test_capacity_sizing_reset_and_scratch_reuse(parser):
    import torch
    from gopacket_amd import parser as P
    from gopacket_amd._lib import GPD_ERR_INVALID
    groups = gen_groups(77, 40, max_segments=50)
    batch, segs, grp = crafted(groups, keys=[2 * j + 1 for j in range(40)], interleave_seed=7)
    n = batch.n
    (b1, s1, g1), (b2, s2, g2) = cut_all(batch, segs, [0, n // 2, n])
    p = Pair(parser, 128, max_pages=4)
    p.feed(b1, s1, g1, ts=list(range(n // 2)), what="first half")
    before_conns, before_stats = p.dev.conns(), p.dev.stats()
    assert before_stats["pages"] > 0
    ts2 = list(range(n // 2, n))
    e = p.ref.run(s2, g2, b2.packet, ts=ts2, T=n // 2 + 5, close_all=True)
    nr, ns, nb = e.out[:3]
    db, dsegs, dgroups = P.DeviceBatch(b2, 0), _up(s2), _up(g2)
    dts = torch.from_numpy(np.asarray(ts2, np.int64)).cuda()
    head = (db, dsegs, len(s2), dgroups, len(g2), dts, 0, (n // 2 + 5, True, False))
    rc, out = p.dev.run_raw(*head, None, 0, None, None, 0, None, 0)  # the sizing call
    assert rc == 0 and out == e.out
    assert np.array_equal(p.dev.conns(), before_conns) and p.dev.stats() == before_stats
    for mr, ms, mb in ((nr - 1, ns, nb), (nr, ns - 1, nb), (nr, ns, nb - 1)):
        recs = torch.full((nr * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        seen = torch.full((nr,), -1, dtype=torch.int64, device="cuda")
        streams = torch.full((ns * 48,), 0xA5, dtype=torch.uint8, device="cuda")
        byts = torch.full((nb + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, out = p.dev.run_raw(*head, recs, mr, seen, streams, ms, byts, mb)
        torch.cuda.synchronize()
        assert rc == GPD_ERR_INVALID and out[:4] == e.out[:4]
        assert bool((recs == 0xA5).all()) and bool((streams == 0xA5).all()) and bool((byts == 0xA5).all())
        assert bool((seen == -1).all())
        assert np.array_equal(p.dev.conns(), before_conns) and p.dev.stats() == before_stats
    # a group whose flow id is not below id_bound is refused, nothing changes
    bad = g2.copy()
    bad["flow_id"][-1] = 128
    rc, out = p.dev.run_raw(db, dsegs, len(s2), _up(bad), len(g2), dts, 0, (0, False, False), None, 0, None, None, 0,
                            None, 0)
    assert rc == GPD_ERR_INVALID and np.array_equal(p.dev.conns(), before_conns)
    # the repeated call with enough room equals the oracle
    res = p.dev.AssembleBatch(db, dsegs, dgroups, len(s2), len(g2), ts=dts, flush_older_than=n // 2 + 5, close_all=True)
    _same(p.dev, res, e, "second half")
    # reset zeroes everything
    p.dev.reset()
    assert not p.dev.conns().view(np.uint8).any() and p.dev.stats() == AR.Model(128).stats()
    res = p.dev.FlushAll()
    assert (res.nrecs, res.nstreams, res.connections) == (0, 0, 0)
    p.close()
    # scratch reuse, large then small
    q = Pair(parser, 4)
    big = [_chain(3000, plen=2500), _chain(2000, syn=False, plen=2000)]
    bb, sb, gb = crafted(big, interleave_seed=8)
    q.feed(bb, sb, gb, what="large")
    small = [[(10, 0, 3), (5, 0, 3)], [(1, SYN, 2)]]
    bs, ss, gs = crafted(small, keys=[2, 3])
    for k in range(2):
        q.feed(bs, ss, gs, T=1 << 62, close_all=True, what=("small", k))
    q.close()


# ---------------------------------------------------------------- 7. the pipeline
def test_pipeline_fragmented_reordered_tcp_over_three_batches(parser):
    """Four TCP conversations whose segments arrive IP-fragmented and reordered, across three
    batches: decode -> IPv4Fragments -> DefragBatch -> decode of the datagrams -> flow table ->
    TCPSegments -> AssembleBatch, the defragmenter, the table and the assembler living across the
    batches.  Every conversation's stream is the bytes that were sent, with no gap, and equals the
    stream of the same conversation sent in order in one batch."""
    from gopacket_amd import defrag as DF
    from gopacket_amd import ip4reasm as I
    from gopacket_amd import parser as P
    from gopacket_amd import tcpasm as M
    from gopacket_amd import tcpassembly as T
    from gopacket_amd.flows import NewFlowTable
    from test_ip4reasm_gpu import _fragment
    rng = np.random.default_rng(12)
    sent, ordered, shuffled, ident = {}, [], [], 100
    for c in range(4):
        seq = 1000 * (c + 1)
        segs = [(seq, 0x02, b"")]
        seq += 1
        for _ in range(9):
            pay = rng.bytes(int(rng.integers(200, 1400)))
            segs.append((seq, 0x18, pay))
            seq += len(pay)
        segs.append((seq, 0x11, b""))
        sent[5000 + c] = b"".join(pay for _, _, pay in segs)
        frames = [synth.tcp_frame(A4, B4, 5000 + c, 80, s, ack=1, flags=fl, payload=pay) for s, fl, pay in segs]
        ordered.append(frames)
        data = frames[1:-1]
        data = [data[i] for i in rng.permutation(len(data))]  # reordered far enough to cross the cuts
        parts = []
        for f in data:
            ident += 1
            fr = _fragment(f, ident, [8 * int(rng.integers(3, 40)) for _ in range(3)])
            parts += [fr[i] for i in rng.permutation(len(fr))]
        shuffled.append([frames[0]] + parts + [frames[-1]])
    mixed, nxt = [], [0] * 4
    while any(nxt[c] < len(shuffled[c]) for c in range(4)):
        c = int(rng.integers(4))
        if nxt[c] < len(shuffled[c]):
            mixed.append(shuffled[c][nxt[c]])
            nxt[c] += 1
    p4 = P.NewDecodingLayerParser(L.LayerTypeIPv4)
    p4._mask = ALL

    def run(batches, fragmented):
        table = NewFlowTable(p4, 256)
        asm = M.NewAssembler(p4, table)
        defrag = I.NewIPv4Defragmenter(parser) if fragmented else None
        fac_calls, pool = {}, {}

        class Fac:
            def New(self, key):
                class St:
                    def Reassembled(self, rs):
                        fac_calls.setdefault(key, []).extend(r.as_tuple() for r in rs)

                    def ReassemblyComplete(self):
                        pass
                return St()
        port_of = {}
        for frames in batches:
            ip = [f[14:] for f in frames]
            if fragmented:
                batch = PacketBatch.from_packets(frames)
                db = P.DeviceBatch(batch, 0)
                dr = P.DeviceResult(batch.n, 0)
                parser.decode_device(db, dr)
                out, cnt = DF.IPv4Fragments(parser, db, dr)
                recs = DF.fragments_to_host(out, cnt)
                h = I.defrag_to_host(defrag.DefragBatch(db, out, cnt))
                done = {int(g["packet"]): k for k, g in enumerate(h.dgrams)}
                frag_pk = {int(r["packet"]) for r in recs}
                ip = []
                for i, f in enumerate(frames):
                    if i in done:
                        k = done[i]
                        ip.append(h.bytes[int(h.offset[k]):int(h.offset[k]) + int(h.caplen[k])].tobytes())
                    elif i not in frag_pk:
                        ip.append(f[14:])
            if not ip:
                continue
            dbatch = P.DeviceBatch(PacketBatch.from_packets(ip), 0)
            d = P.DeviceResult(dbatch.n, 0)
            p4.decode_device(dbatch, d)
            ids = table.Insert(dbatch, d)
            dsegs, dgroups, count, ngroups, ungrouped = T.TCPSegments(p4, dbatch, d, flow_id=ids, table=table)
            assert ungrouped == 0
            for r in T.segments_to_host(dsegs, count):
                port_of[int(r["flow_id"])] = int.from_bytes(ip[int(r["packet"])][20:22], "big")
            M.deliver(asm.AssembleBatch(dbatch, dsegs, dgroups, count, ngroups), Fac(), pool)
            dbatch.data.fill_(0xEE)
        M.deliver(asm.FlushAll(), Fac(), pool)
        assert asm.stats()["connections"] == 0
        asm.close()
        if defrag is not None:
            assert defrag.stats()["lists"] == 0
            defrag.close()
        return {port_of[k]: v for k, v in fac_calls.items()}

    n = len(mixed)
    cut = run([mixed[:n // 3], mixed[n // 3:2 * n // 3], mixed[2 * n // 3:]], True)
    whole = run([[f for k in range(11) for c in range(4) for f in [ordered[c][k]]]], False)
    assert set(cut) == set(sent)
    for port, want in sent.items():
        assert all(skip == 0 for _, skip, _, _ in cut[port]) and all(skip == 0 for _, skip, _, _ in whole[port])
        assert b"".join(b for b, _, _, _ in cut[port]) == want == b"".join(b for b, _, _, _ in whole[port])
