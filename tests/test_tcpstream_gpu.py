"""The TCP stream assembly on the GPU (gpd_tcp_assemble, include/gpd_tcpstream.h): records,
streams, bytes and state compared byte for byte with the oracle (tests/tcpstream_ref.py, the
restated assembler plus the cited drain), on hand-offs the device made from real frames (decode,
flow table, gpd_tcp_segments) and on hand-offs built straight from segment lists."""
import numpy as np
import pytest

import tcpassembly_ref as TA
import tcpstream_ref as SR
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.batch import PacketBatch
from tcpseg_cases import A4, A6, ACK, ALL, B4, B6, VEC, hand_built, vec_bytes, vec_want, vxlan_around
from tcpstream_cases import FIN, SYN, crafted, gen_groups

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = ALL
    return p


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _host_state(t):
    return t.cpu().numpy().view(SR.CONN_DTYPE).copy()


def _same(res, e, what=""):
    from gopacket_amd import tcpstream as S
    h = S.streams_to_host(res)
    assert (res.nrecs, res.nstreams, res.nbytes, res.ncalls) == (e.nrecs, e.nstreams, e.nbytes, e.ncalls), what
    if not np.array_equal(h.recs.view(np.uint8), e.recs.view(np.uint8)):
        k = int(np.nonzero(h.recs != e.recs)[0][0])
        raise AssertionError((what, "record", k, h.recs[max(k - 2, 0):k + 2], e.recs[max(k - 2, 0):k + 2]))
    if not np.array_equal(h.streams.view(np.uint8), e.streams.view(np.uint8)):
        k = int(np.nonzero(h.streams != e.streams)[0][0])
        raise AssertionError((what, "stream", k, h.streams[k], e.streams[k]))
    if h.bytes is not None and not np.array_equal(h.bytes, e.bytes):
        k = int(np.nonzero(h.bytes != e.bytes)[0][0])
        raise AssertionError((what, "byte", k, h.bytes[max(k - 8, 0):k + 8], e.bytes[max(k - 8, 0):k + 8]))


class Crafted:
    """A hand-off built from segment lists, on the device."""

    def __init__(self, groups, **kw):
        from gopacket_amd import parser as P
        self.batch, self.segs, self.groups = crafted(groups, **kw)
        self.db = P.DeviceBatch(self.batch, 0)
        self.dsegs, self.dgroups = _up(self.segs), _up(self.groups)

    def run(self, parser, **kw):
        from gopacket_amd import tcpstream as S
        return S.TCPStreams(parser, self.db, self.dsegs, self.dgroups, len(self.segs), len(self.groups), **kw)

    def want(self, **kw):
        return SR.assemble(self.segs, self.groups, self.batch.packet, **kw)


class Piped:
    """Real frames through the pipeline: decode, flow table, grouped segment hand-off."""

    def __init__(self, parser, frames, table, records=False, align=16):
        from gopacket_amd import parser as P
        from gopacket_amd import tcpassembly as T
        self.batch = PacketBatch.from_packets(frames, align=align)
        self.db = P.DeviceBatch(self.batch, 0)
        dr = P.DeviceResult(self.batch.n, 0, records=records)
        parser.decode_device(self.db, dr)
        ids = table.Insert(self.db, dr)
        self.dsegs, self.dgroups, self.count, self.ngroups, self.ungrouped = T.TCPSegments(
            parser, self.db, dr, flow_id=ids, table=table)
        self.segs = T.segments_to_host(self.dsegs, self.count)
        self.groups = T.groups_to_host(self.dgroups, self.ngroups)

    def run(self, parser, **kw):
        from gopacket_amd import tcpstream as S
        return S.TCPStreams(parser, self.db, self.dsegs, self.dgroups, self.count, self.ngroups, **kw)

    def want(self, **kw):
        return SR.assemble(self.segs, self.groups, self.batch.packet, **kw)


def _frames(groups, interleave_seed, sport0=1000, fill_seed=5):
    """Eth/IPv4/TCP frames for segment lists, group j on key (sport0 + j, 80), interleaved."""
    rng = np.random.default_rng(fill_seed)
    owner = [j for j, g in enumerate(groups) for _ in g]
    owner = list(np.random.default_rng(interleave_seed).permutation(owner))
    nxt = [0] * len(groups)
    out = []
    for j in owner:
        seq, flags, plen = groups[j][nxt[j]]
        nxt[j] += 1
        out.append(synth.tcp_frame(A4, B4, sport0 + j, 80, seq, ack=1, flags=flags | ACK, payload=rng.bytes(plen),
                                   pad_to=60))
    return out, owner


# ---------------------------------------------------------------- 1. the reference's vectors
@pytest.mark.parametrize("with_state", [False, True])
def test_reference_vectors(parser, with_state):
    """All eight assembly_test.go streams as real packets over eight keys in one batch, page
    limit 4: device == oracle, and the calls before the drain are the vectors' lists."""
    from gopacket_amd import tcpstream as S
    from gopacket_amd.flows import NewFlowTable
    names = list(VEC["tests"])
    assert len(names) == 8
    streams = [[synth.tcp_frame(A4, B4, 1 + j, 2, s["seq"], flags=SYN if s["syn"] else 0,
                                payload=vec_bytes(s["payload"]), pad_to=60) for s in VEC["tests"][name]]
               for j, name in enumerate(names)]
    pk, owner = [], []
    for step in range(max(map(len, streams))):
        for j, fr in enumerate(streams):
            if step < len(fr):
                pk.append(fr[step])
                owner.append(j)
    table = NewFlowTable(parser, 128)
    c = Piped(parser, pk, table)
    assert c.ngroups == 8 and c.ungrouped == 0 and c.count == len(pk)
    state = S.NewConnState(table) if with_state else None
    host_state = None if state is None else _host_state(state)
    e = c.want(max_pages=4, state=host_state)
    res = c.run(parser, state=state, max_pages_per_connection=4)
    _same(res, e)
    if with_state:
        assert np.array_equal(_host_state(state), e.state) and e.state["flags"].sum() == int(e.streams["open"].sum())
    h = S.streams_to_host(res)
    for j, name in enumerate(names):
        key = int(c.segs["flow_id"][list(c.segs["packet"]).index(owner.index(j))])
        s = h.streams[list(h.streams["flow_id"]).index(key)]
        recs = h.recs[int(s["first_rec"]):int(s["first_rec"]) + int(s["nrec"])]
        calls = []
        for ci in range(int(s["ncalls"])):
            rs = recs[recs["call"] == ci]
            if not (rs["flags"] & S.R_FLUSHED).any():
                calls.append([(h.bytes[int(r["stream_off"]):int(r["stream_off"]) + int(r["len"])].tobytes(),
                               int(r["skip"]), bool(r["flags"] & S.R_START), bool(r["flags"] & S.R_END)) for r in rs])
        assert calls == [vec_want(st) for st in VEC["tests"][name] if st["want"]], name


# ---------------------------------------------------------------- 2. random groups
@pytest.fixture(scope="module")
def randcase(parser):
    """300 generated groups of 1 to 200 segments (tests/tcpstream_cases.gen_group) as real frames
    over 300 keys, interleaved at random; decoded, keyed and handed over once."""
    from gopacket_amd.flows import NewFlowTable
    groups = gen_groups(0x5EED0051, 300)
    frames, _ = _frames(groups, interleave_seed=0x51)
    c = Piped(parser, frames, NewFlowTable(parser, 1 << 12))
    assert c.ngroups == 300 and c.ungrouped == 0 and 20000 < c.count < 40000
    return frames, c


@pytest.mark.parametrize("close_all", [False, True])
@pytest.mark.parametrize("max_pages", [0, 4])
def test_random_groups(parser, randcase, max_pages, close_all):
    _, c = randcase
    e = c.want(max_pages=max_pages, close_all=close_all)
    _same(c.run(parser, max_pages_per_connection=max_pages, close_all=close_all), e)
    r = e.recs
    assert (r["skip"] > 0).any() and (r["skip"] == -1).any() and (r["len"] == 0).any()
    assert (r["flags"] & SR.R_END).any() and (r["flags"] & SR.R_START).any() and (r["flags"] & SR.R_FLUSHED).any()
    assert (np.bincount(r["call"]) > 1).any() and int(e.streams["completed"].sum()) > 50


# ---------------------------------------------------------------- 3. the chain run's edges
def _chain(n, syn=True, start=1000, plen=7, brk=None, total=None):
    """A SYN, then in-order segments; brk = (run lane, kind): the segment at that lane of the
    first run is a gap, a one-byte retransmit or carries FIN.  n segments after the SYN."""
    segs, seq = [], start
    if syn:
        segs.append((seq, SYN, 0))
        seq += 1
    for k in range(n):
        flags, s = 0, seq
        if brk and k == brk[0]:
            if brk[1] == "gap":
                s = seq = seq + 5
            elif brk[1] == "retransmit":
                s = seq - 1
                seq = s
            else:
                flags = FIN
        ln = plen + k % 3
        segs.append((s & 0xFFFFFFFF, flags, ln))
        seq += ln
    return segs


@pytest.mark.parametrize("max_pages", [0, 4])
def test_chain_run_edges(parser, max_pages):
    """Runs of 63, 64, 65, 128 and 129 in-order segments after a SYN (one, two, three rounds of
    the 64-lane run), across the sequence wrap too; the chain broken at run lane 0, 1 and 63 by a
    gap, a one-byte retransmit and a FIN; a group with no SYN, where nothing runs before the drain."""
    groups = [_chain(n) for n in (63, 64, 65, 128, 129)]
    groups += [_chain(129, start=(1 << 32) - 300)]
    groups += [_chain(100, brk=(lane, kind)) for lane in (0, 1, 63) for kind in ("gap", "retransmit", "fin")]
    groups += [_chain(70, syn=False), _chain(1), [(5, SYN, 3)], [(5, 0, 3)]]
    c = Crafted(groups, interleave_seed=3)
    for close_all in (False, True):
        e = c.want(max_pages=max_pages, close_all=close_all)
        _same(c.run(parser, max_pages_per_connection=max_pages, close_all=close_all), e, close_all)
    assert list(e.streams["ncalls"][:5]) == [64, 65, 66, 129, 130]


# ---------------------------------------------------------------- 4. a group across the sort's tiles
def test_group_spanning_sort_tiles(parser):
    """One key over 3 x 8,192 + 1 in-order segments (more than 64 x 64 rounds of the run, its
    records and bytes across many gather waves) next to 100 one-segment keys."""
    from gopacket_amd.tcpassembly import SORT_TILE
    big = _chain(3 * SORT_TILE, plen=9)
    assert len(big) == 3 * SORT_TILE + 1
    groups = [[(100 + j, SYN if j % 2 else 0, 5)] for j in range(50)] + [big] + \
             [[(100 + j, 0, 5)] for j in range(50)]
    c = Crafted(groups, interleave_seed=4)
    e = c.want()
    _same(c.run(parser), e)
    assert int(e.streams["nrec"][50]) == len(big) and e.nstreams == 101


# ---------------------------------------------------------------- 5. state carry
def test_state_carry_over_three_batches(parser, randcase):
    """Test 2's packets cut into three batches at arbitrary packet indices, keyed by one real
    flow table and assembled with `state`; the oracle is drained (not closed) between batches."""
    from gopacket_amd import tcpstream as S
    from gopacket_amd.flows import NewFlowTable
    frames, _ = randcase
    table = NewFlowTable(parser, 1 << 12)
    state = S.NewConnState(table)
    host = _host_state(state)
    assert len(host) == 1 << 12 and not host.view(np.uint32).any()
    cuts = [0, 7919, 7919 + 12347, len(frames)]
    closed_then_reopened = 0
    for b in range(3):
        c = Piped(parser, frames[cuts[b]:cuts[b + 1]], table)
        assert c.ungrouped == 0
        e = c.want(max_pages=4, state=host)
        _same(c.run(parser, state=state, max_pages_per_connection=4), e, b)
        new = _host_state(state)
        assert np.array_equal(new, e.state)
        for s in e.streams:  # a closed key's state is zero; a later SYN opens it again
            k = int(s["flow_id"])
            if not s["open"]:
                assert tuple(new[k]) == (0, 0)
            if not host[k]["flags"] and s["open"] and s["completed"]:
                closed_then_reopened += 1
        host = new
    assert host["flags"].sum() > 50 and closed_then_reopened > 0
    # closed in one batch, opened by a SYN in the next
    syn_open = [(900, SYN, 0), (901, 0, 4), (905, FIN, 0)]
    c1 = Piped(parser, _frames([syn_open], 1, sport0=7)[0], table)
    e1 = c1.want(state=host)
    _same(c1.run(parser, state=state), e1)
    host = _host_state(state)
    k = int(c1.groups["flow_id"][0])
    assert tuple(host[k]) == (0, 0) and int(e1.streams["completed"][0]) == 1
    c2 = Piped(parser, _frames([syn_open[:2]], 1, sport0=7)[0], table)
    e2 = c2.want(state=host)
    _same(c2.run(parser, state=state), e2)
    assert int(c2.groups["flow_id"][0]) == k and tuple(_host_state(state)[k]) == (905, 1)


# ---------------------------------------------------------------- 6. gather alignment
def test_gather_alignment_and_sentinels(parser):
    """In-order segments of lengths 0 to 40, cycling (records of 0 to 15 bytes: chunks that span
    many records); TCP options and 802.1Q tags move src_off, and frames of odd sizes packed back
    to back move the packets, so that the source bytes start at every residue mod 16.  64
    sentinel bytes behind nbytes stay untouched; gather=False gives the same records and writes
    no byte."""
    import torch
    from gopacket_amd import tcpstream as S
    from gopacket_amd.flows import NewFlowTable
    rng = np.random.default_rng(6)
    frames, seqs = [], [1000, 50000, 7]
    for i in range(3 * 41 * 4):
        key, ln = i % 3, (i // 3) % 41
        opts = bytes([1] * (4 * ((i // 7) % 4)))
        flags = ACK | (SYN if ln == 0 else 0)  # (an empty segment is handed over only with a flag)
        frames.append(synth.tcp_frame(A4, B4, 300 + key, 80, seqs[key], ack=1, flags=flags, payload=rng.bytes(ln),
                                      options=opts, tags=(i // 5) % 3, pad_to=60 + i % 5))
        seqs[key] += ln + (1 if i < 3 else 0)  # (the first SYN takes a sequence number)
    c = Piped(parser, frames, NewFlowTable(parser, 128), align=1)
    assert c.ngroups == 3 and c.count == len(frames)
    e = c.want()
    _same(c.run(parser), e)
    full = e.recs[e.recs["len"] > 0]
    src = c.batch.offset[full["packet"]].astype(np.int64) + full["src_off"]
    assert set(full["src_off"] % 16) == {2, 6, 10, 14}  # (Ethernet's 14 bytes, then multiples of 4)
    assert set(src % 16) == set(range(16)) and set(e.recs["stream_off"] % 16) == set(range(16))
    assert (e.recs["len"] == 0).sum() > 10 and (e.recs["len"] < 16).sum() > 100
    s = torch.cuda.current_stream(0)
    recs = torch.zeros(e.nrecs * 32, dtype=torch.uint8, device="cuda")
    streams = torch.zeros(c.ngroups * 48, dtype=torch.uint8, device="cuda")
    byts = torch.full((e.nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, out = S._call(parser, c.db, c.dsegs, c.count, c.dgroups, c.ngroups, None, 0, 0, False, recs, e.nrecs, streams,
                      byts, e.nbytes, s)
    assert rc == 0 and out == (e.nrecs, e.nstreams, e.nbytes, e.ncalls)
    got = byts.cpu().numpy()
    assert np.array_equal(got[:e.nbytes], e.bytes) and (got[e.nbytes:] == 0xA5).all()
    byts.fill_(0xA5)
    recs.zero_()
    rc, out = S._call(parser, c.db, c.dsegs, c.count, c.dgroups, c.ngroups, None, 0, 0, False, recs, e.nrecs, streams,
                      None, 0, s)
    assert rc == 0 and out == (e.nrecs, e.nstreams, e.nbytes, e.ncalls)
    assert np.array_equal(recs.cpu().numpy(), e.recs.view(np.uint8)) and bool((byts == 0xA5).all())
    res = c.run(parser, gather=False)
    assert res.bytes is None and res.nbytes == e.nbytes
    _same(res, e)


# ---------------------------------------------------------------- 7. capacity
def test_capacity_sizing_and_empty_hand_offs(parser):
    import torch
    from gopacket_amd import tcpstream as S
    from gopacket_amd._lib import GPD_ERR_INVALID
    groups = gen_groups(77, 40, max_segments=50)
    c = Crafted(groups, keys=[2 * j + 1 for j in range(40)], interleave_seed=7)
    st0 = np.zeros(128, SR.CONN_DTYPE)
    st0[1] = ((groups[0][0][0] + 1) & 0xFFFFFFFF, 1)
    st0[5] = (12345, 1)
    e = c.want(max_pages=4, state=st0)
    s = torch.cuda.current_stream(0)
    args = (parser, c.db, c.dsegs, len(c.segs), c.dgroups, len(c.groups))
    # the sizing call
    state = _up(st0)
    rc, out = S._call(*args, state, 128, 4, False, None, 0, None, None, 0, s)
    assert rc == 0 and out == (e.nrecs, e.nstreams, e.nbytes, e.ncalls)
    assert np.array_equal(_host_state(state), st0)
    # one short in records, then in bytes: nothing written, state unchanged, out[] right
    for mr, mb in ((e.nrecs - 1, e.nbytes), (e.nrecs, e.nbytes - 1)):
        recs = torch.full((e.nrecs * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        streams = torch.full((len(c.groups) * 48,), 0xA5, dtype=torch.uint8, device="cuda")
        byts = torch.full((e.nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, out = S._call(*args, state, 128, 4, False, recs, mr, streams, byts, mb, s)
        torch.cuda.synchronize()
        assert rc == GPD_ERR_INVALID and out == (e.nrecs, e.nstreams, e.nbytes, e.ncalls)
        assert bool((recs == 0xA5).all()) and bool((streams == 0xA5).all()) and bool((byts == 0xA5).all())
        assert np.array_equal(_host_state(state), st0)
    with pytest.raises(Exception):
        c.run(parser, state=state, max_pages_per_connection=4, max_recs=e.nrecs - 1)
    assert np.array_equal(_host_state(state), st0)
    # exact capacities
    _same(c.run(parser, state=state, max_pages_per_connection=4, max_recs=e.nrecs, max_bytes=e.nbytes), e)
    assert np.array_equal(_host_state(state), e.state) and not np.array_equal(e.state, st0)
    # zero segments
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    res = S.TCPStreams(parser, c.db, empty, empty, 0, 0)
    assert (res.nrecs, res.nstreams, res.nbytes, res.ncalls) == (0, 0, 0, 0) and res.recs.numel() == 0
    # a hand-off that is only the ungrouped run (flow ids given, id_bound 0)
    un = c.segs.copy()
    un = un[np.argsort(un["packet"], kind="stable")]
    g = np.array([(SR.UNGROUPED, 0, len(un), int(un["packet"][0]))], S.GROUP_DTYPE)
    res = S.TCPStreams(parser, c.db, _up(un), _up(g), len(un), 1)
    assert (res.nrecs, res.nstreams, res.nbytes, res.ncalls) == (0, 0, 0, 0)


def test_scratch_reuse_large_then_small(parser):
    """A large call (pages beyond one per segment: the scratch grows after the page count), then
    a small one on the same context: nothing of the first is left in the second's output."""
    big = Crafted([_chain(5000, plen=2500), _chain(3000, syn=False, plen=2000)], interleave_seed=8)
    _same(big.run(parser, max_pages_per_connection=4), big.want(max_pages=4))
    small = Crafted([[(10, 0, 3), (5, 0, 3)], [(1, SYN, 2)]])
    for _ in range(2):
        _same(small.run(parser, close_all=True), small.want(close_all=True))


# ---------------------------------------------------------------- 8. the pipeline
@pytest.fixture(scope="module")
def mixframes():
    """The 20,000-packet mix of the segment hand-off's test (tests/test_tcpassembly_gpu.py): the
    traffic mix with bare ACKs, SYN / FIN frames, the hand-built cases and VXLAN-inner bare ACKs."""
    mix = synth.make_traffic_mix(19000, 0x5EED0031)
    hb = [f if cap is None else f[:cap] for f, cap, _ in hand_built()]
    pk = []
    for i in range(mix.n):
        pk.append(bytes(mix.packet(i)))
        if i % 19 == 0:
            c = i // 19
            port = 1000 + c % 37
            kind = c % 5
            if kind == 0:
                pk.append(synth.tcp_frame(A4, B4, port, 80, c, ack=1, flags=ACK, pad_to=60))
            elif kind == 1:
                pk.append(synth.tcp_frame(A4, B4, port, 80, c, flags=TA.SYN, pad_to=60))
            elif kind == 2:
                pk.append(synth.tcp_frame(A6, B6, port, 80, c, ack=1, flags=TA.FIN | ACK))
            elif kind == 3:
                pk.append(vxlan_around(synth.tcp_frame(A4, B4, port, 80, c, ack=1, flags=ACK, pad_to=60)))
            else:
                pk.append(hb[c % len(hb)])
    return pk


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("capacity", [128, 1 << 17])
def test_pipeline(parser, mixframes, capacity, records):
    """Decode, a real flow table (128 records: full, with an ungrouped tail; 2^17), the grouped
    hand-off and the assembly, in both result forms."""
    from gopacket_amd import tcpstream as S
    from gopacket_amd.flows import NewFlowTable
    table = NewFlowTable(parser, capacity)
    c = Piped(parser, mixframes, table, records=records)
    assert 19000 < c.batch.n < 21000 and c.count > 5000
    assert (c.ungrouped > 0) == (capacity == 128)
    state = S.NewConnState(table)
    e = c.want(max_pages=4, close_all=True, state=_host_state(state))
    res = c.run(parser, state=state, max_pages_per_connection=4, close_all=True)
    _same(res, e)
    assert np.array_equal(_host_state(state), e.state)
    assert e.nstreams == c.ngroups - (1 if c.ungrouped else 0) and e.nrecs > (100 if c.ungrouped else 1000)
