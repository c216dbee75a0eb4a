"""The IPv4 defragmentation on the GPU (gpd_ip4_defrag_run, include/gpd_ip4reasm.h): outcomes,
datagram records, offset / caplen, bytes and stats compared byte for byte with the oracle
(tests/ip4reasm_ref.py, the restated ip4defrag driven in packet order), on hand-offs the device
made from real frames (decode, gpd_ip4_fragments), all through the C-ABI."""
import struct

import numpy as np
import pytest

import ip4reasm_ref as RR
import oracle_ref as O
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.batch import PacketBatch
from ip4reasm_cases import frames_of, in_order, interleave, key_of, quirk_complete, random_frames, spec
from test_defrag import ALL, VEC, _frames, ip4_frame, struct_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = ALL
    return p


class Pair:
    """A device defragmenter and the oracle, fed the same batches."""

    def __init__(self, parser):
        from gopacket_amd import ip4reasm as I
        self.parser, self.dev, self.ref = parser, I.NewIPv4Defragmenter(parser), RR.RefDefragmenter()

    def handoff(self, frames, align=16):
        import torch
        from gopacket_amd import defrag as DF
        from gopacket_amd import parser as P
        batch = PacketBatch.from_packets(frames, align=align)
        db = P.DeviceBatch(batch, 0)
        dr = P.DeviceResult(batch.n, 0)
        self.parser.decode_device(db, dr)
        out, cnt = DF.IPv4Fragments(self.parser, db, dr)
        torch.cuda.synchronize()
        return batch, db, out, cnt, DF.fragments_to_host(out, cnt)

    def feed(self, frames, ts=None, now=0, align=16, what="", scrub=False, **kw):
        """One batch through both; asserts equality and returns (device result on the host, oracle's)."""
        import torch
        from gopacket_amd import ip4reasm as I
        batch, db, out, cnt, recs = self.handoff(frames, align)
        dts = None if ts is None else torch.from_numpy(np.asarray(ts, np.int64)).cuda()
        e = self.ref.run(batch, recs, ts=ts, now=now)
        res = self.dev.DefragBatch(db, out, cnt, ts=dts, now=now, **kw)
        h = I.defrag_to_host(res)
        if scrub:  # the caller frees or reuses its buffers: carried fragments must not depend on them
            db.data.fill_(0xEE)
            out.fill_(0xEE)
            torch.cuda.synchronize()
        same(res, h, e, what)
        assert self.dev.stats() == self.ref.stats(), what
        assert res.nlists == self.ref.stats()["lists"], what
        return h, e

    def close(self):
        self.dev.close()


def same(res, h, e, what=""):
    assert (res.ndgrams, res.noutcomes, res.nbytes) == (len(e.dgrams), len(e.outcomes), len(e.bytes)), what
    if not np.array_equal(h.outcomes.view(np.uint8), e.outcomes.view(np.uint8)):
        k = int(np.nonzero(h.outcomes != e.outcomes)[0][0])
        raise AssertionError((what, "outcome", k, h.outcomes[max(k - 2, 0):k + 2], e.outcomes[max(k - 2, 0):k + 2]))
    if not np.array_equal(h.dgrams.view(np.uint8), e.dgrams.view(np.uint8)):
        k = int(np.nonzero(h.dgrams != e.dgrams)[0][0])
        raise AssertionError((what, "datagram", k, h.dgrams[k], e.dgrams[k]))
    if h.bytes is not None:
        assert np.array_equal(h.offset, e.offset) and np.array_equal(h.caplen, e.caplen), what
        if not np.array_equal(h.bytes, e.bytes):
            k = int(np.nonzero(h.bytes != e.bytes)[0][0])
            raise AssertionError((what, "byte", k, h.bytes[max(k - 8, 0):k + 8], e.bytes[max(k - 8, 0):k + 8]))


# ---------------------------------------------------------------- 1. the reference's vectors
def test_reference_vectors(parser):
    """defrag_test.go's eight ping fragments in TestDefragPing1and2's order and the struct cases
    as real frames, interleaved over their three keys: the ping payloads byte for byte."""
    fr = _frames()
    a = VEC["asserted"]
    pings = [fr[k] for k in a["ping1_and2_order"]]
    frames = interleave(np.random.default_rng(1), [pings, [f for _, f in struct_frames()]])
    p = Pair(parser)
    h, e = p.feed(frames)
    assert len(h.dgrams) == 2 and set(h.outcomes["what"]) == {RR.FILED, RR.COMPLETE, RR.REJECTED}
    for k, ping in enumerate((1, 2)):
        want = b"".join(fr[f"testPing{ping}Frag{j}"][a["payload_from"]:] for j in (1, 2, 3, 4))
        o = int(h.offset[k])
        assert h.bytes[o + 20:o + int(h.caplen[k])].tobytes() == want
    p.close()


# ---------------------------------------------------------------- 2. random groups
def test_random_groups(parser):
    """300 generated groups (tests/ip4reasm_cases.gen_group: permutations, duplicates, overlaps
    under both of build's branches and the :298 quirk, holes followed by the missing piece,
    missing first or last fragments, id reuse, IHL 6-15, truncated payloads, Length 0, keys that
    differ in one field only, VXLAN-inner fragments) interleaved in one batch, then a second batch
    of 100 more groups on a defragmenter that still holds the first batch's unfinished lists."""
    p = Pair(parser)
    h, e = p.feed(random_frames(41, 300), what="batch 1")
    assert set(h.outcomes["what"]) == {RR.FILED, RR.COMPLETE, RR.REJECTED, RR.HOLE, RR.INVALID}
    assert (h.dgrams["flags"] & RR.D_SHORT_SLICE).any() and (h.dgrams["ihl"] > 5).any()
    assert (h.dgrams["payload_len"] != h.dgrams["length"]).any() and p.ref.stats()["lists"] > 20
    assert len(h.dgrams) > 150
    p.feed(random_frames(42, 100), what="batch 2")  # the same keys again: carried lists meet new fragments
    p.close()


@pytest.mark.parametrize("n", [255, 256])
def test_sort_pass_count_step(parser, n):
    """A fresh defragmenter (no carried lists, so the sort's items are the n records) with 255 and
    with 256 records: gpd_radix_sort.h's sort_passes(n) goes from 1 (the last pass alone, with
    reassembly's sink) to 2 (a leading pass, then the last).  Datagrams of 2 and 3 fragments under
    distinct keys, every fifth without its last fragment, interleaved."""
    rng = np.random.default_rng(70 + n)
    groups, left = [], n
    while left:
        k = len(groups)
        g = in_order(rng, 2 + k % 2, hi=3)
        g = g[:min(len(g) - (k % 5 == 4), left)]
        groups.append(frames_of(rng, g, key_of(k)))
        left -= len(g)
    p = Pair(parser)
    h, e = p.feed(interleave(rng, groups))
    assert len(h.outcomes) == n and set(h.outcomes["what"]) == {RR.FILED, RR.COMPLETE}
    assert set(h.dgrams["nfrags"]) == {2, 3} and len(h.dgrams) > 60
    assert p.dev.stats()["lists"] >= len(groups) // 5
    p.close()


# ---------------------------------------------------------------- 3. the in-order run's edges
def _eights(n, first=0, last_mf=False):
    return [spec(8 * k, 8, last_mf or k != n - 1) for k in range(first, n)]


def test_in_order_run_lengths(parser):
    """Datagrams of 2, 63, 64, 65 and 129 in-order fragments, each key alone and all interleaved."""
    rng = np.random.default_rng(5)
    groups = [frames_of(rng, in_order(rng, n, hi=3), key_of(k)) for k, n in enumerate((2, 63, 64, 65, 129))]
    p = Pair(parser)
    h, _ = p.feed([f for g in groups for f in g], what="alone")
    assert list(h.dgrams["nfrags"]) == [2, 63, 64, 65, 129]
    h, _ = p.feed(interleave(rng, groups), what="interleaved")
    assert sorted(h.dgrams["nfrags"]) == [2, 63, 64, 65, 129] and p.ref.stats()["lists"] == 0
    p.close()


@pytest.mark.parametrize("b", [0, 1, 63])
def test_in_order_run_broken(parser, b):
    """A run of b in-order fragments, then the record that breaks it: a gap (the next fragment
    but one), a duplicate, an overlap, and an early MF=0 in a datagram whose first fragment comes
    last; the datagrams go on in order behind the break."""
    rng = np.random.default_rng(60 + b)
    n = 70
    base = _eights(n)
    gap = base[:b] + [base[b + 1], base[b]] + base[b + 2:]
    dup = base[:b] + [dict(base[max(b - 1, 0)])] + base[b:] if b else [base[0], dict(base[0])] + base[1:]
    over = base[:b] + [spec(max(8 * b - 8, 0), 16, True)] + base[b:]
    early = _eights(n, first=1)
    early[b] = dict(early[b], mf=False)
    early.append(base[0])
    groups = [frames_of(rng, g, key_of(k)) for k, g in enumerate((gap, dup, over, early))]
    p = Pair(parser)
    h, _ = p.feed([f for g in groups for f in g], what="alone")
    assert RR.COMPLETE in set(h.outcomes["what"])
    p.feed(interleave(rng, groups), what="interleaved")
    p.close()


def test_in_order_run_to_the_last_offset(parser):
    """8,184 eight-byte fragments in order up to FragOffset 8183, the last one 100 bytes long:
    Highest + Length-20 passes 65535 there and the uint16 sum wraps."""
    rng = np.random.default_rng(7)
    g = [spec(8 * k, 8, True) for k in range(8183)] + [spec(8 * 8183, 100, False)]
    p = Pair(parser)
    h, e = p.feed(frames_of(rng, g, key_of(0)))
    assert set(h.outcomes["what"]) == {RR.FILED} and p.ref.stats()["fragments"] == 8184
    fl = next(iter(p.ref.d.ip_flows.values()))
    assert (fl.highest, fl.current) == (65464, 28)
    h, e = p.feed(frames_of(rng, [spec(0, 8, True)], key_of(0)), what="a duplicate afterwards")
    assert list(h.outcomes["what"]) == [RR.FILED]
    p.close()


# ---------------------------------------------------------------- 4. the length limit
def test_list_length_limit(parser):
    """The MaxSize shape: one key, 8,193 fragments at offset 8183 whose end wraps, so each is a
    PushBack.  The 8,192nd flushes the list (LIST_FULL); the 8,193rd starts the key afresh."""
    f = ip4_frame(120, 1, 8183, 77, src=(1, 1, 1, 1), dst=(2, 2, 2, 2))
    p = Pair(parser)
    h, _ = p.feed([f] * 8193)
    assert list(h.outcomes["what"]) == [RR.FILED] * 8191 + [RR.LIST_FULL, RR.FILED]
    assert p.dev.stats() == {"lists": 1, "fragments": 1, "bytes": 100}
    p.close()


# ---------------------------------------------------------------- 5. the carry
def test_carry_over_three_batches(parser):
    """One datagram split over three batches, out of order, the device buffers of each batch
    overwritten after its call; a second key's list is carried untouched through the middle batch."""
    rng = np.random.default_rng(8)
    g = in_order(rng, 9, hi=20)
    fa = frames_of(rng, [g[i] for i in (3, 0, 8, 5, 1, 2, 7, 4, 6)], key_of(0))
    fb = frames_of(rng, in_order(rng, 4), key_of(1))
    p = Pair(parser)
    p.feed(fa[:3] + fb[:2], scrub=True, what="batch 1")
    assert p.dev.stats()["lists"] == 2 and p.dev.stats()["fragments"] == 5
    p.feed(fa[3:6], scrub=True, what="batch 2")
    h, e = p.feed(fa[6:] + fb[2:], scrub=True, what="batch 3")
    assert list(h.dgrams["nfrags"]) == [9, 4] and p.dev.stats()["lists"] == 0
    p.close()


@pytest.mark.parametrize("with_ts", [False, True])
def test_discard_between_batches(parser, with_ts):
    """DiscardOlderThan between batches: LastSeen is the last stored fragment's timestamp (ts_ns)
    or the call's now_ns; a discarded key starts afresh, a kept one completes."""
    rng = np.random.default_rng(9)
    groups = [frames_of(rng, in_order(rng, 4), key_of(k)) for k in range(6)]
    first = [f for g in groups for f in g[:2]]
    p = Pair(parser)
    ts = [1000 + 10 * k for k in range(len(first))] if with_ts else None
    p.feed(first, ts=ts, now=1055)
    t = 1055 if with_ts else 1056
    want = p.ref.discard(t)
    assert p.dev.DiscardOlderThan(t) == want and want == (3 if with_ts else 6)
    assert p.dev.stats() == p.ref.stats()
    assert p.dev.DiscardOlderThan(t) == 0
    rest = [f for g in groups for f in g[2:]]
    h, _ = p.feed(rest, ts=None if ts is None else [2000 + k for k in range(len(rest))], now=2000)
    assert len(h.dgrams) == 6 - want
    assert p.dev.DiscardOlderThan(1 << 62) == p.ref.discard(1 << 62) and p.dev.stats()["lists"] == 0
    p.close()


# ---------------------------------------------------------------- 6. the gather
def test_gather_alignments_and_short_pieces(parser):
    """Packets laid out without alignment, payloads and slices of 1 to 15 bytes (truncated
    captures and the quirk's Payload[startAt:]), datagrams back to back: every source and every
    output alignment 0-15 occurs.  A buffer with sentinels behind out[2] keeps them."""
    import torch
    from gopacket_amd import ip4reasm as I
    rng = np.random.default_rng(10)
    groups = []
    for k in range(96):
        r = k % 16
        if k % 3 == 0:  # a truncated middle fragment: r payload bytes
            g = in_order(rng, 3, hi=3, tail=8 + r)
            g[1]["cap"] = 14 + 20 + r
        elif k % 3 == 1:  # the quirk's slice: the overlapping fragment keeps r bytes past startAt
            g = quirk_complete(2, cap=14 + 20 + 16 + r)
        else:
            g = in_order(rng, 2 + r % 3, hi=2, tail=8 + r)
        groups.append(frames_of(rng, g, key_of(k)))
    frames = interleave(rng, groups)
    p = Pair(parser)
    h, e = p.feed(frames, align=1)
    assert {int(o) % 16 for o in h.offset} == set(range(16))
    lens = {int(x) for x in e.dgrams["payload_len"]}
    assert len(h.dgrams) == 96 and len(lens) > 20
    # the raw call into a larger buffer of sentinels
    batch, db, out, cnt, recs = p.handoff(frames, align=1)
    assert {(int(batch.offset[int(r["packet"])]) + int(r["net_off"]) + 4 * int(r["ihl"])) % 16 for r in recs} == set(range(16))
    assert {int(r["payload_len"]) for r in recs} >= set(range(1, 16))
    e2 = p.ref.run(batch, recs)
    nb, nd = len(e2.bytes), len(e2.dgrams)
    byts = torch.full((nb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    oc = torch.empty(cnt * 8, dtype=torch.uint8, device="cuda")
    dg = torch.empty(nd * 32, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(2 * (nd + 16), dtype=torch.int32, device="cuda")
    m = (nd + 15) // 16 * 16
    rc, o4 = p.dev._run(db, out, cnt, None, 0, oc, dg, nd, desc[:m], desc[m:], byts, nb, torch.cuda.current_stream())
    assert rc == 0 and o4[:3] == (nd, cnt, nb)
    got = byts.cpu().numpy()
    assert np.array_equal(got[:nb], e2.bytes) and (got[nb:] == 0xA5).all()
    p.close()


# ---------------------------------------------------------------- 7. capacity
def test_capacity_sizing_and_records_only(parser):
    import torch
    from gopacket_amd import ip4reasm as I
    from gopacket_amd._lib import GpdError
    frames = random_frames(43, 60)
    p = Pair(parser)
    batch, db, out, cnt, recs = p.handoff(frames)
    # the sizing call: out[] only, nothing changes
    rc, o4 = p.dev._run(db, out, cnt, None, 0, None, None, 0, None, None, None, 0, torch.cuda.current_stream())
    probe = RR.RefDefragmenter().run(batch, recs)
    assert rc == 0 and (o4[0], o4[1], o4[2]) == (len(probe.dgrams), 0, len(probe.bytes))
    assert p.dev.stats() == {"lists": 0, "fragments": 0, "bytes": 0}
    # too small: refused, nothing written, state unchanged (the next call's result shows it)
    oc = torch.full((cnt * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    dg = torch.full((o4[0] * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    byts = torch.full((o4[2] + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    desc = torch.zeros(2 * (o4[0] + 16), dtype=torch.int32, device="cuda")
    m = (o4[0] + 15) // 16 * 16
    for md, mb in ((o4[0] - 1, o4[2]), (o4[0], o4[2] - 1)):
        rc, o = p.dev._run(db, out, cnt, None, 0, oc, dg, md, desc[:m], desc[m:], byts, mb, torch.cuda.current_stream())
        assert rc != 0 and (o[0], o[1], o[2]) == (o4[0], 0, o4[2])
        assert (oc.cpu().numpy() == 0xA5).all() and (dg.cpu().numpy() == 0xA5).all() and (byts.cpu().numpy() == 0xA5).all()
        assert p.dev.stats() == {"lists": 0, "fragments": 0, "bytes": 0}
    with pytest.raises(GpdError):
        p.dev.DefragBatch(db, out, cnt, max_dgrams=1)
    p.feed(frames, what="after the refused calls")
    # records only
    p2 = Pair(parser)
    h, e = p2.feed(frames, gather=False, what="records only")
    assert h.bytes is None and len(h.dgrams) == len(e.dgrams) > 10
    p2.feed(random_frames(44, 30), what="gather after records only")
    p.close()
    p2.close()


def test_empty_fragment_free_and_scratch_reuse(parser):
    """An empty batch, a fragment-free one, and a large call followed by a small one."""
    p = Pair(parser)
    p.feed(frames_of(np.random.default_rng(1), in_order(np.random.default_rng(1), 3)[:2], key_of(0)))
    h, _ = p.feed([])
    assert len(h.outcomes) == 0 and p.dev.stats()["lists"] == 1
    b = synth.make_udp64(2000)
    h, _ = p.feed([b.packet(i) for i in range(b.n)])
    assert len(h.outcomes) == 0 and p.dev.stats()["lists"] == 1
    p.feed(random_frames(45, 250), what="large")
    p.feed(random_frames(46, 3), what="small")
    p.close()


def test_out_of_order_handoff_is_refused(parser):
    from gopacket_amd._lib import GpdError
    p = Pair(parser)
    rng = np.random.default_rng(2)
    batch, db, out, cnt, recs = p.handoff(frames_of(rng, in_order(rng, 4), key_of(0)))
    import torch
    swapped = torch.cat([out[32:64], out[:32], out[64:]])
    with pytest.raises(GpdError):
        p.dev.DefragBatch(db, swapped, cnt)
    assert p.dev.stats()["lists"] == 0
    p.close()


# ---------------------------------------------------------------- 8. the pipeline
A4, B4 = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])


def _fragment(frame, ident, sizes):
    """An Ethernet/IPv4 frame's datagram cut into fragments of the given payload sizes (the last
    takes the rest)."""
    eth, ip = frame[:14], frame[14:]
    total = struct.unpack(">H", ip[2:4])[0]
    payload, out, off = ip[20:total], [], 0
    cuts = list(sizes) + [len(payload)]
    for c in cuts:
        if 0 < len(payload) - (off + c) < 8:  # (securityChecks rejects a fragment under 8 bytes)
            c = len(payload) - off
        part = payload[off:off + c]
        if not part:
            break
        mf = off + len(part) < len(payload)
        h = bytearray(ip[:20])
        h[2:4] = struct.pack(">H", 20 + len(part))
        h[4:6] = struct.pack(">H", ident)
        h[6:8] = struct.pack(">H", (0x2000 if mf else 0) | (off // 8))
        h[10:12] = b"\0\0"
        h[10:12] = struct.pack(">H", RR.ip_checksum(bytes(h)))
        out.append(eth + bytes(h) + part)
        off += len(part)
    return out


def _stream_view(S, res):
    """Per stream: (its bytes, [(len, skip, flags)]), sorted: flow ids differ between tables."""
    h = S.streams_to_host(res)
    out = []
    for s in h.streams:
        recs = h.recs[int(s["first_rec"]):int(s["first_rec"]) + int(s["nrec"])]
        out.append((h.bytes[int(s["byte_off"]):int(s["byte_off"]) + int(s["nbytes"])].tobytes(),
                    [(int(r["len"]), int(r["skip"]), int(r["flags"])) for r in recs], int(s["completed"])))
    return sorted(out)


def test_pipeline_fragmented_tcp_reaches_the_streams(parser):
    """Four TCP connections whose segments arrive IP-fragmented and out of order among
    unfragmented TCP and UDP traffic: decode -> IPv4Fragments -> DefragBatch -> decode of the
    datagram batch (first layer IPv4) == the oracle decode of the same bytes; then flow table ->
    TCPSegments -> TCPStreams on the datagram batch gives the streams of the same conversations
    sent unfragmented."""
    import torch
    from gopacket_amd import ip4reasm as I
    from gopacket_amd import parser as P
    from gopacket_amd import tcpassembly as T
    from gopacket_amd import tcpstream as S
    from gopacket_amd.flows import NewFlowTable
    rng = np.random.default_rng(12)
    whole, frag_groups, ident, sent = {}, [], 100, []
    for c in range(4):
        seq = 1000 * (c + 1)
        segs = [(seq, 0x02, b"")]  # SYN
        seq += 1
        for _ in range(5):
            pay = rng.bytes(int(rng.integers(200, 1400)))
            segs.append((seq, 0x18, pay))
            seq += len(pay)
        segs.append((seq, 0x11, b""))  # FIN
        sent.append(b"".join(pay for _, _, pay in segs))
        frames = []
        for s, fl, pay in segs:
            f = synth.tcp_frame(A4, B4, 5000 + c, 80, s, ack=1, flags=fl, payload=pay)
            if pay:
                ident += 1
                whole[ident] = f
                parts = _fragment(f, ident, [8 * int(rng.integers(3, 40)) for _ in range(3)])
                frames += [parts[i] for i in rng.permutation(len(parts))]
            else:
                frames.append(f)  # SYN and FIN travel whole
        frag_groups.append(frames)
    udp = synth.make_udp64(40)
    noise = [udp.packet(i) for i in range(udp.n)] + [
        synth.tcp_frame(A4, B4, 6000, 443, 50 + 10 * k, ack=1, flags=0x18, payload=rng.bytes(10)) for k in range(8)]
    frames = interleave(rng, frag_groups + [noise])
    p = Pair(parser)
    batch, db, out, cnt, recs = p.handoff(frames)
    assert cnt > 40
    res = p.dev.DefragBatch(db, out, cnt)
    h = I.defrag_to_host(res)
    e = p.ref.run(batch, recs)
    same(res, h, e)
    assert res.ndgrams == 20 and p.dev.stats()["lists"] == 0
    # every datagram is the unfragmented segment's IPv4 datagram, but for Id, the DF flag and the checksum
    for g, o, ln in zip(h.dgrams, h.offset, h.caplen):
        b = h.bytes[int(o):int(o) + int(ln)].tobytes()
        w = whole[int(g["id"])][14:]
        assert b[:4] == w[:4] and b[12:] == w[12:] and b[8:10] == w[8:10] and RR.ip_checksum(b[:20]) == 0
    # the datagram batch through the parser, first layer IPv4, against the oracle decode
    p4 = P.NewDecodingLayerParser(L.LayerTypeIPv4)
    p4._mask = ALL
    dr = P.DeviceResult(res.batch.n, 0)
    p4.decode_device(res.batch, dr)
    torch.cuda.synchronize()
    hb = PacketBatch.from_arrays(h.bytes, h.offset, h.caplen, data_len=len(h.bytes))
    want = O.decode(hb, L.LayerTypeIPv4, ALL, 0, ext=False)
    got = dr.to_host()
    for f in ("status", "layers", "net_hash", "tp_hash", "csum", "hdr_off"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert all(got.decoded(i)[:2] == [L.LayerTypeIPv4, L.LayerTypeTCP] for i in range(res.batch.n))
    # flow table -> segments -> streams on the reassembled datagrams plus the segments that
    # travelled whole, against the same conversations unfragmented in the same order
    def streams_of(prs, dbatch):
        d = P.DeviceResult(dbatch.n, 0)
        prs.decode_device(dbatch, d)
        table = NewFlowTable(prs, 256)
        ids = table.Insert(dbatch, d)
        dsegs, dgroups, count, ngroups, ungrouped = T.TCPSegments(prs, dbatch, d, flow_id=ids, table=table)
        assert ungrouped == 0
        return S.TCPStreams(prs, dbatch, dsegs, dgroups, count, ngroups, close_all=True)
    # what the application sees after defragmentation, in arrival order: the unfragmented
    # packets of the batch and each datagram at its completing packet
    done = {int(g["packet"]): k for k, g in enumerate(h.dgrams)}
    frag_pk = {int(r["packet"]) for r in recs}
    seen_ip, seen_whole = [], []
    for i, f in enumerate(frames):
        if i in done:
            g = h.dgrams[done[i]]
            seen_ip.append(h.bytes[int(h.offset[done[i]]):int(h.offset[done[i]]) + int(h.caplen[done[i]])].tobytes())
            seen_whole.append(whole[int(g["id"])])
        elif i not in frag_pk and f[12:14] == b"\x08\x00" and f[23] == 6:
            seen_ip.append(f[14:])
            seen_whole.append(f)
    a = streams_of(p4, P.DeviceBatch(PacketBatch.from_packets(seen_ip), 0))
    b = streams_of(parser, P.DeviceBatch(PacketBatch.from_packets(seen_whole), 0))
    va, vb = _stream_view(S, a), _stream_view(S, b)
    assert va == vb and len(va) == 5
    assert set(sent) <= {x[0] for x in va}  # every fragmented conversation's bytes, whole and in order
    p.close()
