"""Every single-workgroup pass that loops over its input in fixed-size rounds and carries a running
total from one round to the next, driven into its second and third round: the ordered
compaction's block scan (gpd_compact.h compact_scan, as the fragment hand-off's, the segment
hand-off's, the stream builders' and the reassembler's scan kernels), the radix sort's
histogram scan, and the two writers' block-total scans with their backward pass.

With R the loop's items per round and B its block, every loop sees R (one full round, last
block full), R + 1 (a second round of one block of one item) and 2R + 3B + 5 (a third round, a
partial last block, a carry built from a carry); R and B are expressions of the kernels'
constants mirrored in tests/rounds_cases.py.  Every output word is compared with an expectation
computed off the device: the project's oracles on a small pool (or one period), expanded with
numpy.  Kept items lie at item 0 and n - 1, on both sides of a block edge and of both round
edges, in one block that is kept entirely, and around a whole round with nothing kept."""
import os
import sys

import numpy as np
import pytest

import oracle_ref as O
import pcapngwrite_ref as NR
import pcapwrite_ref as WR
import rounds_cases as RC
import tcpseg_ref as TS
from gopacket_amd import layers as L
from gopacket_amd import synth
from conftest import ROOT
from tcpseg_cases import ALL

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import defrag_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = ALL
    return p


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    yield
    for c in (_writer_cache, _seg_cache):
        c.clear()


def _one(cache, key, make):
    """The input for `key`, built once and kept until another key is asked for (one large input
    on the device at a time)."""
    if cache.get("key") != key:
        cache.clear()
        cache.update(key=key, value=make())
    return cache["value"]


def _same_bytes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{what}: first difference at byte {k} of {len(want)}: "
                             f"{got[k & ~15:(k & ~15) + 16].tobytes().hex()} != "
                             f"{want[k & ~15:(k & ~15) + 16].tobytes().hex()}")


def _same_records(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
        k = int(np.nonzero(got != want)[0][0])
        raise AssertionError((what, "record", k, got[max(k - 1, 0):k + 2], want[max(k - 1, 0):k + 2]))


# ---------------------------------------------------------------- 6. the writers
W_SIZES = RC.sizes(RC.WRITE_ROUND, RC.WRITE_BLOCK)
W_CASES = [(k, m) for k in (0, 1) for m in ("all", "edges")] + \
          [(2, m) for m in ("all", "round2", "first", "last", "edges", "gap", "bad")]
NG_PREFIX = (NR.section_block(b"amd64", b"linux", b"gopacket") + NR.interface_block(1, 0, b"intf0", os_=b"linux") +
             NR.interface_block(0, 96, b"lo", filter_=b"none", tsoffset=100) + NR.interface_block(1, 0, b"if2"))
_writer_cache = {}


class _WriterDev:
    def __init__(self, n):
        from gopacket_amd import parser as P
        from gopacket_amd.pcapwrite import _dev
        self.w = w = RC.WriterInput(n, 0x5EED0700 + n % 251)
        self.db = P.DeviceBatch(w.batch)
        d = lambda a, t: _dev(a, t, self.db.device, n, "input")
        self.ts, self.ts_raw = d(w.ts, np.uint64), d(w.ts_raw, np.uint64)
        self.length, self.length_bad = d(w.length, np.uint32), d(w.length_bad, np.uint32)
        self.ifindex = d(w.ifindex, np.uint32)


def _writer_input(k):
    return _one(_writer_cache, k, lambda: _WriterDev(W_SIZES[k]))


def _prove_writer_expectation(w, fmt, keep):
    """The numpy construction of the stream is the reference's loop, on the first 5,000 packets:
    under the case's own mask, under a dense one, and with a rejected packet."""
    k = 5000
    b = RC.prefix_batch(w.batch, k)
    dense = (np.random.default_rng(0x5EED0705).integers(0, 2, k) == 0).astype(np.uint8)
    good, short = w.length[:k].copy(), w.length[:k].copy()
    b.caplen[3000], good[3000], short[3000], dense[3000] = 9, 10, 8, 1
    for kp, ln in ((None if keep is None else keep[:k], good), (dense, good), (dense, short)):
        if fmt == "pcap":
            got, want = RC.pcap_stream(b, w.ts[:k], ln, kp, False, (65535, 1)), WR.write(b, w.ts[:k], ln, kp, False,
                                                                                         (65535, 1))
            assert RC.pcap_stream(b, w.ts[:k], None, kp, True)[0].tobytes() == WR.write(b, w.ts[:k], None, kp, True)[0]
        else:
            got = RC.ng_stream(b, w.ts_raw[:k], ln, w.ifindex[:k], 3, kp, NG_PREFIX)
            want = NR.write(b, w.ts_raw[:k], ln, w.ifindex[:k], 3, kp, NG_PREFIX)
            two = RC.ng_stream(b, w.ts_raw[:k], ln, w.ifindex[:k], 2, kp)  # interface 2 was not added
            assert (two[0].tobytes(),) + two[1:] == NR.write(b, w.ts_raw[:k], ln, w.ifindex[:k], 2, kp)
        assert (got[0].tobytes(),) + got[1:] == want
    assert want[2] == 3000


@pytest.mark.parametrize("k,mask,fmt", [(k, m, f) for k, m in W_CASES for f in ("pcap", "pcapng")])
def test_writer_block_totals_past_the_first_round(parser, k, mask, fmt):
    """scan_kernel (gpd_write_scan.h, both writers): the forward carries of positions and counts into the
    second and third chunk of 1024 block totals, and `mcarry`, the first kept packet of any later
    chunk, backwards ("round2": across two chunks; "last": from the stream's last packet).  "bad":
    a kept packet with length < capture length in the third round cuts the stream there."""
    from gopacket_amd import pcapwrite as PW
    from gopacket_amd.pcap import PcapError
    d = _writer_input(k)
    w, n, R = d.w, d.w.n, RC.WRITE_ROUND
    assert n == W_SIZES[k] and RC.rounds(n, R) == k + 1 and (k < 2 or n > 2 * R)
    keep = w.mask(mask)
    bad = mask == "bad"
    _prove_writer_expectation(w, fmt, keep)
    length, d_length = (w.length_bad, d.length_bad) if bad else (w.length, d.length)
    if fmt == "pcap":
        want, wn, wbad = RC.pcap_stream(w.batch, w.ts, length, keep, False, (65535, 1))
        call = lambda: PW.write_device(parser, d.db, d.ts, d_length, keep, file_header=(65535, 1))
    else:
        want, wn, wbad, why = RC.ng_stream(w.batch, w.ts_raw, length, w.ifindex, 3, keep, NG_PREFIX)
        call = lambda: PW.write_device_ng(parser, d.db, d.ts_raw, d_length, d.ifindex, 3, keep, NG_PREFIX)
    if bad:
        assert wbad == w.bad and wbad > 2 * R and wn > 3 * RC.WRITE_BLOCK
        with pytest.raises(PcapError) as e:
            call()
        stream, nw = e.value.stream, e.value.n_written
        assert e.value.bad_index == wbad and (fmt == "pcap" or e.value.bad_reason == NR.BAD_LENGTH)
    else:
        assert wbad == WR.NO_BAD
        stream, nw = call()
    assert nw == wn
    _same_bytes(stream.cpu().numpy(), want, (fmt, n, mask))
    if mask == "round2":
        first = int(np.nonzero(keep)[0][0])
        assert first >= 2 * R and nw == 4


# ---------------------------------------------------------------- 1. the IPv4 fragment hand-off
F_SIZES = RC.sizes(RC.COMPACT_ROUND, RC.COMPACT_BLOCK)
F_CASES = [(0, "edges", False), (1, "edges", False), (2, "edges", False), (2, "gap", False), (2, "edges", True)]


@pytest.fixture(scope="module")
def fragpool(parser):
    """The pool's frames and the defrag oracle's records of them (oracle/defrag_ref.py)."""
    from gopacket_amd.batch import PacketBatch
    frames, is_frag = RC.frag_pool()
    pb = PacketBatch.from_packets(frames)
    ref = O.decode(pb, L.LayerTypeEthernet, parser.decoders, parser.options, ext=True)
    recs = D.ip4_fragments(pb, ref)
    assert list(recs["packet"]) == list(np.nonzero(is_frag)[0])  # one record per fragment, none else
    assert set(recs["verdict"]) == {D.FRAG_INSERT, D.FRAG_TOO_SMALL, D.FRAG_OFFSET}
    return frames, is_frag, recs, ref


@pytest.mark.parametrize("k,variant,records", F_CASES)
def test_fragment_hand_off_past_the_first_round(parser, fragpool, k, variant, records):
    """frag_scan_kernel (compact_scan over the block counts of frag_count_kernel): the carry into
    the second and third round of 1024 blocks; every record against the defrag oracle's record of
    its pool frame.  The decode the hand-off reads is checked against the C oracle on the whole
    batch, so a difference is the hand-off's."""
    import torch
    from gopacket_amd import defrag as DF
    from gopacket_amd import parser as P
    frames, is_frag, pool_recs, _ = fragpool
    n, R, B = F_SIZES[k], RC.COMPACT_ROUND, RC.COMPACT_BLOCK
    assert RC.rounds((n + B - 1) // B, 1024) == k + 1 and (k < 2 or n > 2 * R)
    kept = RC.place(n, R, B, variant, 0x5EED0710 + k)
    idx = RC.frag_index(kept, is_frag, 0x5EED0711 + k)
    batch = RC.tile_frames(frames, idx)
    want = RC.expand_by_packet(pool_recs, len(frames), idx)
    assert np.array_equal(want["packet"], np.nonzero(kept)[0])
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(n, 0, records=records)
    parser.decode_device(db, dr)
    out, cnt = DF.IPv4Fragments(parser, db, dr)
    torch.cuda.synchronize()
    assert cnt == len(want)
    _same_records(DF.fragments_to_host(out, cnt), want, (n, variant, records))
    if not records:
        ref = O.decode(batch, L.LayerTypeEthernet, parser.decoders, parser.options, ext=False, nthreads=8)
        host = dr.to_host()
        for f in ("status", "layers", "hdr_off"):
            assert np.array_equal(getattr(host, f), getattr(ref, f)), f


# ---------------------------------------------------------------- 2. the TCP segment hand-off
S_SIZES = RC.sizes(RC.SORT_ROUND, RC.SORT_TILE) + RC.sizes(RC.COMPACT_ROUND, RC.COMPACT_BLOCK)
# (size, ids, id_bound): 1, 2, 3 and 4 passes of the sort (sort_passes: ceil(bitlen(bound) / 8))
S_CASES = [(0, "hot", 200), (0, "distinct", 1 << 20), (1, "hot", 60000), (1, "distinct", 1 << 20),
           (2, "hot", 1 << 20), (2, "distinct", 1 << 24),
           (3, "hot", 200), (3, "distinct", 1 << 24), (4, "hot", 1 << 24), (4, "distinct", 1 << 24),
           (5, "hot", 60000), (5, "distinct", 1 << 24)]
_seg_cache = {}


@pytest.fixture(scope="module")
def segpool(parser):
    pool = synth.make_tcp64(256)
    ref = O.decode(pool, L.LayerTypeEthernet, parser.decoders, parser.options, ext=True)
    recs = TS.segments(pool, ref)
    assert list(recs["packet"]) == list(range(256))  # every frame is handed over
    return [pool.packet(i) for i in range(256)], recs


def _seg_input(parser, segpool, k):
    def make():
        from gopacket_amd import parser as P
        frames, pool_recs = segpool
        n = S_SIZES[k]
        idx = np.random.default_rng(0x5EED0720 + k).integers(0, len(frames), n)
        idx[:len(frames)] = np.arange(len(frames))
        batch = RC.tile_frames(frames, idx)
        base = RC.expand_by_packet(pool_recs, len(frames), idx)
        db = P.DeviceBatch(batch, 0)
        dr = P.DeviceResult(n, 0)
        parser.decode_device(db, dr)
        return db, dr, base
    return _one(_seg_cache, k, make)


@pytest.mark.parametrize("k,ids,bound", S_CASES)
def test_segment_hand_off_past_the_first_round(parser, segpool, k, ids, bound):
    """Every packet is a handed-over segment, so the packet scan (ts_scan_kernel), the sort
    (sort_scan_kernel, a round = 64 tiles' counts of hist[256][ntile]) and the head scan
    (ts_scan_kernel again, over the sorted keys' head flags) all see n: the sort scan's rounds at
    the first three sizes, compact_scan's at the last three.  "distinct" makes more groups than a
    round has items (ts_index_kernel and ts_group_kernel past it); bound 2^24 takes four passes."""
    import torch
    from gopacket_amd import tcpassembly as T
    db, dr, base = _seg_input(parser, segpool, k)
    n = S_SIZES[k]
    assert len(base) == n and T.SORT_TILE == RC.SORT_TILE
    if k < 3:
        assert RC.rounds(256 * ((n + RC.SORT_TILE - 1) // RC.SORT_TILE), 16384) == k + 1
        assert k < 2 or n > 2 * RC.SORT_ROUND
    else:
        assert RC.rounds((n + RC.COMPACT_BLOCK - 1) // RC.COMPACT_BLOCK, 1024) == k - 2
        assert k < 5 or n > 2 * RC.COMPACT_ROUND
    fid = RC.flow_ids(ids, n, bound, 0x5EED0730 + k)
    s = base.copy()
    s["flow_id"] = fid
    ws, wg, wun = TS.group(s, bound)
    assert wun > 0 and (ids != "distinct" or len(wg) > n - 100)
    if k == 5 and ids == "distinct":
        assert len(wg) > 2 * RC.COMPACT_ROUND
    d_fid = torch.from_numpy(fid.view(np.int32)).cuda()
    segs, groups, cnt, ng, un = T.TCPSegments(parser, db, dr, flow_id=d_fid, id_bound=bound)
    assert (cnt, ng, un) == (n, len(wg), wun)
    _same_records(T.segments_to_host(segs, cnt), ws, (n, ids, bound, "segs"))
    _same_records(T.groups_to_host(groups, ng), wg, (n, ids, bound, "groups"))
    if ids == "hot":  # and in packet order, ungrouped: the packet scan alone
        segs, _, cnt, ng, un = T.TCPSegments(parser, db, dr)
        assert (cnt, ng, un) == (n, 0, 0)
        _same_records(T.segments_to_host(segs, cnt), base, (n, "packet order"))


# ---------------------------------------------------------------- 3. stream assembly
def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


A_SIZES = RC.sizes(RC.COMPACT_ROUND, RC.COMPACT_BLOCK)
A_OPTS = {"long": dict(max_pages=4, close_all=False), "short": dict(max_pages=0, close_all=True)}


@pytest.fixture(scope="module")
def stream_periods():
    """Per shape: the period's hand-off and the oracle's output for it (tests/tcpstream_ref.py)."""
    import tcpstream_ref as SR
    out = {}
    for shape, seed in (("long", 0x5EED0740), ("short", 0x5EED0741)):
        batch, segs, groups, main = RC.stream_period(shape, seed, 64 if shape == "long" else 256)
        e = SR.assemble(segs, groups, batch.packet, **A_OPTS[shape])
        assert e.nstreams == main + 1
        out[shape] = (batch, segs, groups, main, e)
    return out


@pytest.mark.parametrize("shape,k", [(s, k) for s in ("long", "short") for k in range(3)])
def test_stream_assembly_past_the_first_round(parser, stream_periods, shape, k):
    """ta_scan_kernel (compact_scan over the block sums of the page counts per segment, then of
    three per-group arrays at stride nblk + 1).  "long": connections of up to 200 segments, the
    segments at R, R + 1 and 2R + 3B + 5 (the page scan's rounds); "short": one or two segments a
    connection, the groups at those sizes (the group scans' rounds, and the segments beyond
    them).  Records, streams, bytes and the four result words against the oracle's, tiled."""
    from gopacket_amd import parser as P
    from gopacket_amd import tcpstream as S
    batch, segs, groups, main, e = stream_periods[shape]
    n, R, B = A_SIZES[k], RC.COMPACT_ROUND, RC.COMPACT_BLOCK
    per = int(groups["start"][main]) if shape == "long" else main  # the main part's segments / groups
    reps, unit = n // per, n % per
    tsegs, tgroups = RC.tile_hand_off(segs, groups, main, reps, unit)
    items = len(tsegs) if shape == "long" else len(tgroups)
    assert items == n and RC.rounds((n + B - 1) // B, 1024) == k + 1 and (k < 2 or n > 2 * R)
    assert shape == "short" or len(tgroups) < R
    wrecs, wstreams, wbytes = RC.tile_streams(e.recs, e.streams, e.bytes, main, reps, unit)
    assert len(set(e.recs["len"] // S.PAGE_BYTES)) > 1 if shape == "long" else (e.recs["len"] > S.PAGE_BYTES).any()
    res = S.TCPStreams(parser, P.DeviceBatch(batch, 0), _up(tsegs), _up(tgroups), len(tsegs), len(tgroups),
                       max_pages_per_connection=A_OPTS[shape]["max_pages"], close_all=A_OPTS[shape]["close_all"])
    assert (res.nrecs, res.nstreams, res.nbytes, res.ncalls) == \
        (len(wrecs), len(wstreams), len(wbytes), int(wstreams["ncalls"].sum()))
    h = S.streams_to_host(res)
    _same_records(h.recs, wrecs, (shape, n, "recs"))
    _same_records(h.streams, wstreams, (shape, n, "streams"))
    _same_bytes(h.bytes, wbytes, (shape, n))


# ---------------------------------------------------------------- 5. the stateful assembler
@pytest.fixture(scope="module")
def asm_periods():
    """The period's two runs and the oracle's output after each (tests/tcpasm_ref.py)."""
    import tcpasm_ref as AR
    (b1, s1, g1), (b2, s2, g2), main = RC.asm_period(0x5EED0750)
    ts1 = 1000 + 10 * np.arange(b1.n, dtype=np.int64)
    ts2 = 100000 + 10 * np.arange(b2.n, dtype=np.int64)
    model = AR.Model(main + 1)
    e1 = model.run(s1, g1, b1.packet, ts=ts1)
    e2 = model.run(s2, g2, b2.packet, ts=ts2)
    assert e1.out[1] == e2.out[1] == main + 1  # a stream per connection in both runs: no extra items
    assert e1.stats["pages"] > main * 3 // 4 and (e2.recs["flags"] & AR.R_CARRIED).any() and e2.stats["pages"] > 0
    return ((b1, s1, g1, ts1, e1), (b2, s2, g2, ts2, e2)), main, model


@pytest.mark.parametrize("k", range(3))
def test_stateful_assembler_past_the_first_round(parser, asm_periods, k):
    """tam_scan_kernel over the segments' page counts, the connection table's select mask
    (id_bound blocks) and the items' arrays, with R, R + 1 and 2R + 3B + 5 connections: run 1
    leaves an out-of-order page in most connections, run 2 fills the gaps, so the carry gather
    moves a store that was built past the round (at the third size it holds more pages than a
    round has items).  Everything the run returns, conns() and stats()
    against the oracle's, tiled, after each run."""
    import torch
    from gopacket_amd import parser as P
    from gopacket_amd import tcpasm as M
    runs, main, model = asm_periods
    n, R, B = A_SIZES[k], RC.COMPACT_ROUND, RC.COMPACT_BLOCK
    reps, unit = n // main, n % main
    assert RC.rounds((n + B - 1) // B, 1024) == k + 1 and (k < 2 or n > 2 * R)
    asm = M.NewAssembler(parser, n, 0)
    try:
        for run, (batch, segs, groups, ts, e) in enumerate(runs):
            tsegs, tgroups = RC.tile_hand_off(segs, groups, main, reps, unit)
            assert len(tgroups) == n
            wrecs, wstreams, wbytes, wseen = RC.tile_streams(e.recs, e.streams, e.bytes, main, reps, unit,
                                                             per_rec=(e.seen_ns,))
            wconns = RC.tile_by_id(e.conns, main, reps, unit)
            wstats = model.stats(wconns)
            assert run or k < 2 or wstats["pages"] > R  # (the store itself is larger than a round at the third size)
            res = asm.AssembleBatch(P.DeviceBatch(batch, 0), _up(tsegs), _up(tgroups), len(tsegs), len(tgroups),
                                    ts=torch.from_numpy(ts).cuda())
            got = (res.nrecs, res.nstreams, res.nbytes, res.ncalls, res.connections, res.pages, res.page_bytes)
            assert got == (len(wrecs), n, len(wbytes), int(wstreams["ncalls"].sum()), wstats["connections"],
                           wstats["pages"], wstats["page_bytes"]), run
            h = M.to_host(res)
            _same_records(h.recs, wrecs, (n, run, "recs"))
            assert np.array_equal(h.seen_ns, wseen), (n, run, "seen")
            _same_records(h.streams, wstreams, (n, run, "streams"))
            _same_bytes(h.bytes, wbytes, (n, run))
            _same_records(asm.conns(), wconns, (n, run, "conns"))
            assert asm.stats() == wstats, (n, run)
            del res, h
    finally:
        asm.close()


# ---------------------------------------------------------------- 4. the IPv4 reassembly
I_SIZES = RC.sizes(RC.SORT_ROUND, RC.SORT_TILE) + RC.sizes(RC.COMPACT_ROUND, RC.COMPACT_BLOCK)


@pytest.fixture(scope="module")
def reasm_periods(parser):
    """The period's two calls and the unit: frames, the defrag oracle's hand-off records, and the
    reassembly oracle's result and stats after each (tests/ip4reasm_ref.py)."""
    import ip4reasm_ref as RR
    from gopacket_amd.batch import PacketBatch
    out = []
    ref = RR.RefDefragmenter()
    for frames, r in zip(RC.reasm_period(0x5EED0770), (ref, ref, RR.RefDefragmenter())):
        b = PacketBatch.from_packets(frames)
        recs = D.ip4_fragments(b, O.decode(b, L.LayerTypeEthernet, parser.decoders, parser.options, ext=True))
        e = r.run(b, recs)
        out.append((frames, recs, e, r.stats()))
    (_, _, e1, st1), (_, _, e2, st2), (_, _, eu, stu) = out
    assert len(e1.dgrams) >= 8 and st1["lists"] >= 20 and len(e2.dgrams) == st1["lists"] and stu["lists"] == 1
    assert set(e1.outcomes["what"]) == {RR.FILED, RR.COMPLETE, RR.REJECTED}
    return out


@pytest.mark.parametrize("k", range(6))
def test_reassembly_past_the_first_round(parser, reasm_periods, k):
    """sort_scan_kernel (gpd_radix_sort.h, the sort's histogram scan over M = carried lists +
    records: a round is 64 tiles) at the first three sizes, ir_scan_kernel (compact_scan over the
    head flags of the M items, then the records' and the groups' block sums, three arrays each) at
    the last three.
    Call 1 takes n records of datagrams of 2, 3 and 8 fragments, every replica under a key of its
    own, and leaves three lists in four carried; call 2 completes the lists of the first, a middle
    and the last replica from a store that was built past the round, with M = the carried lists
    + its records.  Outcomes, datagram records, offsets, lengths, bytes and stats() against the
    oracle's, tiled."""
    n = I_SIZES[k]
    if k < 3:
        assert RC.rounds(256 * ((n + RC.SORT_TILE - 1) // RC.SORT_TILE), 16384) == k + 1
        assert k < 2 or n > 2 * RC.SORT_ROUND
    else:
        assert RC.rounds((n + RC.COMPACT_BLOCK - 1) // RC.COMPACT_BLOCK, 1024) == k - 2
        assert k < 5 or n > 2 * RC.COMPACT_ROUND
    _reasm_two_calls(parser, reasm_periods, n, k)


@pytest.mark.parametrize("n", [65535, 65536])
def test_reassembly_at_the_three_pass_step(parser, reasm_periods, n):
    """The same two calls on a fresh defragmenter at M = 65,535 and 65,536 items, where the sort's
    keys [0, M] go from 16 to 17 bits: two passes (one leading pass and the last) become three.
    Every size of test_reassembly_past_the_first_round lies above the step (M >= 524,288 in call 1
    and more than 65,536 carried lists in call 2: three passes); the one- and two-pass sorts are
    test_ip4reasm_gpu.py's (255, 256, 8,184 and 8,193 records)."""
    _reasm_two_calls(parser, reasm_periods, n, None)


def _reasm_two_calls(parser, reasm_periods, n, k):
    from gopacket_amd import ip4reasm as I
    from gopacket_amd import parser as P
    (f1, r1, e1, st1), (f2, r2, e2, st2), (fu, ru, eu, stu) = reasm_periods
    reps, unit = n // len(f1), n % len(f1)
    main_ids, unit_ids = np.arange(reps), reps + np.arange(unit)
    dev = I.NewIPv4Defragmenter(parser)
    try:
        batch, recs = RC.reasm_input([(f1, r1, main_ids), (fu, ru, unit_ids)])
        assert batch.n == len(recs) == n
        want = RC.reasm_expected([(e1, len(f1), main_ids), (eu, len(fu), unit_ids)])
        res = dev.DefragBatch(P.DeviceBatch(batch, 0), _up(recs), n)
        stats = {f: reps * st1[f] + unit * stu[f] for f in st1}
        _same_reasm(I, res, want, stats, dev, (n, "call 1"))
        assert res.nlists > n // 8 and (k != 5 or res.nlists > RC.SORT_ROUND)
        del res
        some = np.unique([0, reps // 2, reps - 1])
        batch, recs = RC.reasm_input([(f2, r2, some)])
        want = RC.reasm_expected([(e2, len(f2), some)])
        res = dev.DefragBatch(P.DeviceBatch(batch, 0), _up(recs), len(recs))
        stats = {f: (reps - len(some)) * st1[f] + len(some) * st2[f] + unit * stu[f] for f in st1}
        _same_reasm(I, res, want, stats, dev, (n, "call 2"))
    finally:
        dev.close()


def _same_reasm(I, res, want, stats, dev, what):
    outcomes, dgrams, offset, caplen, byts = want
    assert (res.ndgrams, res.noutcomes, res.nbytes, res.nlists) == (len(dgrams), len(outcomes), len(byts),
                                                                    stats["lists"]), what
    h = I.defrag_to_host(res)
    _same_records(h.outcomes, outcomes, (what, "outcomes"))
    _same_records(h.dgrams, dgrams, (what, "dgrams"))
    assert np.array_equal(h.offset, offset) and np.array_equal(h.caplen, caplen), what
    _same_bytes(h.bytes, byts, what)
    assert dev.stats() == stats, what
