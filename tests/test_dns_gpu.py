"""The DNS decode on the GPU (gpd_dns_decode, include/gpd_dns.h): message records, entries and
names compared byte for byte with the model (tests/dns_ref.py) over the candidates and payloads
the CPU oracle finds, and `messages()` against the model's objects."""
import numpy as np
import pytest

import dns_cases as DC
import dns_ref as R
import oracle_ref as O
from gopacket_amd import layers as L
from gopacket_amd.batch import PAD, PacketBatch

pytestmark = pytest.mark.gpu

ALL = 0xFFF


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = ALL
    return p


def _decode(parser, batch, records=False):
    from gopacket_amd import parser as P
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(batch.n, 0, records=records)
    parser.decode_device(db, dr)
    return db, dr


def _oracle(batch, parser, first=L.LayerTypeEthernet):
    return O.decode(batch, first, parser.decoders, parser.options, ext=True, nthreads=8)


def _check(parser, frames, records=False, max_work=4096, first=L.LayerTypeEthernet, objects=True):
    """Decode the frames, run DecodeDNS and compare everything with the model; returns (result,
    host msgs, the model's (data, DNS) pairs)."""
    from gopacket_amd import dns as D
    batch = PacketBatch.from_packets(frames)
    db, dr = _decode(parser, batch, records)
    res = D.DecodeDNS(parser, db, dr, max_work=max_work)
    wm, we, wn, models = DC.expect(batch, _oracle(batch, parser, first), max_work)
    gm, ge, gn = res.to_host()
    assert res.count == len(wm) and res.n_entries == len(we) and res.name_bytes == len(wn)
    for k in range(len(wm)):
        assert gm[k:k + 1].tobytes() == wm[k:k + 1].tobytes(), (k, gm[k], wm[k])
    assert ge.tobytes() == we.tobytes()
    assert gn == wn
    assert res.deferred == int((wm["verdict"] == R.DEFERRED).sum())
    if objects:
        objs = res.messages()
        assert len(objs) == len(models)
        for o, m, (data, d) in zip(objs, wm, models):
            assert o.packet == int(m["packet"])
            DC.same_object(o, d)
    return res, gm, models


ALL_MESSAGES = [m for _, m in DC.vector_messages()] + list(DC.named_cases().values())


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("encap", list(DC.ENCAPS))
def test_vectors_and_cases_in_every_encapsulation(parser, encap, records):
    """The reference's vectors and every hand-built case as real frames, between non-DNS UDP and
    TCP, ARP, runts, empty port-53 packets and a cut UDP header, in both result forms."""
    frames = DC.interleave([DC.ENCAPS[encap](m) for m in ALL_MESSAGES])
    res, gm, models = _check(parser, frames, records)
    assert res.count == len(ALL_MESSAGES)  # none of the noise is a candidate, every message is
    assert [d for d, _ in models] == ALL_MESSAGES
    # every reachable verdict is seen, and nothing else; none is deferred at the default budget
    assert set(int(v) for v in gm["verdict"]) == R.REACHABLE
    assert res.deferred == 0


def test_udp_length_trims_the_message(parser):
    """udp.go:42-51: data ends where UDP Length says (shorter than the capture), Length 0 takes
    the rest, a Length past the capture is cut by the capture."""
    m = DC.named_cases()["sections"]
    frames = [DC.eth(DC.ip4(DC.udp(m, length=8 + k), 17)) for k in (1, 11, 12, 40, len(m) - 1, len(m))]
    frames += [DC.eth(DC.ip4(DC.udp(m, length=0), 17)), DC.eth(DC.ip4(DC.udp(m, length=len(m) + 100), 17)),
               DC.eth(DC.ip4(DC.udp(m) + b"trailer", 17, length=20 + 8 + len(m))) + b"pad"]
    res, gm, _ = _check(parser, frames)
    assert list(gm["data_len"]) == [1, 11, 12, 40, len(m) - 1, len(m), len(m), len(m), len(m)]
    assert (gm["data_off"] == 42).all()


def test_compressed_response_cut_at_every_length(parser):
    m = DC.compressed_response()
    frames = [DC.eth(DC.ip4(DC.udp(m[:k]), 17)) for k in range(1, len(m) + 1)]
    res, gm, _ = _check(parser, DC.interleave(frames))
    assert list(gm["data_len"]) == list(range(1, len(m) + 1))
    assert int(gm["verdict"][-1]) == 0 and len(set(int(v) for v in gm["verdict"])) >= 8


def _with_work(target):
    """A query message whose work is exactly `target`: questions of one label of k bytes cost
    4 + k (the question, the call, the iteration, the dot and the label)."""
    assert target >= 5
    qs, left = [], target
    while left:
        k = min(63, left - 4)
        if 0 < left - (4 + k) < 5:  # leave room for a last question
            k -= 5
        qs.append(k)
        left -= 4 + k
    m = DC.hdr(len(qs)) + b"".join(DC.q(DC.name(b"a" * k)) for k in qs)
    assert R.decode(m).work == target and R.decode(m).err is None
    return m


@pytest.mark.parametrize("max_work", [40, 4096])
def test_budget_boundary(parser, max_work):
    """work == max_work decodes, max_work + 1 is deferred; a pointer chain bomb is deferred and
    then equals the model through messages(); an error inside the budget stays an error."""
    from gopacket_amd import dns as D
    msgs = [_with_work(max_work), _with_work(max_work + 1), _with_work(max_work - 1), DC.bomb(),
            DC.named_cases()["self_pointer"], DC.named_cases()["index_range"], DC.pointer_chain(16)]
    frames = DC.interleave([DC.eth(DC.ip4(DC.udp(m), 17)) for m in msgs])
    res, gm, models = _check(parser, frames, max_work=max_work)
    v = [int(x) for x in gm["verdict"]]
    assert v[0] == 0 and v[1] == R.DEFERRED and v[2] == 0 and v[3] == R.DEFERRED
    assert v[4] == (R.E_MAX_RECURSION if max_work >= 512 else R.DEFERRED)  # its work is 512
    assert v[5] == R.E_INDEX_RANGE and v[6] == (0 if max_work >= 39 else R.DEFERRED)
    assert int(gm["n_q"][1]) == 0 and int(gm["qdcount"][1]) > 0
    bomb = res.messages()[3]
    assert bomb.err is None and len(bomb.Answers) == 400 and len(bomb.Answers[399].CNAME) == 253
    with pytest.raises(Exception):
        D.DecodeDNS(parser, *_decode(parser, PacketBatch.from_packets(frames)), max_work=0)
    with pytest.raises(Exception):
        D.DecodeDNS(parser, *_decode(parser, PacketBatch.from_packets(frames)), max_work=65536)


def test_capacities_exact_and_one_short(parser):
    from gopacket_amd import _lib
    from gopacket_amd import dns as D
    frames = DC.interleave([DC.eth(DC.ip4(DC.udp(m), 17)) for m in ALL_MESSAGES[:24]])
    batch = PacketBatch.from_packets(frames)
    db, dr = _decode(parser, batch)
    full = D.DecodeDNS(parser, db, dr)
    need = (full.count, full.n_entries, full.name_bytes)
    assert min(need) > 1
    want = full.to_host()
    for k in range(3):
        caps = tuple(c - (1 if j == k else 0) for j, c in enumerate(need))
        with pytest.raises(_lib.GpdError) as e:
            D.DecodeDNS(parser, db, dr, caps=caps)
        c = e.value.counts
        assert (c["msgs"], c["entries"], c["name_bytes"]) == need  # the needs are reported
        again = D.DecodeDNS(parser, db, dr, caps=need).to_host()   # and the retry succeeds
        assert all(np.array_equal(np.frombuffer(a if isinstance(a, bytes) else a.tobytes(), np.uint8),
                                  np.frombuffer(b if isinstance(b, bytes) else b.tobytes(), np.uint8))
                   for a, b in zip(again, want))
    roomy = D.DecodeDNS(parser, db, dr, caps=(need[0] + 3, need[1] + 5, need[2] + 7))
    assert (roomy.count, roomy.n_entries, roomy.name_bytes) == need


def test_no_candidates_and_empty_batch(parser):
    from gopacket_amd import dns as D
    res, gm, _ = _check(parser, DC.NOISE * 3)
    assert res.count == 0 and res.messages() == []


def test_scans_past_their_first_round(parser):
    """The smallest candidate count that takes gpd_compact.h's scan over the block counts, and the
    two-level scans of the entry counts and name bytes, into a second round: SCAN_ROUND blocks of
    COMPACT_BLOCK candidates and one more (2,097,153), short queries, with a non-DNS packet after
    every fourth so that the compaction moves every index."""
    from gopacket_amd import dns as D
    cand = D.COMPACT_BLOCK * D.SCAN_ROUND + 1
    assert cand == 2097153
    labels = (b"a", b"bcd", b"efghi", b"jk")
    tmpl = [DC.eth(DC.ip4(DC.udp(DC.hdr(1, flags=0x0100) + DC.q(DC.name(x, b"example", b"org"), t=1 + 27 * (k & 1))), 17))
            for k, x in enumerate(labels)]
    tmpl.append(DC.eth(DC.ip4(DC.udp(b"x" * 20, dport=5000), 17)))
    slot = 96
    assert max(len(t) for t in tmpl) <= slot
    period = np.zeros((5, slot), np.uint8)
    for k, t in enumerate(tmpl):
        period[k, :len(t)] = np.frombuffer(t, np.uint8)
    n = cand + (cand - 1) // 4
    reps = (n + 4) // 5
    data = np.tile(period.reshape(-1), reps)[:n * slot]
    kind = np.arange(n) % 5
    caplen = np.array([len(t) for t in tmpl], np.uint32)[kind]
    ids = (np.arange(n, dtype=np.uint32) * 40503) & 0xFFFF
    data = data.reshape(n, slot)
    data[:, 42], data[:, 43] = ids >> 8, ids & 0xFF  # the message's ID
    batch = PacketBatch.from_arrays(np.concatenate([data.reshape(-1), np.zeros(PAD, np.uint8)]),
                                    np.arange(n, dtype=np.uint64) * slot, caplen, data_len=n * slot)
    db, dr = _decode(parser, batch)
    res = D.DecodeDNS(parser, db, dr)
    gm, ge, gn = res.to_host()
    is_c = kind != 4
    pk = np.nonzero(is_c)[0]
    assert res.count == cand == len(pk) and res.n_entries == cand and res.deferred == 0
    # every msg record's header fields, vectorised
    assert np.array_equal(gm["packet"], pk.astype(np.uint32))
    assert (gm["data_off"] == 42).all() and np.array_equal(gm["data_len"], caplen[pk] - 42)
    assert np.array_equal(gm["id"], ids[pk].astype(np.uint16)) and (gm["flags"] == 0x0100).all()
    assert (gm["qdcount"] == 1).all() and (gm["n_q"] == 1).all() and (gm["verdict"] == 0).all()
    for f in ("ancount", "nscount", "arcount", "n_an", "n_ns", "n_ar", "rcode", "truncated", "reserved", "err_arg0",
              "err_arg1"):
        assert not gm[f].any(), f
    assert np.array_equal(gm["first_entry"], np.arange(cand, dtype=np.uint32))
    # the entries: name lengths by kind, offsets their exclusive prefix sum (the full totals)
    nlen = np.array([len(x) + 12 for x in labels], np.uint16)[kind[pk]]
    assert np.array_equal(ge["name_len"], nlen)
    off = np.concatenate([[0], np.cumsum(nlen.astype(np.uint64))])
    assert res.name_bytes == int(off[-1]) == len(gn)
    assert np.array_equal(ge["name_off"], off[:-1].astype(np.uint32))
    assert np.array_equal(ge["type"], np.where(kind[pk] & 1, 28, 1).astype(np.uint16)) and (ge["klass"] == 1).all()
    for f in ("rname1_len", "rname2_len", "rdlength", "ttl", "rdata_off", "fixed_off", "section"):
        assert not ge[f].any(), f
    # the names: every byte, by kind
    want_names = [x + b".example.org" for x in labels]
    names = np.frombuffer(gn, np.uint8)
    for k, w in enumerate(want_names):
        starts = off[:-1][kind[pk] == k].astype(np.int64)
        got = names[starts[:, None] + np.arange(len(w))]
        assert (got == np.frombuffer(w, np.uint8)).all(), k
    # a strided sample and both ends against the model
    for j in list(range(0, cand, 99991)) + [D.COMPACT_BLOCK * D.SCAN_ROUND - 1, cand - 1]:
        i = int(pk[j])
        m = batch.packet(i)[42:]
        wm, we, wn = R.records(R.decode(m), len(m), 4096, packet=i, data_off=42, first_entry=j, name_base=int(off[j]))
        assert gm[j:j + 1].tobytes() == wm.tobytes() and ge[j:j + 1].tobytes() == we.tobytes()
        assert gn[int(off[j]):int(off[j + 1])] == wn


def test_fragmented_response_through_defrag(parser):
    """A DNS response over three IPv4 fragments goes through DefragBatch; its datagram batch,
    decoded with first layer IPv4, reaches DecodeDNS with the result of the unfragmented packet."""
    from gopacket_amd import dns as D
    from gopacket_amd import parser as P
    from gopacket_amd.defrag import IPv4Fragments
    from gopacket_amd.ip4reasm import NewIPv4Defragmenter
    m = DC.hdr(1, 1, flags=0x8180) + DC.q(DC.WWW, t=16) + DC.rr(DC.ptr(12), 16, b"\x3f" + b"t" * 63 + b"\x20" + b"u" * 32)
    dgram = DC.udp(m)
    assert len(dgram) > 120
    cuts = (0, 48, 96, len(dgram))
    frags = [DC.eth(DC.ip4(dgram[a:b], 17, frag=(0x2000 if b < len(dgram) else 0) | (a // 8), ident=77))
             for a, b in zip(cuts, cuts[1:])]
    whole = DC.eth(DC.ip4(dgram, 17, ident=77))
    batch = PacketBatch.from_packets([DC.NOISE[0], frags[0], frags[2], DC.NOISE[1], frags[1]])
    db, dr = _decode(parser, batch)
    assert D.DecodeDNS(parser, db, dr).count == 0  # a fragment's decode ends at Fragment
    out, cnt = IPv4Fragments(parser, db, dr)
    assert cnt == 3
    dg = NewIPv4Defragmenter(parser).DefragBatch(db, out, cnt)
    assert dg.ndgrams == 1
    p4 = P.NewDecodingLayerParser(L.LayerTypeIPv4)
    p4._mask = ALL
    dr4 = P.DeviceResult(dg.batch.n, 0)
    p4.decode_device(dg.batch, dr4)
    got = D.DecodeDNS(p4, dg.batch, dr4)
    ref, gm, _ = _check(parser, [whole])
    a, b = got.to_host(), ref.to_host()
    assert got.count == 1 and int(a[0]["data_off"][0]) == 28 and int(b[0]["data_off"][0]) == 42
    a[0]["data_off"] = 42
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    DC.same_object(got.messages()[0], R.decode(m))


def test_bpf_keep_mask_then_select_then_dns(parser):
    """`udp port 53` as a BPF keep mask, pcapwrite.select, decode, DecodeDNS: the UDP messages of
    the batch, in order."""
    import bpf_cases as BC
    from gopacket_amd import bpf as B
    from gopacket_amd import dns as D
    from gopacket_amd import parser as P
    from gopacket_amd import pcapwrite as PW
    udp53 = list(BC.UDP80)
    udp53[8], udp53[10] = (0x15, 2, 0, 53), (0x15, 0, 1, 53)
    msgs = ALL_MESSAGES[:30]
    frames = DC.interleave([DC.ENCAPS["eth_ip4_tcp" if k % 3 == 0 else "eth_ip4_udp"](m) for k, m in enumerate(msgs)])
    batch = PacketBatch.from_packets(frames)
    db = P.DeviceBatch(batch, 0)
    f = B.NewBPFInstructionFilter([B.BPFInstruction(*i) for i in udp53], parser)
    keep = f.match_device(db)
    sel, index = PW.select(parser, db, keep)
    dr = P.DeviceResult(sel.n, 0)
    parser.decode_device(sel, dr)
    res = D.DecodeDNS(parser, sel, dr)
    kept = [frames[int(i)] for i in index.cpu().numpy()]
    sub = PacketBatch.from_packets(kept)
    wm, we, wn, models = DC.expect(sub, _oracle(sub, parser))
    gm, ge, gn = res.to_host()
    assert gm.tobytes() == wm.tobytes() and ge.tobytes() == we.tobytes() and gn == wn
    assert [d for d, _ in models] == [m for k, m in enumerate(msgs) if k % 3]
