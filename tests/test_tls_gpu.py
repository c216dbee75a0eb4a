"""The TLS record decode on the GPU (gpd_tls_decode, gpd_tls_decode_ranges, include/gpd_tls.h):
message records and record entries compared byte for byte with the model (tests/tls_ref.py) over
the candidates and payloads the CPU oracle finds, `messages()` against the model's objects, the
ranges entry against the model and against the per-packet path, and the streams the TCP assembly
gathered decoded where they lie."""
import ctypes as C

import numpy as np
import pytest

import oracle_ref as O
import tls_cases as TC
import tls_ref as R
from gopacket_amd import layers as L
from gopacket_amd import synth
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


def _oracle(batch, parser, first=L.LayerTypeEthernet, tables=None):
    kw = {} if tables is None else {"tables": tables}
    return O.decode(batch, first, parser.decoders, parser.options, ext=True, nthreads=8, **kw)


def _same_arrays(res, wm, wr):
    gm, gr = res.to_host()
    assert res.count == len(wm) and res.n_records == len(wr)
    for k in range(len(wm)):
        assert gm[k:k + 1].tobytes() == wm[k:k + 1].tobytes(), (k, gm[k], wm[k])
    assert gr.tobytes() == wr.tobytes()
    assert res.deferred == int((wm["verdict"] == R.DEFERRED).sum())
    return gm, gr


def _same_objects(res, wm, models):
    objs = res.messages()
    assert len(objs) == len(models)
    for o, m, (data, t) in zip(objs, wm, models):
        assert o.packet == int(m["packet"])
        TC.same_object(o, t)


def _check(parser, frames, records=False, max_records=1024, objects=True, align=16, tables=None):
    """Decode the frames, run DecodeTLS and compare everything with the model; returns (result,
    host msgs, host recs, the model's (data, TLS) pairs)."""
    from gopacket_amd import tls as T
    batch = frames if isinstance(frames, PacketBatch) else PacketBatch.from_packets(frames, align=align)
    db, dr = _decode(parser, batch, records)
    res = T.DecodeTLS(parser, db, dr, max_records=max_records)
    wm, wr, models = TC.expect(batch, _oracle(batch, parser, tables=tables), max_records)
    gm, gr = _same_arrays(res, wm, wr)
    if objects:
        _same_objects(res, wm, models)
    return res, gm, gr, models


def _up(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to("cuda:0")


ALL_MESSAGES = [m for _, m in TC.vector_messages()] + list(TC.packet_cases().values())


# ---------------------------------------------------------------- 1. vectors and cases, every encapsulation
@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("encap", list(TC.ENCAPS))
def test_vectors_and_cases_in_every_encapsulation(parser, encap, records):
    """The reference's vectors and every hand-built case a packet can carry as real frames, between
    non-TLS TCP, UDP, ARP, runts, empty port-443 packets and a cut TCP header, in both result
    forms; the data-offset encapsulations packed back to back, so that `data` starts at every
    alignment mod 4."""
    packed = encap.startswith("doff")
    frames = TC.interleave([TC.ENCAPS[encap](m) for m in ALL_MESSAGES])
    batch = PacketBatch.from_packets(frames, align=1 if packed else 16)
    res, gm, gr, models = _check(parser, batch, records)
    assert res.count == len(ALL_MESSAGES)  # none of the noise is a candidate, every message is
    assert [d for d, _ in models] == ALL_MESSAGES
    assert [int(p) for p in gm["packet"]] == list(range(1, 2 * len(ALL_MESSAGES), 2))
    # every reachable verdict is seen, and nothing else; none is deferred at the default budget
    assert set(int(v) for v in gm["verdict"]) == R.REACHABLE
    assert res.deferred == 0
    if packed:
        start = batch.offset[gm["packet"]].astype(np.int64) + gm["data_off"]
        assert set(int(x) for x in start % 4) == {0, 1, 2, 3}


# ---------------------------------------------------------------- 2. padding, capture cuts, port tables
def test_padding_and_ip_length_bound_the_data(parser):
    """A 7-byte alert in a padded frame (64 bytes: the headers' 54 and the alert are 61): data is
    the 7 bytes, not the padding.  With the IP length one short the alert loses its description;
    with one more, a padding byte follows."""
    alert = TC.rec(TC.ALERT, b"\x02\x28")
    fr = lambda ln: synth.tcp_frame(TC.MAC[:4], TC.MAC[4:8], 40000, 443, 1, flags=0x18, payload=alert,
                                    ip_length=ln, pad_to=64)
    frames = [fr(None), fr(20 + 20 + 6), fr(20 + 20 + 8)]
    assert all(len(f) == 64 for f in frames)
    res, gm, gr, _ = _check(parser, frames)
    assert list(gm["data_len"]) == [7, 6, 8] and (gm["data_off"] == 54).all()
    assert [int(v) for v in gm["verdict"]] == [R.OK, R.E_LENGTH_MISMATCH, R.E_TOO_SHORT]
    assert list(gm["err_off"]) == [7, 0, 7] and res.n_records == 2


def test_client_hello_captured_at_every_length(parser):
    v = TC.VEC["vectors"][0]
    frame = bytes.fromhex(v["hex"])
    assert v["tls_off"] == 54
    caps = list(range(54, len(frame) + 1))
    data = np.concatenate([np.frombuffer(frame, np.uint8)] * len(caps) + [np.zeros(PAD, np.uint8)])
    batch = PacketBatch.from_arrays(data, np.arange(len(caps), dtype=np.uint64) * len(frame),
                                    np.array(caps, np.uint32), data_len=len(caps) * len(frame))
    res, gm, gr, _ = _check(parser, batch)
    # caplen 54 has no payload and is no candidate; from 55 on data_len follows the capture
    assert list(gm["data_len"]) == [c - 54 for c in caps[1:]]
    v = [int(x) for x in gm["verdict"]]
    assert v[-1] == R.OK and all(x in (R.E_TOO_SHORT, R.E_LENGTH_MISMATCH) for x in v[:-1])
    assert v[:4] == [R.E_TOO_SHORT] * 4 and v[4] == R.E_LENGTH_MISMATCH and gm["truncated"][:-1].all()


def test_candidates_follow_the_port_tables():
    """RegisterTCPPortLayerType / RegisterUDPPortLayerType and reload_tables: a port registered to
    TLS at run time is a candidate (a UDP one too), an unregistered one is none."""
    from gopacket_amd import parser as P
    from gopacket_amd import tls as T
    saved = L.TABLES.copy()
    try:
        p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
        p._mask = ALL
        m = TC.named_cases()["all_four"]
        frames = [TC.eth(TC.ip4(TC.tcp(m, dport=8443), 6)), TC.eth(TC.ip4(TC.tcp(m, dport=443), 6)),
                  TC.eth(TC.ip4(TC.udp(m, dport=4433), 17)), TC.eth(TC.ip4(TC.tcp(m, dport=993), 6))]
        batch = PacketBatch.from_packets(frames)
        res, gm, _, _ = _check(p, batch)
        assert list(gm["packet"]) == [1, 3]
        L.RegisterTCPPortLayerType(8443, L.LayerTypeTLS)
        L.RegisterUDPPortLayerType(4433, L.LayerTypeTLS)
        L.TABLES.tcp_port[993] = 0  # unregistered
        p.reload_tables()
        res, gm, _, _ = _check(p, batch, tables=L.TABLES)
        assert list(gm["packet"]) == [0, 1, 2] and list(gm["data_off"]) == [54, 54, 42]
        assert (gm["verdict"] == 0).all() and res.n_records == 15
    finally:
        L.TABLES.tcp_port[:] = saved.tcp_port
        L.TABLES.udp_port[:] = saved.udp_port


# ---------------------------------------------------------------- 3. compaction edges
@pytest.mark.parametrize("cand", [63, 64, 65, 2047, 2048, 2049])
def test_compaction_edges(parser, cand):
    """Candidate counts around a wave and a compaction block, a non-candidate after every third
    packet, record counts cycling 0..4: first_record is the exclusive prefix sum."""
    from gopacket_amd import tls as T
    msgs = [b"\x16\x03\x03"] + [TC.rec(TC.APP, bytes([k])) * k for k in (1, 2, 3, 4)]  # 0 records: too short
    frames = []
    for j in range(cand):
        frames.append(TC.eth(TC.ip4(TC.tcp(msgs[j % 5], sport=1024 + j), 6)))
        if j % 3 == 2:
            frames.append(TC.NOISE[(j // 3) % 4])
    batch = PacketBatch.from_packets(frames)
    db, dr = _decode(parser, batch)
    res = T.DecodeTLS(parser, db, dr)
    gm, gr = res.to_host()
    nrec = np.arange(cand) % 5
    assert res.count == cand and res.n_records == int(nrec.sum())
    assert np.array_equal(gm["first_record"], np.concatenate([[0], np.cumsum(nrec)[:-1]]).astype(np.uint32))
    assert np.array_equal(gm["n_appdata"], nrec.astype(np.uint32))
    assert np.array_equal(gm["packet"], (np.arange(cand) + np.arange(cand) // 3).astype(np.uint32))
    assert np.array_equal(gr["index_in_kind"], np.concatenate([np.arange(k) for k in nrec]).astype(np.uint32))
    wm, wr, _ = TC.expect(batch, _oracle(batch, parser))
    assert gm.tobytes() == wm.tobytes() and gr.tobytes() == wr.tobytes()


# ---------------------------------------------------------------- 4. scans past their first round
def test_scans_past_their_first_round(parser):
    """The smallest candidate count that takes gpd_compact.h's scan over the block counts, and the
    two-level scan of the record counts, into a second round: SCAN_ROUND blocks of COMPACT_BLOCK
    candidates and one more (2,097,153), one or two records each, with a non-TLS packet after every
    fourth so that the compaction moves every index."""
    from gopacket_amd import tls as T
    cand = T.COMPACT_BLOCK * T.SCAN_ROUND + 1
    assert cand == 2097153
    bodies = (TC.rec(TC.APP, b"a"), TC.rec(TC.HS, b"bcd") + TC.rec(TC.APP, b"xy"), TC.rec(TC.APP, b"efghi"),
              TC.rec(TC.CCS, b"\x01") + TC.rec(TC.ALERT, b"\x01\x00"))
    tmpl = [TC.eth(TC.ip4(TC.tcp(b), 6)) for b in bodies]
    tmpl.append(TC.eth(TC.ip4(TC.tcp(b"x" * 20, dport=8080), 6)))
    slot = 80
    assert max(len(t) for t in tmpl) <= slot
    period = np.zeros((5, slot), np.uint8)
    for k, t in enumerate(tmpl):
        period[k, :len(t)] = np.frombuffer(t, np.uint8)
    n = cand + (cand - 1) // 4
    reps = (n + 4) // 5
    data = np.tile(period.reshape(-1), reps)[:n * slot]
    kind = np.arange(n) % 5
    caplen = np.array([len(t) for t in tmpl], np.uint32)[kind]
    vers = (np.arange(n, dtype=np.uint32) * 40503) & 0xFFFF
    data = data.reshape(n, slot)
    data[:, 55], data[:, 56] = vers >> 8, vers & 0xFF  # the first record's version
    batch = PacketBatch.from_arrays(np.concatenate([data.reshape(-1), np.zeros(PAD, np.uint8)]),
                                    np.arange(n, dtype=np.uint64) * slot, caplen, data_len=n * slot)
    db, dr = _decode(parser, batch)
    res = T.DecodeTLS(parser, db, dr)
    gm, gr = res.to_host()
    pk = np.nonzero(kind != 4)[0]
    kd = kind[pk]
    nrec = np.array([1, 2, 1, 2], np.uint32)[kd]
    assert res.count == cand == len(pk) and res.n_records == int(nrec.sum()) and res.deferred == 0
    # every message record's fields, vectorised
    first = np.concatenate([[0], np.cumsum(nrec.astype(np.uint64))])
    assert np.array_equal(gm["packet"], pk.astype(np.uint32))
    assert (gm["data_off"] == 54).all() and np.array_equal(gm["data_len"], caplen[pk] - 54)
    assert np.array_equal(gm["first_record"], first[:-1].astype(np.uint32))
    assert np.array_equal(gm["n_ccs"], (kd == 3).astype(np.uint32))
    assert np.array_equal(gm["n_handshake"], (kd == 1).astype(np.uint32))
    assert np.array_equal(gm["n_appdata"], (kd != 3).astype(np.uint32))
    assert np.array_equal(gm["n_alert"], (kd == 3).astype(np.uint32))
    assert np.array_equal(gm["contents_off"], np.array([0, 8, 0, 6], np.uint32)[kd])
    assert np.array_equal(gm["err_off"], gm["data_len"])
    assert not gm["verdict"].any() and not gm["truncated"].any() and not gm["reserved"].any()
    # every record entry's fields, vectorised: the first record of a message, then the second
    f0 = first[:-1].astype(np.int64)
    two = nrec == 2
    f1 = f0[two] + 1
    assert np.array_equal(gr["off"][f0], np.zeros(cand, np.uint32))
    assert np.array_equal(gr["off"][f1], np.array([0, 8, 0, 6], np.uint32)[kd[two]])
    assert np.array_equal(gr["version"][f0], vers[pk].astype(np.uint16)) and (gr["version"][f1] == 0x0303).all()
    assert np.array_equal(gr["length"][f0], np.array([1, 3, 5, 1], np.uint16)[kd])
    assert (gr["length"][f1] == 2).all()
    assert np.array_equal(gr["content_type"][f0], np.array([23, 22, 23, 20], np.uint8)[kd])
    assert np.array_equal(gr["content_type"][f1], np.array([0, 23, 0, 21], np.uint8)[kd[two]])
    assert not gr["index_in_kind"].any() and not gr["flags"].any()
    assert np.array_equal(gr["a"][f0], (kd == 3).astype(np.uint8))
    assert np.array_equal(gr["a"][f1], (kd[two] == 3).astype(np.uint8)) and not gr["b"].any()
    # a strided sample and both ends against the model
    for j in list(range(0, cand, 99991)) + [T.COMPACT_BLOCK * T.SCAN_ROUND - 1, cand - 1]:
        i = int(pk[j])
        m = batch.packet(i)[54:]
        wm, wr = R.records(R.decode(m), len(m), 1024, packet=i, data_off=54, first_record=int(first[j]))
        assert gm[j:j + 1].tobytes() == wm.tobytes()
        assert gr[int(first[j]):int(first[j + 1])].tobytes() == wr.tobytes()


# ---------------------------------------------------------------- 5. the budget
@pytest.mark.parametrize("max_records", [3, 1024])
def test_budget_boundary(parser, max_records):
    """work == max_records decodes, one more is deferred; an unknown type inside the budget stays an
    error; a jumbo payload of 2,000 zero-length records is deferred at 1024 and then equals the
    model through messages()."""
    from gopacket_amd import tls as T
    k = max_records
    msgs = [TC.zero_records(k), TC.zero_records(k + 1), TC.zero_records(k - 1) + TC.rec(99, b"zz"),
            TC.zero_records(k) + TC.rec(99, b"zz"), TC.zero_records(2000), TC.zero_records(k - 1)]
    frames = TC.interleave([TC.eth(TC.ip4(TC.tcp(m), 6)) for m in msgs])
    res, gm, gr, models = _check(parser, frames, max_records=max_records)
    v = [int(x) for x in gm["verdict"]]
    assert v == [R.OK, R.DEFERRED, R.E_UNKNOWN_TYPE, R.DEFERRED, R.DEFERRED, R.OK]
    assert list(gm["n_handshake"]) == [k, 0, k - 1, 0, 0, k - 1] and res.deferred == 3
    assert int(gm["data_len"][4]) == 10000 and not gm["err_off"][4] and not gm["contents_off"][4]
    jumbo = res.messages()[4]
    assert jumbo.err is None and len(jumbo.Handshake) == 2000 and jumbo.Contents == TC.rec(TC.HS)
    batch = PacketBatch.from_packets(frames)
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(Exception):
            T.DecodeTLS(parser, *_decode(parser, batch), max_records=bad)
    assert T.DecodeTLS(parser, *_decode(parser, batch), max_records=1 << 20).deferred == 0


# ---------------------------------------------------------------- 6. capacities
def test_capacities_exact_and_one_short(parser):
    from gopacket_amd import _lib
    from gopacket_amd import tls as T
    frames = TC.interleave([TC.eth(TC.ip4(TC.tcp(m), 6)) for m in ALL_MESSAGES[:24]])
    batch = PacketBatch.from_packets(frames)
    db, dr = _decode(parser, batch)
    full = T.DecodeTLS(parser, db, dr)
    need = (full.count, full.n_records)
    assert min(need) > 1
    want = full.to_host()
    for k in range(2):
        caps = tuple(c - (1 if j == k else 0) for j, c in enumerate(need))
        with pytest.raises(_lib.GpdError) as e:
            T.DecodeTLS(parser, db, dr, caps=caps)
        c = e.value.counts
        assert (c["msgs"], c["records"]) == need                       # the needs are reported
        again = T.DecodeTLS(parser, db, dr, caps=need).to_host()       # and the retry succeeds
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, want))
    roomy = T.DecodeTLS(parser, db, dr, caps=(need[0] + 3, need[1] + 5))
    assert (roomy.count, roomy.n_records) == need
    assert all(a.tobytes() == b.tobytes() for a, b in zip(roomy.to_host(), want))


# ---------------------------------------------------------------- 7. empty cases
def test_no_candidates_empty_batch_and_no_ranges(parser):
    import torch
    from gopacket_amd import parser as P
    from gopacket_amd import tls as T
    res, gm, gr, _ = _check(parser, TC.NOISE * 3)
    assert res.count == 0 and res.n_records == 0 and res.messages() == []
    empty = PacketBatch.from_packets([])
    res = T.DecodeTLS(parser, P.DeviceBatch(empty, 0), P.DeviceResult(0, 0))
    assert res.count == 0 and res.messages() == []
    z8 = torch.zeros(0, dtype=torch.uint8, device="cuda:0")
    res = T.DecodeTLSRanges(parser, z8, torch.zeros(0, dtype=torch.int64, device="cuda:0"),
                            torch.zeros(0, dtype=torch.int32, device="cuda:0"))
    assert res.count == 0 and res.n_records == 0 and res.messages() == []


# ---------------------------------------------------------------- 8. ranges
def _range_inputs():
    """The vectors, every case and the vectors' truncations back to back, zero-length ranges in
    between; the last range ends at the buffer's last byte."""
    datas = [m for _, m in TC.vector_messages()] + list(TC.named_cases().values())
    for _, m in TC.vector_messages()[:7]:
        step = 1 if len(m) < 80 else 7
        datas += [m[:k] for k in range(0, len(m), step)]
    out = []
    for k, d in enumerate(datas):
        out.append(d)
        if k % 5 == 0:
            out.append(b"")
    out.append(TC.rec(TC.ALERT, b"\x02\x28"))  # its description is the buffer's last byte
    return out


def test_ranges_equal_the_model(parser):
    import torch
    from gopacket_amd import _lib
    from gopacket_amd import tls as T
    datas = _range_inputs()
    lens = np.array([len(d) for d in datas], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    buf = _up(np.frombuffer(b"".join(datas), np.uint8))
    assert buf.numel() == int(lens.sum()) == int(off[-1] + lens[-1])  # no byte behind the last range
    d_off, d_len = _up(off, np.int64), _up(lens, np.int32)
    res = T.DecodeTLSRanges(parser, buf, d_off, d_len)
    wm, wr, models = TC.expect_ranges(datas)
    gm, gr = _same_arrays(res, wm, wr)
    assert np.array_equal(gm["packet"], np.arange(len(datas), dtype=np.uint32)) and not gm["data_off"].any()
    assert int((lens == 0).sum()) > 20 and (gm["verdict"][lens == 0] == R.E_TOO_SHORT).all()
    assert set(int(v) for v in gm["verdict"]) == R.REACHABLE
    _same_objects(res, wm, models)
    # the budget through the ranges: the 300-record case defers at 299
    tight = T.DecodeTLSRanges(parser, buf, d_off, d_len, max_records=299)
    wm2, wr2, _ = TC.expect_ranges(datas, 299)
    _same_arrays(tight, wm2, wr2)
    assert tight.deferred == 1
    # one range passing nbytes: an error, and nothing is written
    bad = off.copy()
    bad[len(bad) // 2] = buf.numel() - 2  # (a 5-byte or longer range there ends past the buffer)
    k = len(bad) // 2
    lens_bad = lens.copy()
    lens_bad[k] = 5
    need = (res.count, res.n_records)
    msgs = torch.full((need[0] * 48,), 0xA5, dtype=torch.uint8, device="cuda:0")
    recs = torch.full((need[1] * 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    keep = (_up(bad, np.int64), _up(lens_bad, np.int32))
    rg = T.GpdTlsRanges(buf.data_ptr(), buf.numel(), keep[0].data_ptr(), keep[1].data_ptr(), len(bad))
    out = T.GpdTlsOut(msgs.data_ptr(), need[0] + 8, recs.data_ptr(), need[1] + 8)
    cnt = T.GpdTlsCounts()
    rc = T.tls_lib().gpd_tls_decode_ranges(parser.ctx().h, C.byref(rg), None, C.byref(out), C.byref(cnt),
                                           C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc != 0 and "1 of the" in _lib.lib.gpd_last_error_string().decode()
    torch.cuda.synchronize()
    assert bool((msgs == 0xA5).all()) and bool((recs == 0xA5).all())
    with pytest.raises(_lib.GpdError):
        T.DecodeTLSRanges(parser, buf, keep[0], keep[1])


def test_ranges_and_packets_agree(parser):
    """The same messages through gpd_tls_decode_ranges and through the per-packet path: identical
    verdicts and entries (the two data sources of one set of kernels)."""
    from gopacket_amd import tls as T
    lens = np.array([len(m) for m in ALL_MESSAGES], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rr = T.DecodeTLSRanges(parser, _up(np.frombuffer(b"".join(ALL_MESSAGES), np.uint8)), _up(off, np.int64),
                           _up(lens, np.int32))
    batch = PacketBatch.from_packets([TC.eth(TC.ip4(TC.tcp(m), 6)) for m in ALL_MESSAGES], align=1)
    pr = T.DecodeTLS(parser, *_decode(parser, batch))
    (rm, rrec), (pm, prec) = rr.to_host(), pr.to_host()
    assert rr.count == pr.count == len(ALL_MESSAGES) and rrec.tobytes() == prec.tobytes()
    assert (pm["data_off"] == 54).all()
    pm["data_off"] = 0
    assert rm.tobytes() == pm.tobytes()


# ---------------------------------------------------------------- 9. through the stream assembly
SYN, ACK, PSH = 0x02, 0x10, 0x08
A4, B4 = bytes([10, 1, 0, 1]), bytes([10, 1, 0, 2])


def _segments(data, cuts, src, dst, sport, dport, isn, swap=None):
    """A bare SYN, then `data` cut at `cuts` into segments in sequence; swap=(i, j) exchanges two."""
    edges = [0] + list(cuts) + [len(data)]
    segs = [synth.tcp_frame(src, dst, sport, dport, isn + 1 + a, ack=1, flags=ACK | PSH, payload=data[a:b], pad_to=60)
            for a, b in zip(edges, edges[1:])]
    if swap:
        segs[swap[0]], segs[swap[1]] = segs[swap[1]], segs[swap[0]]
    return [synth.tcp_frame(src, dst, sport, dport, isn, flags=SYN, pad_to=60)] + segs


def test_streams_through_the_assembly(parser):
    """The vectors' three handshake flights as one client and one server stream, cut into TCP
    segments inside record headers and bodies, two segments of each out of order, through
    TCPSegments (grouped), TCPStreams(close_all) and DecodeTLSStreams: each stream's message is the
    model's decode of the concatenated bytes.  A third stream ends inside a record."""
    from gopacket_amd import parser as P
    from gopacket_amd import tcpassembly as TA
    from gopacket_amd import tcpstream as S
    from gopacket_amd import tls as T
    from gopacket_amd.flows import NewFlowTable
    client = TC.vector("testClientHello") + TC.vector("testClientKeyExchange")
    server = TC.vector("testServerHello") + TC.vector("testNewSessionTicket")
    cut = client[:214 + 100]  # ends inside ClientKeyExchange's second record (81 + 5 + 48 > 100)
    streams = {
        "client": _segments(client, (3, 100, 216, 300), A4, B4, 40001, 443, 1000, swap=(2, 3)),
        "server": _segments(server, (2, 60, 474, 479, 600), B4, A4, 443, 40002, 5000, swap=(1, 2)),
        "cut": _segments(cut, (214, 220), A4, B4, 40003, 443, 9000),
    }
    frames = []
    for step in range(max(map(len, streams.values()))):  # the three connections interleaved
        for fr in streams.values():
            if step < len(fr):
                frames.append(fr[step])
    batch = PacketBatch.from_packets(frames)
    db, dr = _decode(parser, batch)
    table = NewFlowTable(parser, 128)
    ids = table.Insert(db, dr)
    segs, groups, count, ngroups, ungrouped = TA.TCPSegments(parser, db, dr, flow_id=ids, table=table)
    assert ngroups == 3 and ungrouped == 0
    sres = S.TCPStreams(parser, db, segs, groups, count, ngroups, close_all=True)
    assert sres.nstreams == 3 and sres.nbytes == len(client) + len(server) + len(cut)
    res = T.DecodeTLSStreams(parser, sres)
    gm, gr = res.to_host()
    host = S.streams_to_host(sres)
    want = {"client": client, "server": server, "cut": cut}
    seen = {}
    for k, st in enumerate(host.streams):
        data = host.bytes[int(st["byte_off"]):int(st["byte_off"]) + int(st["nbytes"])].tobytes()
        name = next(n for n, d in want.items() if d == data)  # the assembly put the bytes in sequence
        seen[name] = k
        wm, wr = R.records(R.decode(data), len(data), 1024, packet=k, first_record=int(gm["first_record"][k]))
        assert gm[k:k + 1].tobytes() == wm.tobytes(), (name, gm[k], wm)
        n = int(wm["n_ccs"][0] + wm["n_handshake"][0] + wm["n_appdata"][0] + wm["n_alert"][0])
        assert gr[int(gm["first_record"][k]):int(gm["first_record"][k]) + n].tobytes() == wr.tobytes()
    assert sorted(seen) == ["client", "cut", "server"] and res.n_records == 4 + 6 + 3
    for o, k in zip(res.messages(), range(3)):
        name = next(n for n, j in seen.items() if j == k)
        TC.same_object(o, R.decode(want[name]))
    c, s, x = (gm[seen[n]] for n in ("client", "server", "cut"))
    assert int(c["verdict"]) == 0 and (int(c["n_handshake"]), int(c["n_ccs"])) == (3, 1) and int(c["err_off"]) == len(client)
    assert int(s["verdict"]) == 0 and (int(s["n_handshake"]), int(s["n_ccs"])) == (5, 1)
    # the stream that ends mid-record: the records before it kept, err_off at that record's header
    assert int(x["verdict"]) == R.E_LENGTH_MISMATCH and int(x["truncated"]) == 1
    assert int(x["err_off"]) == 214 + 81 == int(x["contents_off"]) and (int(x["n_handshake"]), int(x["n_ccs"])) == (2, 1)
    # the same batch packet by packet: a segment that begins mid-record gets the model's verdict
    # for its own bytes
    pres, pm, _, models = _check(parser, batch)
    assert pres.count == sum(len(f) - 1 for f in streams.values())
    verdicts = {int(m["verdict"]) for m in pm}
    # client[3:100] begins with the length's high byte (0), [0:3] is short, cut[214:220] is a header and a byte
    assert {R.OK, R.E_UNKNOWN_TYPE, R.E_TOO_SHORT, R.E_LENGTH_MISMATCH} <= verdicts


# ---------------------------------------------------------------- 10. BPF mask to TLS
# `tcp port 443` as tcpdump -dd prints it for Ethernet
TCP_PORT_443 = [
    (0x28, 0, 0, 12), (0x15, 0, 6, 0x86DD), (0x30, 0, 0, 20), (0x15, 0, 15, 6), (0x28, 0, 0, 54), (0x15, 12, 0, 443),
    (0x28, 0, 0, 56), (0x15, 10, 11, 443), (0x15, 0, 10, 0x0800), (0x30, 0, 0, 23), (0x15, 0, 8, 6), (0x28, 0, 0, 20),
    (0x45, 6, 0, 0x1FFF), (0xB1, 0, 0, 14), (0x48, 0, 0, 14), (0x15, 2, 0, 443), (0x48, 0, 0, 16), (0x15, 0, 1, 443),
    (0x06, 0, 0, 262144), (0x06, 0, 0, 0),
]


def test_bpf_keep_mask_then_select_then_tls(parser):
    """`tcp port 443` as a BPF keep mask, pcapwrite.select, decode, DecodeTLS: the port-443 messages
    of the batch, in order, equal to DecodeTLS restricted to the kept packets."""
    from gopacket_amd import bpf as B
    from gopacket_amd import parser as P
    from gopacket_amd import pcapwrite as PW
    from gopacket_amd import tls as T
    msgs = ALL_MESSAGES[:30]
    enc = lambda k, m: (TC.eth(TC.ip4(TC.tcp(m, dport=993), 6)) if k % 3 == 0 else
                        TC.eth(TC.ip6(TC.tcp(m), 6), 0x86DD) if k % 3 == 1 else TC.eth(TC.ip4(TC.tcp(m), 6)))
    frames = TC.interleave([enc(k, m) for k, m in enumerate(msgs)])
    batch = PacketBatch.from_packets(frames)
    db = P.DeviceBatch(batch, 0)
    f = B.NewBPFInstructionFilter([B.BPFInstruction(*i) for i in TCP_PORT_443], parser)
    keep = f.match_device(db)
    sel, index = PW.select(parser, db, keep)
    dr = P.DeviceResult(sel.n, 0)
    parser.decode_device(sel, dr)
    res = T.DecodeTLS(parser, sel, dr)
    kept = [frames[int(i)] for i in index.cpu().numpy()]
    sub = PacketBatch.from_packets(kept)
    wm, wr, models = TC.expect(sub, _oracle(sub, parser))
    gm, gr = res.to_host()
    assert gm.tobytes() == wm.tobytes() and gr.tobytes() == wr.tobytes()
    assert [d for d, _ in models] == [m for k, m in enumerate(msgs) if k % 3]
    # DecodeTLS of the whole batch, restricted to the kept packets
    whole = T.DecodeTLS(parser, *_decode(parser, batch)).to_host()[0]
    pos = {int(i): j for j, i in enumerate(index.cpu().numpy())}
    sel_of_whole = [m for m in whole if int(m["packet"]) in pos]
    assert [int(m["verdict"]) for m in sel_of_whole] == [int(v) for v in gm["verdict"]]
    assert [pos[int(m["packet"])] for m in sel_of_whole] == [int(p) for p in gm["packet"]]
