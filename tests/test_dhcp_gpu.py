"""The DHCP message decode on the GPU (gpd_dhcp_decode, include/gpd_dhcp.h): message records and
option entries compared byte for byte with the model (tests/dhcp_ref.py) over the candidates and
payloads the CPU oracle finds, and `messages()` against the model's objects."""
import re

import numpy as np
import pytest

import dhcp_cases as TC
import dhcp_ref as R
import oracle_ref as O
from conftest import ROOT
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


def _oracle(batch, parser, first=L.LayerTypeEthernet, tables=None):
    kw = {} if tables is None else {"tables": tables}
    return O.decode(batch, first, parser.decoders, parser.options, ext=True, nthreads=8, **kw)


def _same_arrays(res, wm, wo):
    gm, go = res.to_host()
    assert res.count == len(wm) and res.n_options == len(wo)
    for k in range(len(wm)):
        assert gm[k:k + 1].tobytes() == wm[k:k + 1].tobytes(), (k, gm[k], wm[k])
    assert go.tobytes() == wo.tobytes()
    assert res.deferred == int((wm["verdict"] == R.DEFERRED).sum())
    return gm, go


def _same_objects(res, wm, models):
    objs = res.messages()
    assert len(objs) == len(models)
    for o, m, (data, d) in zip(objs, wm, models):
        assert o.packet == int(m["packet"])
        TC.same_object(o, d)


def _check(parser, frames, records=False, max_options=2048, objects=True, align=16, tables=None):
    """Decode the frames, run DecodeDHCP and compare everything with the model; returns (result,
    host msgs, host opts, the model's (data, object) pairs)."""
    from gopacket_amd import dhcp as T
    batch = frames if isinstance(frames, PacketBatch) else PacketBatch.from_packets(frames, align=align)
    db, dr = _decode(parser, batch, records)
    res = T.DecodeDHCP(parser, db, dr, max_options=max_options)
    wm, wo, models = TC.expect(batch, _oracle(batch, parser, tables=tables), max_options)
    gm, go = _same_arrays(res, wm, wo)
    if objects:
        _same_objects(res, wm, models)
    return res, gm, go, models


ALL_MESSAGES = [m for _, m in TC.vector_messages()] + list(TC.packet_cases().values())
E4 = TC.ENCAPS["eth_ip4_udp"]


# ---------------------------------------------------------------- 1. vectors and cases, every encapsulation
@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("encap", list(TC.ENCAPS))
def test_vectors_and_cases_in_every_encapsulation(parser, encap, records):
    """The reference's vectors and every hand-built case of both versions as real frames, between
    other UDP, TCP to port 67, ARP, runts, empty port-67 packets and a cut UDP header, in both
    result forms; one encapsulation packed back to back, so that `data` starts at every alignment
    mod 4."""
    packed = encap == "packed"
    frames = TC.interleave([TC.ENCAPS[encap](vm) for vm in ALL_MESSAGES])
    batch = PacketBatch.from_packets(frames, align=1 if packed else 16)
    res, gm, go, models = _check(parser, batch, records)
    assert res.count == len(ALL_MESSAGES)  # none of the noise is a candidate, every message is
    assert [d for d, _ in models] == [m for _, m in ALL_MESSAGES]
    assert [int(v) for v in gm["version"]] == [v for v, _ in ALL_MESSAGES]
    assert [int(p) for p in gm["packet"]] == list(range(1, 2 * len(ALL_MESSAGES), 2))
    # every reachable verdict is seen, and nothing else; none is deferred at the default budget
    assert set(int(v) for v in gm["verdict"]) == R.REACHABLE
    assert set(int(v) for v in gm["verdict"][gm["version"] == 4]) == R.REACHABLE_V4
    assert set(int(v) for v in gm["verdict"][gm["version"] == 6]) == R.REACHABLE_V6
    assert res.deferred == 0 and not gm["reserved"].any()
    assert set(int(f) for f in gm["mflags"]) >= {0, R.F_CONTENTS, R.F_CONTENTS | R.F_RELAY, R.F_HW_PAST_DATA,
                                                 R.F_CONTENTS | R.F_HW_PAST_DATA}
    if packed:
        start = batch.offset[gm["packet"]].astype(np.int64) + gm["data_off"]
        assert set(int(x) for x in start % 4) == {0, 1, 2, 3}


# ---------------------------------------------------------------- 2. what bounds data, capture cuts, port tables
def test_udp_length_and_padding_bound_the_data(parser):
    """udp.go:42-51: data ends where UDP Length says (shorter than the capture), Length 0 takes the
    rest, a Length past the capture is cut by the capture; Ethernet padding behind the IPv4 length
    is not part of data.  A DHCPv6 message of 4 bytes in a padded 60-byte frame is OK with 4 bytes."""
    s, d = TC.SOLICIT, TC.DISCOVER
    u = lambda m, sp, dp, **kw: TC.udp(m, sport=sp, dport=dp, **kw)
    frames = [TC.eth(TC.ip4(u(s, 546, 547, length=8 + k), 17)) for k in (1, 3, 4, 25, 26, len(s) - 1, len(s))]
    frames += [TC.eth(TC.ip4(u(s, 546, 547, length=0), 17)), TC.eth(TC.ip4(u(s, 546, 547, length=len(s) + 100), 17)),
               TC.eth(TC.ip4(u(s, 546, 547) + b"trailer", 17, length=20 + 8 + len(s))) + b"pad",
               TC.eth(TC.ip4(u(s[:4], 546, 547), 17)).ljust(60, b"\xee"),
               TC.eth(TC.ip4(u(d, 68, 67, length=8 + 239), 17)), TC.eth(TC.ip4(u(d, 68, 67, length=8 + 240), 17)),
               TC.eth(TC.ip4(u(d, 68, 67, length=8 + 241), 17)), TC.eth(TC.ip4(u(d, 68, 67), 17)) + b"\x00\x00\xffpad"]
    res, gm, go, _ = _check(parser, frames)
    assert list(gm["data_len"]) == [1, 3, 4, 25, 26, len(s) - 1] + [len(s)] * 4 + [4, 239, 240, 241, len(d)]
    assert (gm["data_off"] == 42).all()
    v = [int(x) for x in gm["verdict"]]
    assert v[:3] == [R.E_V6_TOO_SHORT, R.E_V6_TOO_SHORT, R.OK] and v[10] == R.OK
    assert v[11:] == [R.E_V4_TOO_SHORT, R.OK, R.E_V4_OPT_NO_DATA, R.OK]
    assert list(gm["err_arg"][[0, 1, 11]]) == [1, 3, 239]


def test_messages_captured_at_every_length(parser):
    """A DHCPv4 DISCOVER of 8 options and a DHCPv6 relay-forward with a nested message, each
    captured at every length from its UDP header's end to the whole frame."""
    frames = [E4((4, TC.DISCOVER)), E4((6, TC.RELAY))]
    datas, offs, caps = [], [], []
    at = 0
    for f in frames:
        for c in range(42, len(f) + 1):
            datas.append(np.frombuffer(f, np.uint8))
            offs.append(at)
            caps.append(c)
            at += len(f)
    batch = PacketBatch.from_arrays(np.concatenate(datas + [np.zeros(PAD, np.uint8)]), np.array(offs, np.uint64),
                                    np.array(caps, np.uint32), data_len=at)
    res, gm, go, _ = _check(parser, batch)
    # caplen 42 has no payload and is no candidate; from 43 on data_len follows the capture
    assert list(gm["data_len"]) == list(range(1, len(TC.DISCOVER) + 1)) + list(range(1, len(TC.RELAY) + 1))
    v4, v6 = gm[gm["version"] == 4], gm[gm["version"] == 6]
    assert (v4["verdict"][:239] == R.E_V4_TOO_SHORT).all() and int(v4["verdict"][239]) == R.OK
    assert int(v4["verdict"][-1]) == R.OK and int(v4["n_opts"][-1]) == 8 and int(v4["n_opts"][-2]) == 8
    assert set(int(x) for x in v4["verdict"][240:]) == {R.OK, R.E_V4_OPT_NO_DATA, R.E_V4_OPT_MALFORMED}
    assert (v6["verdict"][:3] == R.E_V6_TOO_SHORT).all() and (v6["verdict"][3:33] == R.E_V6_RELAY_SHORT).all()
    assert int(v6["verdict"][33]) == R.OK and int(v6["verdict"][-1]) == R.OK and int(v6["n_opts"][-1]) == 3
    assert set(int(x) for x in v6["verdict"][34:]) == {R.OK, R.E_V6_OPT_NO_DATA, R.E_V6_OPT_SIZE}
    assert list(v6["err_arg"][3:33]) == list(range(4, 34))


def test_candidates_follow_the_port_tables():
    """RegisterUDPPortLayerType and reload_tables: a UDP port registered to DHCPv4 or DHCPv6 at run
    time is a candidate and gets that version's decode, and with 67 removed a packet to it is none."""
    from gopacket_amd import parser as P
    saved = L.TABLES.copy()
    try:
        p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
        p._mask = ALL
        u = lambda m, sp, dp: TC.eth(TC.ip4(TC.udp(m, sport=sp, dport=dp), 17))
        frames = [u(TC.DISCOVER, 40000, 6767), u(TC.DISCOVER, 40001, 67), u(TC.SOLICIT, 40000, 5470),
                  u(TC.SOLICIT, 40000, 547), u(TC.SOLICIT, 40000, 6767), u(TC.DISCOVER, 40000, 68)]
        batch = PacketBatch.from_packets(frames)
        res, gm, _, _ = _check(p, batch)
        assert list(gm["packet"]) == [1, 3, 5] and list(gm["version"]) == [4, 6, 4]
        L.RegisterUDPPortLayerType(6767, L.LayerTypeDHCPv4)
        L.RegisterUDPPortLayerType(5470, L.LayerTypeDHCPv6)
        L.TABLES.udp_port[67] = 0  # unregistered
        p.reload_tables()
        res, gm, _, _ = _check(p, batch, tables=L.TABLES)
        assert list(gm["packet"]) == [0, 2, 3, 4, 5] and list(gm["version"]) == [4, 6, 6, 4, 4]
        # a DHCPv6 message under the DHCPv4 decode is too short for it
        assert [int(v) for v in gm["verdict"]] == [0, 0, 0, R.E_V4_TOO_SHORT, 0] and res.n_options == 8 + 4 + 4 + 8
    finally:
        L.TABLES.tcp_port[:] = saved.tcp_port
        L.TABLES.udp_port[:] = saved.udp_port


# ---------------------------------------------------------------- 3. compaction edges
EDGE_MSGS = [(4, b"\x01"), (6, TC.SOLICIT[:4]), (6, TC.SOLICIT[:4] + TC.o6(14)), (6, TC.SOLICIT[:4] + TC.o6(8, b"\0\0") + TC.o6(14)),
             (4, TC.DISCOVER)]
EDGE_NOPT = [0, 0, 1, 2, 8]


@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("cand", [1, 255, 256, 257])
def test_compaction_edges(parser, cand, noise):
    """Candidate counts around a workgroup of the compaction, with a non-candidate after every
    third packet or with every packet a candidate; DHCPv4 and DHCPv6 interleaved within every
    wave, option counts cycling 0, 0, 1, 2, 8: first_opt is the exclusive prefix sum."""
    from gopacket_amd import dhcp as T
    frames = []
    for j in range(cand):
        frames.append(E4(EDGE_MSGS[j % 5]))
        if noise and j % 3 == 2:
            frames.append(TC.NOISE[(j // 3) % 4])
    batch = PacketBatch.from_packets(frames)
    db, dr = _decode(parser, batch)
    res = T.DecodeDHCP(parser, db, dr)
    gm, go = res.to_host()
    nopt = np.array(EDGE_NOPT)[np.arange(cand) % 5]
    assert res.count == cand and res.n_options == int(nopt.sum())
    assert np.array_equal(gm["first_opt"], np.concatenate([[0], np.cumsum(nopt)[:-1]]).astype(np.uint32))
    assert np.array_equal(gm["n_opts"], nopt.astype(np.uint32))
    assert np.array_equal(gm["version"], np.array([4, 6, 6, 6, 4], np.uint8)[np.arange(cand) % 5])
    step = np.arange(cand) // 3 if noise else 0
    assert np.array_equal(gm["packet"], (np.arange(cand) + step).astype(np.uint32))
    wm, wo, _ = TC.expect(batch, _oracle(batch, parser))
    assert gm.tobytes() == wm.tobytes() and go.tobytes() == wo.tobytes()


def test_no_candidates_and_empty_batch(parser):
    from gopacket_amd import dhcp as T
    from gopacket_amd import parser as P
    res, gm, go, _ = _check(parser, TC.NOISE * 3)
    assert res.count == 0 and res.n_options == 0 and res.messages() == []
    empty = PacketBatch.from_packets([])
    res = T.DecodeDHCP(parser, P.DeviceBatch(empty, 0), P.DeviceResult(0, 0))
    assert res.count == 0 and res.messages() == []


# ---------------------------------------------------------------- 4. scans past their first round
def test_scans_past_their_first_round(parser):
    """The smallest candidate count that takes gpd_compact.h's scan over the block counts, and the
    two-level scan of the option counts (gpd_stream_util.h: one block sum per kCompactBlock
    messages, scanned by the same compact_scan), into a second round: SCAN_ROUND blocks of
    COMPACT_BLOCK candidates and one more, from the two headers' constants.  Minimal frames: a
    1-byte payload to port 67 (too short), a 4-byte DHCPv6 message (OK, no options) and DHCPv6
    messages of one and two options for the entry scan, with a non-DHCP packet after every fourth
    so that the compaction moves every index."""
    from gopacket_amd import dhcp as T
    csrc = lambda f: open(f"{ROOT}/gopacket_amd/csrc/{f}").read()
    block = int(re.search(r"kCompactBlock = (\d+);", csrc("gpd_compact.h")).group(1))
    rnd = int(re.search(r"c0 \+= (\d+)u", csrc("gpd_compact.h")).group(1))
    assert "kCompactBlock" in csrc("gpd_stream_util.h")  # the entry scan's blocks are the compaction's
    assert (block, rnd) == (T.COMPACT_BLOCK, T.SCAN_ROUND)
    cand = block * rnd + 1
    bodies = EDGE_MSGS[:4]
    tmpl = [E4(vm) for vm in bodies]
    tmpl.append(TC.eth(TC.ip4(TC.udp(b"x" * 4, dport=5000), 17)))
    slot = 64
    assert max(len(t) for t in tmpl) <= slot
    period = np.zeros((5, slot), np.uint8)
    for k, t in enumerate(tmpl):
        period[k, :len(t)] = np.frombuffer(t, np.uint8)
    n = cand + (cand - 1) // 4
    reps = (n + 4) // 5
    data = np.tile(period.reshape(-1), reps)[:n * slot].reshape(n, slot)
    kind = np.arange(n) % 5
    caplen = np.array([len(t) for t in tmpl], np.uint32)[kind]
    xid = (np.arange(n, dtype=np.uint32) * 40503) & 0xFFFF
    v6 = (kind >= 1) & (kind <= 3)
    data[v6, 44], data[v6, 45] = (xid >> 8)[v6], (xid & 0xFF)[v6]  # the transaction id's low bytes
    batch = PacketBatch.from_arrays(np.concatenate([data.reshape(-1), np.zeros(PAD, np.uint8)]),
                                    np.arange(n, dtype=np.uint64) * slot, caplen, data_len=n * slot)
    db, dr = _decode(parser, batch)
    res = T.DecodeDHCP(parser, db, dr)
    gm, go = res.to_host()
    pk = np.nonzero(kind != 4)[0]
    kd = kind[pk]
    nopt = np.array([0, 0, 1, 2], np.uint32)[kd]
    assert res.count == cand == len(pk) and res.n_options == int(nopt.sum()) and res.deferred == 0
    # every message record's fields, vectorised
    first = np.concatenate([[0], np.cumsum(nopt.astype(np.uint64))])
    assert np.array_equal(gm["packet"], pk.astype(np.uint32))
    assert (gm["data_off"] == 42).all() and np.array_equal(gm["data_len"], caplen[pk] - 42)
    assert np.array_equal(gm["first_opt"], first[:-1].astype(np.uint32)) and np.array_equal(gm["n_opts"], nopt)
    assert np.array_equal(gm["version"], np.where(kd == 0, 4, 6).astype(np.uint8))
    assert np.array_equal(gm["verdict"], np.where(kd == 0, R.E_V4_TOO_SHORT, R.OK).astype(np.uint8))
    assert np.array_equal(gm["truncated"], (kd == 0).astype(np.uint8))
    assert np.array_equal(gm["err_arg"], (kd == 0).astype(np.uint32))
    assert np.array_equal(gm["err_off"], np.where(kd == 0, 0, gm["data_len"]).astype(np.uint32))
    assert np.array_equal(gm["xid"], np.where(kd == 0, 0, 0xAB0000 | xid[pk]).astype(np.uint32))
    assert np.array_equal(gm["op"], (kd != 0).astype(np.uint8))
    assert np.array_equal(gm["mflags"], np.where(kd == 0, 0, R.F_CONTENTS).astype(np.uint8))
    for f in ("secs", "flags", "htype", "hlen", "hops", "reserved"):
        assert not gm[f].any(), f
    # every option entry's fields, vectorised: the first option of a message, then the second
    f0 = first[:-1][nopt >= 1].astype(np.int64)
    f1 = first[:-1][nopt == 2].astype(np.int64) + 1
    assert (go["off"][f0] == 4).all() and (go["off"][f1] == 10).all()
    assert np.array_equal(go["code"][f0], np.array([0, 0, 14, 8], np.uint16)[kd[nopt >= 1]]) and (go["code"][f1] == 14).all()
    assert np.array_equal(go["length"][f0], np.array([0, 0, 0, 2], np.uint16)[kd[nopt >= 1]]) and not go["length"][f1].any()
    # a strided sample and both ends against the model
    for j in list(range(0, cand, 99991)) + [block * rnd - 1, cand - 1]:
        i = int(pk[j])
        m = batch.packet(i)[42:]
        wm, wo = R.records(R.decode(4 if kd[j] == 0 else 6, m), len(m), 2048, packet=i, data_off=42, first_opt=int(first[j]))
        assert gm[j:j + 1].tobytes() == wm.tobytes()
        assert go[int(first[j]):int(first[j + 1])].tobytes() == wo.tobytes()


# ---------------------------------------------------------------- 5. the budget
@pytest.mark.parametrize("max_options", [3, 2048])
def test_budget_boundary(parser, max_options):
    """work == max_options decodes, one more is deferred, for both versions; an error inside the
    budget stays an error; a jumbo datagram of 5,000 Pad options is deferred at both budgets and
    then equals the model through messages() (the host walker)."""
    from gopacket_amd import dhcp as T
    k = max_options
    h = TC.bootp()
    msgs = [TC.pads(k - 1), TC.pads(k), (4, h + b"\x00" * (k - 1) + b"\x77"), (4, h + b"\x00" * k + b"\x77"),
            TC.empty_opts6(k), TC.empty_opts6(k + 1), (6, TC.empty_opts6(k - 1)[1] + b"\x00\x07\x00"),
            (6, TC.empty_opts6(k)[1] + b"\x00\x07\x00"), TC.pads(5000), TC.pads(k, end=False)]
    assert [R.decode(v, m).work for v, m in msgs] == [k, k + 1, k, k + 1, k, k + 1, k, k + 1, 5001, k]
    frames = TC.interleave([E4(vm) for vm in msgs])
    res, gm, go, models = _check(parser, frames, max_options=max_options)
    v = [int(x) for x in gm["verdict"]]
    D = R.DEFERRED
    assert v == [R.OK, D, R.E_V4_OPT_NO_DATA, D, R.OK, D, R.E_V6_OPT_NO_DATA, D, D, R.OK]
    assert list(gm["n_opts"]) == [k - 1, 0, k - 1, 0, k, 0, k - 1, 0, 0, k] and res.deferred == 5
    assert int(gm["data_len"][8]) == 5241 and int(gm["version"][8]) == 4 and not gm["err_off"][8] and not gm["mflags"][8]
    jumbo = res.messages()[8]
    assert jumbo.err is None and len(jumbo.Options) == 5000 and jumbo.Contents == msgs[8][1] and jumbo.Xid == 0xDEADBEEF
    batch = PacketBatch.from_packets(frames)
    for bad in (0, (1 << 16) + 1):
        with pytest.raises(Exception):
            T.DecodeDHCP(parser, *_decode(parser, batch), max_options=bad)
    assert T.DecodeDHCP(parser, *_decode(parser, batch), max_options=1 << 16).deferred == 0


# ---------------------------------------------------------------- 6. capacities
def test_capacities_exact_and_one_short(parser):
    from gopacket_amd import _lib
    from gopacket_amd import dhcp as T
    frames = TC.interleave([E4(vm) for vm in ALL_MESSAGES[:24]])
    batch = PacketBatch.from_packets(frames)
    db, dr = _decode(parser, batch)
    full = T.DecodeDHCP(parser, db, dr)  # (the sizing call with all capacities 0, then the exact one)
    need = (full.count, full.n_options)
    assert min(need) > 1
    want = full.to_host()
    with pytest.raises(_lib.GpdError) as e:  # the sizing call itself
        T.DecodeDHCP(parser, db, dr, caps=(0, 0))
    assert (e.value.counts["msgs"], e.value.counts["options"]) == need
    for k in range(2):
        caps = tuple(c - (1 if j == k else 0) for j, c in enumerate(need))
        with pytest.raises(_lib.GpdError) as e:
            T.DecodeDHCP(parser, db, dr, caps=caps)
        c = e.value.counts
        assert (c["msgs"], c["options"]) == need                        # the needs are reported
        again = T.DecodeDHCP(parser, db, dr, caps=need).to_host()       # and the retry succeeds
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, want))
    roomy = T.DecodeDHCP(parser, db, dr, caps=(need[0] + 3, need[1] + 5))
    assert (roomy.count, roomy.n_options) == need
    assert all(a.tobytes() == b.tobytes() for a, b in zip(roomy.to_host(), want))


# ---------------------------------------------------------------- 7. through the defragmentation
def test_fragmented_reply_through_defrag(parser):
    """A DHCPv4 reply over three IPv4 fragments goes through DefragBatch; its datagram batch,
    decoded with first layer IPv4, reaches DecodeDHCP with the result of the unfragmented packet."""
    from gopacket_amd import dhcp as T
    from gopacket_amd import parser as P
    from gopacket_amd.defrag import IPv4Fragments
    from gopacket_amd.ip4reasm import NewIPv4Defragmenter
    m = bytes.fromhex(TC.VEC["v4"][1]["hex"])
    dgram = TC.udp(m, sport=67, dport=68)
    cuts = (0, 96, 200, len(dgram))
    frags = [TC.eth(TC.ip4(dgram[a:b], 17, frag=(0x2000 if b < len(dgram) else 0) | (a // 8), ident=77))
             for a, b in zip(cuts, cuts[1:])]
    whole = TC.eth(TC.ip4(dgram, 17, ident=77))
    batch = PacketBatch.from_packets([TC.NOISE[0], frags[0], frags[2], TC.NOISE[1], frags[1]])
    db, dr = _decode(parser, batch)
    assert T.DecodeDHCP(parser, db, dr).count == 0  # a fragment's decode ends at Fragment
    out, cnt = IPv4Fragments(parser, db, dr)
    assert cnt == 3
    dg = NewIPv4Defragmenter(parser).DefragBatch(db, out, cnt)
    assert dg.ndgrams == 1
    p4 = P.NewDecodingLayerParser(L.LayerTypeIPv4)
    p4._mask = ALL
    dr4 = P.DeviceResult(dg.batch.n, 0)
    p4.decode_device(dg.batch, dr4)
    got = T.DecodeDHCP(p4, dg.batch, dr4)
    ref, gm, _, _ = _check(parser, [whole])
    a, b = got.to_host(), ref.to_host()
    assert got.count == 1 and int(a[0]["data_off"][0]) == 28 and int(b[0]["data_off"][0]) == 42
    a[0]["data_off"] = 42
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    o = got.messages()[0]
    TC.same_object(o, R.decode(4, m))
    assert o.YourClientIP == bytes([192, 168, 0, 123]) and len(o.Options) == 7


# ---------------------------------------------------------------- 8. BPF mask to DHCP
# `udp port 67 or udp port 68` over Ethernet/IPv4 as a classic BPF program: the ethertype, the
# protocol, no later fragment, then either port against 67 and 68
UDP_PORT_67_OR_68 = [
    (0x28, 0, 0, 12), (0x15, 0, 12, 0x0800), (0x30, 0, 0, 23), (0x15, 0, 10, 17), (0x28, 0, 0, 20),
    (0x45, 8, 0, 0x1FFF), (0xB1, 0, 0, 14), (0x48, 0, 0, 14), (0x15, 4, 0, 67), (0x15, 3, 0, 68), (0x48, 0, 0, 16),
    (0x15, 1, 0, 67), (0x15, 0, 1, 68), (0x06, 0, 0, 262144), (0x06, 0, 0, 0),
]


def test_bpf_keep_mask_then_select_then_dhcp(parser):
    """`udp port 67 or udp port 68` as a BPF keep mask, pcapwrite.select, decode, DecodeDHCP: the
    DHCPv4 messages of the batch, in order, equal to DecodeDHCP restricted to the kept packets."""
    from gopacket_amd import bpf as B
    from gopacket_amd import dhcp as T
    from gopacket_amd import parser as P
    from gopacket_amd import pcapwrite as PW
    msgs = ALL_MESSAGES[:36]
    enc = lambda k, vm: TC.ENCAPS["dot1q" if k % 4 == 3 else "eth_ip4_udp"](vm)
    frames = TC.interleave([enc(k, vm) for k, vm in enumerate(msgs)])
    batch = PacketBatch.from_packets(frames)
    db = P.DeviceBatch(batch, 0)
    f = B.NewBPFInstructionFilter([B.BPFInstruction(*i) for i in UDP_PORT_67_OR_68], parser)
    keep = f.match_device(db)
    sel, index = PW.select(parser, db, keep)
    dr = P.DeviceResult(sel.n, 0)
    parser.decode_device(sel, dr)
    res = T.DecodeDHCP(parser, sel, dr)
    kept = [frames[int(i)] for i in index.cpu().numpy()]
    sub = PacketBatch.from_packets(kept)
    wm, wo, models = TC.expect(sub, _oracle(sub, parser))
    gm, go = res.to_host()
    assert gm.tobytes() == wm.tobytes() and go.tobytes() == wo.tobytes()
    # the untagged DHCPv4 messages (the filter reads the ethertype at 12: no VLAN tag, no DHCPv6 port)
    assert [d for d, _ in models] == [m for k, (v, m) in enumerate(msgs) if v == 4 and k % 4 != 3]
    assert len(models) >= 20 and (gm["version"] == 4).all()
    whole = T.DecodeDHCP(parser, *_decode(parser, batch)).to_host()[0]
    pos = {int(i): j for j, i in enumerate(index.cpu().numpy())}
    sel_of_whole = [m for m in whole if int(m["packet"]) in pos]
    assert [int(m["verdict"]) for m in sel_of_whole] == [int(v) for v in gm["verdict"]]
    assert [pos[int(m["packet"])] for m in sel_of_whole] == [int(p) for p in gm["packet"]]
