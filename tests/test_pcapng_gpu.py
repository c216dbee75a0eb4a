"""pcapng through the GPU (gpd_decode_pcapng, gpd_ngwalk.hip): with the block walk on the device
every result — packet count, stop, error text, the reader's next position and every decoded
field — equals the host walk's (gpd_pcapng.cpp, pinned to pcapgo's NgReader by
tests/test_pcapng.py), and the host walk's equals DecodeBatchHost of the indexed batch (the
existing path).  chunk_bytes = 65536 (32 walking segments per chunk), so captures of a few
hundred KiB span several chunks."""
import struct

import numpy as np
import pytest

import ng_synth as S
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.pcap import capture_array

pytestmark = pytest.mark.gpu
FIELDS = ("status", "layers", "net_hash", "tp_hash", "csum", "hdr_off")
CHUNK = 65536
_parsers = {}


def _parser():
    from gopacket_amd import parser as P
    if "p" not in _parsers:
        _parsers["p"] = P.NewDecodingLayerParser(L.LayerTypeEthernet, P.Ethernet(), P.Dot1Q(), P.IPv4(), P.IPv6(),
                                                 P.IPv6ExtensionSkipper(), P.TCP(), P.UDP(), P.VXLAN(), P.Payload(),
                                                 P.Fragment())
    return _parsers["p"]


def frames(n, seed, mixed=False):
    b = synth.make_mixed(n, seed=seed) if mixed else synth.make_imix(n, seed=seed)
    return [b.data[o:o + c].tobytes() for o, c in zip(b.offset.tolist(), b.caplen.tolist())]


def decode(raw, dw, flags=(False, False, False), steps=None, chunk=CHUNK):
    """(fields, n, stop, err, next position, walk counts) of DecodePcapNg over the capture; with
    `steps`, in bounded calls of those sizes (the last repeated) continued to the stop."""
    from gopacket_amd import pcapng
    cap = raw if isinstance(raw, np.ndarray) else capture_array(raw)
    rd = pcapng.NgReader(cap, pcapng.NgReaderOptions(*flags, device_walk=dw, chunk_bytes=chunk))
    p = _parser()
    if steps is None:
        res, n, stop, err = p.DecodePcapNg(rd, nthreads=8)
        got = {f: getattr(res, f)[:n].copy() for f in FIELDS}
        return got, n, stop, err, rd.pos(), pcapng.last_walk_counts()
    parts, total, counts, i = [], 0, np.zeros(8, np.int64), 0
    while True:
        m = steps[min(i, len(steps) - 1)]
        i += 1
        res, n, stop, err = p.DecodePcapNg(rd, max_n=m, nthreads=8)
        parts.append({f: getattr(res, f)[:n].copy() for f in FIELDS})
        counts += pcapng.last_walk_counts()
        total += n
        if stop != pcapng.STOP_LIMIT:
            break
        assert n == m
    got = {f: np.concatenate([q[f] for q in parts]) for f in FIELDS}
    return got, total, stop, err, rd.pos(), list(counts)


def same(a, b):
    assert a[1:5] == b[1:5]
    for f in FIELDS:
        assert np.array_equal(a[0][f], b[0][f]), f


def both(raw, flags=(False, False, False), chunk=CHUNK):
    """Device walk == host walk == DecodeBatchHost of the indexed batch; returns the device walk's."""
    from gopacket_amd import pcapng
    cap = raw if isinstance(raw, np.ndarray) else capture_array(raw)
    dev, host = decode(cap, 1, flags, chunk=chunk), decode(cap, 0, flags, chunk=chunk)
    same(dev, host)
    assert host[5][0] == 0  # the host walk sends no chunk through the device walk
    idx = pcapng.NgReader(cap, pcapng.NgReaderOptions(*flags)).ReadAll()
    assert (idx.batch.n, idx.stop, idx.err, idx.next_pos) == host[1:5]
    ref = _parser().DecodeBatchHost(idx.batch)
    for f in FIELDS:
        assert np.array_equal(host[0][f], getattr(ref, f)[:host[1]]), f
    return dev


def head(e="<", snaplen=0, comment=b""):
    return S.shb(e, (S.opt(1, comment, e) + S.END[e]) if comment else b"") + S.idb(e, 1, snaplen)


def test_imix_jumbo_and_empty_packets_stay_on_the_device():
    pk = frames(4096, 0x61)
    rng = np.random.default_rng(0x61)
    for i in rng.choice(4096, size=20, replace=False):  # a block longer than four segments
        pk[i] = pk[i] + bytes(rng.integers(0, 256, size=9000 - len(pk[i]), dtype=np.uint8))
    for i in rng.choice(4096, size=8, replace=False):
        pk[i] = b""
    raw = head() + b"".join(S.epb(p, ts=i) for i, p in enumerate(pk))
    got, n, stop, err, pos, c = both(raw)
    assert (n, stop, err, pos) == (4096, 1, None, len(raw))
    assert c[0] >= len(raw) // CHUNK and c[1] == 0 and c[2] == 0, c


def test_stitch_lanes_own_several_segments():
    """ng_stitch_kernel (gpd_segwalk.h seg_stitch_body): lane t of its one workgroup owns
    ceil(nseg / 1024) consecutive 2,048-byte segments, one with the 64 KiB chunks of the other
    tests.  Chunks of 4 MiB + 4 KiB have 2,050 segments: three a lane, the last owning lane one,
    the lanes behind it none; the capture's last chunk is shorter (two a lane).  Jumbo blocks
    make segments no header starts in, empty packets and a refuted speculation's re-walk
    (payloads that look like block headers) move the counts the lanes add up."""
    chunk = (1 << 22) + 4096
    pk = frames(28000, 0x62)
    rng = np.random.default_rng(0x62)
    for i in rng.choice(len(pk), size=40, replace=False):
        pk[i] = pk[i] + bytes(rng.integers(0, 256, size=9000 - len(pk[i]), dtype=np.uint8))
    for i in rng.choice(len(pk), size=16, replace=False):
        pk[i] = b""
    for i in rng.choice(len(pk), size=16, replace=False):  # an enhanced packet block's first words, as payload
        pk[i] = struct.pack("<IIIIIII", 6, 96, 0, 0, i, 64, 64) * 3
    raw = head() + b"".join(S.epb(p, ts=i) for i, p in enumerate(pk))
    assert 2 * chunk < len(raw) < 3 * chunk and (len(raw) - 2 * chunk) // 2048 > 1024
    got, n, stop, err, pos, c = both(raw, chunk=chunk)
    assert (n, stop, err, pos) == (len(pk), 1, None, len(raw))
    assert c[0] == 3 and c[1] == 0 and c[2] == 0, c


def test_block_header_at_every_position_around_a_chunk_edge():
    pk = frames(1400, 0x62, mixed=True)
    pk = [(p + bytes(64))[:64] for p in pk]           # 96-byte blocks
    body = b"".join(S.epb(p) for p in pk)
    rel = set()
    for lead in (52, 68):                              # an unknown block that sets the phase
        for pad in (0, 4, 8, 12):                      # ... and the section comment that moves it
            raw = head(comment=b"c" * (8 + pad)) + S.block(0xBAD, bytes(lead - 12), "<") + body
            from gopacket_amd import pcapng
            p0 = pcapng.NgReader(raw).pos()
            edge = (p0 & ~15) + CHUNK
            rel |= {p0 + lead + 96 * j - edge for j in range(675, 690)} & set(range(-12, 5, 4))
            got, n, stop, err, pos, c = both(raw)
            assert (n, stop, err, c[1], c[2]) == (1400, 1, None, 0, 0)
    assert rel == {-12, -8, -4, 0, 4}


def test_enhanced_simple_and_obsolete_blocks_with_a_dropped_interface():
    pk = frames(1500, 0x63)
    out = [S.shb(), S.idb("<", 1, 128), S.idb("<", 0, 0)]  # interface 1: LINKTYPE_NULL, dropped
    kept = 0
    for i, p in enumerate(pk):
        k = i % 5
        if k == 0:
            out.append(S.spb(p))                      # clipped to interface 0's snap length
        elif k == 1:
            out.append(S.pb(p, ifindex=0, ts=i))
        elif k == 2:
            out.append(S.epb(p, ifindex=1, ts=i))     # dropped, not counted
        else:
            out.append(S.epb(p, ifindex=0, ts=i))
        kept += k != 2
    raw = b"".join(out)
    got, n, stop, err, pos, c = both(raw)
    assert (n, stop, err, c[1]) == (kept, 1, None, 0)
    from gopacket_amd import pcapng
    idx = pcapng.NgReader(raw).ReadAll()
    simple = idx.batch.caplen[0::4][:50]
    assert simple.max() == 128 and (idx.length[0::4][:50] >= simple).all()
    # with ErrorOnMismatchingLinkType the first such packet stops the reader
    got, n, stop, err, pos, c = both(raw, (False, True, False))
    assert (n, err) == (2, "Link type of current interface is different from first one")


def test_big_endian_capture():
    pk = frames(1200, 0x64)
    raw = head(">") + b"".join((S.epb if i % 3 else S.pb)(p, ">", ts=i << 20) for i, p in enumerate(pk))
    got, n, stop, err, pos, c = both(raw)
    assert (n, stop, err, c[1], c[2]) == (1200, 1, None, 0, 0)


def test_unknown_block_types_interleaved():
    pk = frames(1200, 0x65)
    rng = np.random.default_rng(0x65)
    out = [head()]
    for i, p in enumerate(pk):
        out.append(S.epb(p, ts=i))
        if i % 3 == 0:
            typ = (4, 10, 0xBAD, 0x80000001)[i % 4]
            out.append(S.block(typ, bytes(rng.integers(0, 256, size=4 * int(rng.integers(0, 700)), dtype=np.uint8)), "<"))
    got, n, stop, err, pos, c = both(b"".join(out))
    assert (n, stop, err, c[1], c[2]) == (1200, 1, None, 0, 0)


def test_state_changing_blocks_hand_over_tails_only():
    pk = frames(1500, 0x66)
    out = [head()]
    out += [S.epb(p, ts=i) for i, p in enumerate(pk[:500])]
    out.append(S.idb("<", 1, 0, S.opt(2, b"late", "<") + S.END["<"]))    # a mid-capture interface
    out += [S.epb(p, ifindex=i & 1, ts=i) for i, p in enumerate(pk[500:900])]
    out.append(S.isb("<", 1, 5))
    out += [S.shb(">"), S.idb(">", 1, 0)]                               # a section in the other byte order
    out += [S.epb(p, ">", ts=i) for i, p in enumerate(pk[900:])]
    out.append(S.isb(">", 0, 77, S.opt(4, struct.pack(">Q", 600), ">") + S.END[">"]))  # dumpcap's last block
    raw = b"".join(out)
    got, n, stop, err, pos, c = both(raw)
    assert (n, stop, err, pos) == (1500, 1, None, len(raw))
    assert c[1] == 0 and c[2] == 3 and c[4] == 0, c   # tails at the 3 state-changing spots, no whole chunk


def test_blocks_the_reader_stops_at():
    pk = frames(700, 0x67)
    pk[-1] = pk[-1][:60]                              # (a short last block: it is cut below)
    blocks = [S.epb(p, ts=i) for i, p in enumerate(pk)]
    k = 611

    def with_block(b):
        return head() + b"".join(blocks[:k]) + b + b"".join(blocks[k + 1:])

    got, n, stop, err, pos, c = both(with_block(S.epb(pk[k], ifindex=7)))
    assert (n, err) == (k, "Interface id 7 not present in section (have only 1 interfaces)")
    got, n, stop, err, pos, c = both(with_block(S.epb(pk[k], caplen=len(pk[k]) + 9)))
    assert (n, err) == (k, "bufio: negative count")
    got, n, stop, err, pos, c = both(with_block(S.epb(pk[k], caplen=(len(pk[k]) + 3 & ~3) + 3)))
    assert (n, err) == (700, None)                    # reaches into the trailing length: the reader takes it
    for total in (0, 4, 8):
        got, n, stop, err, pos, c = both(with_block(S.epb(pk[k], total=total)))
        assert (n, err) == (k, "EOF")
    bad = S.epb(pk[k] + b"xyz")                       # a total length that is no multiple of 4
    bad = bad[:4] + struct.pack("<I", len(bad) - 3) + bad[8:-7] + bad[-4:]
    both(with_block(bad))
    # one block cut at every 4th byte
    raw = head() + b"".join(blocks)
    start = len(raw) - len(blocks[-1])
    for cut in range(start, len(raw), 4):
        got, n, stop, err, pos, c = both(raw[:cut])
        assert n == 699 and (stop, err) == ((1, None) if cut == start else (2, "EOF"))


def test_payloads_that_are_pcapng_streams():
    eth = frames(8, 0x68, mixed=True)
    inner = b"".join(S.epb(bytes([i]) * 16, ts=i) for i in range(60))   # 48-byte blocks, 4-byte aligned
    pk = []
    for i in range(120):
        h = (eth[i % 8] + bytes(44))[:44]             # 44: the inner blocks start 4-byte aligned in the file
        pk.append(h + inner)
    raw = head() + b"".join(S.epb(p, ts=i) for i, p in enumerate(pk))
    got, n, stop, err, pos, c = both(raw)
    assert (n, stop, err) == (120, 1, None)
    assert c[1] == 0 and c[7] > 0, c                  # refuted speculations, corrected on the device


def test_bounded_calls_continue_exactly():
    pk = frames(2500, 0x69)
    out = [head()] + [S.epb(p, ts=i) for i, p in enumerate(pk[:1300])]
    out.append(S.idb("<", 1, 0))
    out += [S.epb(p, ifindex=1, ts=i) for i, p in enumerate(pk[1300:])]
    out.append(S.isb("<", 0, 1))
    raw = capture_array(b"".join(out))
    whole = both(raw)
    assert whole[1] == 2500
    for dw in (1, 0):
        same(decode(raw, dw, steps=[1, 63, 1000, 7, 1 << 20]), whole)
        same(decode(raw, dw, steps=[1299, 1, 1, 600]), whole)


def test_decode_refuses_a_mixed_linktype_reader():
    from gopacket_amd import pcapng
    from gopacket_amd._lib import GpdError
    rd = pcapng.NgReader(head() + S.epb(b"x" * 60), pcapng.NgReaderOptions(WantMixedLinkType=True))
    with pytest.raises(GpdError, match="want_mixed_linktype"):
        _parser().DecodePcapNg(rd)
