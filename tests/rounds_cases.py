"""TEST INFRASTRUCTURE ONLY: inputs and expectations for tests/test_rounds_gpu.py, the tests that
drive every single-workgroup multi-round loop of the pipeline past its first round.

Such a loop takes its input in rounds of R items (blocks of B) and carries a running total from
one round to the next; an input below R never executes the carry.  The constants below mirror
the kernels' (source line named beside each), the sizes are expressions of them, and nothing
here loops over packets or segments in Python: a small pool of distinct items is built with the
existing builders, an index array picks from it (`data = pool[idx]`), and an expectation is the
project's oracle on the pool (or on one period), expanded with numpy."""
from __future__ import annotations

import numpy as np

import pcapngwrite_ref as NR
import pcapwrite_ref as WR
from gopacket_amd.batch import PAD, PacketBatch

# ---- the kernels' constants -------------------------------------------------------------------
COMPACT_BLOCK = 2048                        # gpd_compact.h:18 kCompactBlock
COMPACT_ROUND = 1024 * COMPACT_BLOCK        # gpd_compact.h:56 `c0 += 1024u` block counts a round
SORT_TILE = 8192                            # gpd_radix_sort.h:30 kSortTile (tcpassembly.SORT_TILE)
SORT_ROUND = 16384 // 256 * SORT_TILE       # gpd_radix_sort.h:32 kSortScanRound of hist[256][ntile]: the
#                                             one scan of the hand-off, the tracker and reassembly
WRITE_BLOCK = 1024                          # gpd_pcapwrite.hip:47, gpd_pcapngwrite.hip:53 kScanBlock
WRITE_ROUND = 1024 * WRITE_BLOCK            # gpd_pcapwrite.hip:185, gpd_pcapngwrite.hip:186 `c * 1024u + t`


def sizes(R, B):
    """One full round with a full last block; a second round of one block of one item; a third
    round with a partial last block, reached with a carry that was built from a carry."""
    return (R, R + 1, 2 * R + 3 * B + 5)


def rounds(n, R):
    return (n + R - 1) // R


def place(n, R, B, variant, seed, rate=1000):
    """A boolean mask over n items: where the kept / interesting ones go.

    "edges": item 0 and n - 1, both sides of a block edge (B - 1, B), of the first round edge
    (R - 1, R) and of the second (2R - 1, 2R), one block that is entirely kept in the first round
    and one in the third, and a seeded 1-in-`rate` sprinkle elsewhere.
    "gap": the same without anything in [R, 2R): a whole round through which a nonzero carry
    must pass unchanged; R - 1 and 2R are kept."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, rate, n) == 0
    for p in (0, n - 1, B - 1, B, R - 1, R, 2 * R - 1, 2 * R):
        if 0 <= p < n:
            m[p] = True
    m[3 * B:4 * B] = True
    if n > 2 * R + 2 * B:
        m[2 * R + B:2 * R + 2 * B] = True
    if variant == "gap":
        assert n > 2 * R
        m[R:2 * R] = False
    else:
        assert variant == "edges"
    return m


def tile_frames(pool_frames, idx, stride=64):
    """The batch whose packet i is pool_frames[idx[i]], at i * stride."""
    pool = np.zeros((len(pool_frames), stride), np.uint8)
    lens = np.zeros(len(pool_frames), np.uint32)
    for k, f in enumerate(pool_frames):
        assert len(f) <= stride
        pool[k, :len(f)] = np.frombuffer(f, np.uint8)
        lens[k] = len(f)
    n = len(idx)
    data = np.zeros(n * stride + PAD, np.uint8)
    data[:n * stride].reshape(n, stride)[:] = pool[idx]
    return PacketBatch(data, n * stride, (np.arange(n, dtype=np.uint64) * np.uint64(stride)).astype(np.uint32),
                       lens[idx])


# ---- the writers ------------------------------------------------------------------------------
_CHUNK = 1 << 18


def _put_rows(out, pos, rows):
    """out[pos[i]:pos[i] + w] = rows[i] for rows of one width w."""
    ar = np.arange(rows.shape[1])
    for c0 in range(0, len(pos), _CHUNK):
        out[pos[c0:c0 + _CHUNK, None] + ar] = rows[c0:c0 + _CHUNK]


def _put_ragged(out, pos, data, off, ln):
    """out[pos[i]:pos[i] + ln[i]] = data[off[i]:off[i] + ln[i]]: one fancy copy per distinct
    length (the writers' packets have 41 of them)."""
    for L in np.unique(ln):
        if L == 0:
            continue
        sel = np.nonzero(ln == L)[0]
        ar = np.arange(int(L))
        for c0 in range(0, len(sel), _CHUNK):
            s = sel[c0:c0 + _CHUNK]
            out[pos[s, None] + ar] = data[off[s, None] + ar]


def _kept_before_bad(n, keep, reject):
    kept = np.ones(n, bool) if keep is None else np.asarray(keep) != 0
    rej = np.nonzero(kept & reject)[0]
    bad = int(rej[0]) if len(rej) else None
    idx = np.nonzero(kept)[0]
    return (idx if bad is None else idx[idx < bad]), bad


def _in_range(batch):
    off, cap = batch.offset.astype(np.int64), batch.caplen.astype(np.int64)
    assert int((off + cap).max(initial=0)) <= batch.data_len  # (no descriptor needs the clamp)
    return off, cap


def pcap_stream(batch, ts_ns, length=None, keep=None, nanos=False, header=None):
    """pcapwrite_ref.write's (stream, records written, bad index or NO_BAD) with numpy, the stream
    as a uint8 array: 16 header bytes and the packet's bytes per kept packet in front of the first
    kept one with capture length > length."""
    off, cap = _in_range(batch)
    wl = cap if length is None else np.asarray(length).astype(np.int64)
    idx, bad = _kept_before_bad(batch.n, keep, cap > wl)
    c = cap[idx]
    size = 16 + c
    base = 24 if header is not None else 0
    pos = base + np.cumsum(size) - size
    out = np.zeros(base + int(size.sum()), np.uint8)
    if header is not None:
        out[:24] = np.frombuffer(WR.file_header(header[0], header[1], nanos), np.uint8)
    t = np.asarray(ts_ns, np.uint64)[idx]
    e9 = np.uint64(1000000000)
    hdr = np.empty((len(idx), 4), "<u4")
    hdr[:, 0] = (t // e9) & np.uint64(0xFFFFFFFF)
    hdr[:, 1] = (t % e9) // np.uint64(1 if nanos else 1000)
    hdr[:, 2] = c
    hdr[:, 3] = wl[idx] & 0xFFFFFFFF
    _put_rows(out, pos, hdr.view(np.uint8).reshape(len(idx), 16))
    _put_ragged(out, pos + 16, batch.data, off[idx], c)
    return out, len(idx), WR.NO_BAD if bad is None else bad


def ng_stream(batch, ts_ns, length=None, ifindex=None, n_ifaces=1, keep=None, prefix=b""):
    """pcapngwrite_ref.write's (stream, records written, bad index or NO_BAD, BAD_* reason) with
    numpy: an enhanced packet block of 28 header bytes, the packet's bytes padded to 4 and the
    total length again per kept packet in front of the first rejected kept one."""
    off, cap = _in_range(batch)
    wl = cap if length is None else np.asarray(length).astype(np.int64)
    ifx = np.zeros(batch.n, np.int64) if ifindex is None else np.asarray(ifindex).astype(np.int64)
    idx, bad = _kept_before_bad(batch.n, keep, (ifx >= n_ifaces) | (cap > wl))
    c = cap[idx]
    total = 32 + c + ((-c) & 3)
    pos = len(prefix) + np.cumsum(total) - total
    out = np.zeros(len(prefix) + int(total.sum()), np.uint8)
    out[:len(prefix)] = np.frombuffer(bytes(prefix), np.uint8)
    t = np.asarray(ts_ns, np.uint64)[idx]
    hdr = np.empty((len(idx), 7), "<u4")
    hdr[:, 0] = 6
    hdr[:, 1] = total
    hdr[:, 2] = ifx[idx]
    hdr[:, 3] = t >> np.uint64(32)
    hdr[:, 4] = t & np.uint64(0xFFFFFFFF)
    hdr[:, 5] = c
    hdr[:, 6] = wl[idx] & 0xFFFFFFFF
    _put_rows(out, pos, hdr.view(np.uint8).reshape(len(idx), 28))
    _put_ragged(out, pos + 28, batch.data, off[idx], c)
    _put_rows(out, pos + total - 4, hdr[:, 1:2].copy().view(np.uint8).reshape(len(idx), 4))
    why = NR.BAD_NONE if bad is None else (NR.BAD_IFACE if ifx[bad] >= n_ifaces else NR.BAD_LENGTH)
    return out, len(idx), NR.NO_BAD if bad is None else bad, why


def prefix_batch(batch, k):
    """The first k packets as their own batch over the same data buffer."""
    return PacketBatch(batch.data, batch.data_len, batch.offset[:k].copy(), batch.caplen[:k].copy())


class WriterInput:
    """n packets of caplen 0..40 (zero included) at random places of one small data buffer, with
    capture infos for both formats.  `bad` is a packet of the third round (when there is one)
    whose length in `length_bad` is one below its capture length."""

    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        size = 4096
        data = rng.integers(0, 256, size + PAD, dtype=np.uint8)
        cap = rng.integers(0, 41, n).astype(np.uint32)
        cap[:41] = np.arange(41)  # every length is present (and in the 5,000-packet prefix)
        self.bad = 2 * WRITE_ROUND + WRITE_BLOCK + 17 if n > 2 * WRITE_ROUND + 2 * WRITE_BLOCK else n // 2
        cap[self.bad] = 7
        off = rng.integers(0, size - 40, n).astype(np.uint32)
        self.batch = PacketBatch(data, size, off, cap)
        self.n = n
        self.ts = rng.integers(0, 1 << 62, n).astype(np.uint64)                 # pcap: seconds below 2^32
        self.ts_raw = rng.integers(0, 1 << 64, n, dtype=np.uint64)              # pcapng: raw bit patterns
        self.length = cap + rng.integers(0, 3, n).astype(np.uint32)
        self.length_bad = self.length.copy()
        self.length_bad[self.bad] = 6
        self.ifindex = rng.integers(0, 3, n).astype(np.uint32)

    def mask(self, name):
        """The keep mask `name` (None: every packet): "all"; "first" / "last" (one packet);
        "round2" (nothing kept in the first two rounds); "edges" / "gap" (place()); "bad" ("edges"
        with the rejected packet kept)."""
        n, R, B = self.n, WRITE_ROUND, WRITE_BLOCK
        z = np.zeros(n, np.uint8)
        if name == "all":
            return None
        if name == "first":
            z[0] = 1
        elif name == "last":
            z[n - 1] = 1
        elif name == "round2":  # nothing in rounds 0 and 1: `first` travels back across two chunks
            for p in (2 * R + 5, 2 * R + B - 1, 2 * R + B, n - 1):
                z[p] = 1
        elif name in ("edges", "gap"):
            z = place(n, R, B, name, 0x5EED0760).astype(np.uint8)
            z[self.bad] = 0
        elif name == "bad":  # the rejected packet is kept: the stream ends in front of it
            z = place(n, R, B, "edges", 0x5EED0761).astype(np.uint8)
            z[self.bad] = 1
        else:
            raise ValueError(name)
        return z


# ---- the IPv4 fragment hand-off -----------------------------------------------------------------
def frag_pool():
    """(frames, is_fragment): 64-byte Eth/IPv4/UDP frames that are not fragments and a frame with
    DontFragment (GPD_FRAG_WHOLE: DefragIPv4 returns it unchanged, no record), then one fragment
    per verdict securityChecks can give — TOO_SMALL, OFFSET, and INSERT as a first, a middle and
    a last fragment; the OVERRUN check is a uint16 sum that never exceeds 65535 (defrag_ref.py),
    so the frame at the highest admitted offset stands for it and is an INSERT too."""
    from gopacket_amd import synth
    from test_defrag import ip4_frame
    plain = synth.make_udp64(24)
    frames = [plain.packet(i) for i in range(plain.n)]
    frames.append(ip4_frame(50, 2, 0, 0x0D0F, proto=17))          # DF
    frames.append(ip4_frame(50, 3, 0, 0x0D10, proto=17))          # DF | MF: DF wins
    nplain = len(frames)
    frames.append(ip4_frame(27, 1, 0, 0x7001, proto=17))          # TOO_SMALL (7 < 8)
    frames.append(ip4_frame(50, 1, 8184, 0x7002, proto=17))       # OFFSET (8184 > 8183)
    frames.append(ip4_frame(50, 1, 8183, 0x7003, proto=17))       # the highest offset: INSERT
    frames.append(ip4_frame(50, 1, 0, 0x7004, proto=17))          # first
    frames.append(ip4_frame(50, 1, 3, 0x7004, proto=17))          # middle
    frames.append(ip4_frame(46, 0, 6, 0x7004, proto=17))          # last
    frames.append(ip4_frame(44, 1, 2, 0x7005, proto=1, tags=1))   # behind an 802.1Q tag
    return frames, np.arange(len(frames)) >= nplain


def frag_index(kept, is_frag, seed):
    """Pool indices for a batch whose packet i is a fragment exactly where kept[i]."""
    rng = np.random.default_rng(seed)
    plain, frag = np.nonzero(~is_frag)[0], np.nonzero(is_frag)[0]
    idx = plain[rng.integers(0, len(plain), len(kept))]
    at = np.nonzero(kept)[0]
    idx[at] = frag[rng.integers(0, len(frag), len(at))]
    idx[at[:len(frag)]] = frag  # every fragment kind is present
    return idx


def expand_by_packet(pool_recs, npool, idx):
    """Records of a tiled batch from the oracle's records of the pool (at most one per pool
    frame, field `packet` = the pool index): packet i gets pool frame idx[i]'s record, if any,
    with `packet` set to i, in index order."""
    slot = np.full(npool, -1, np.int64)
    slot[pool_recs["packet"]] = np.arange(len(pool_recs))
    s = slot[idx]
    at = np.nonzero(s >= 0)[0]
    out = pool_recs[s[at]]
    out["packet"] = at
    return out


# ---- the TCP segment hand-off -------------------------------------------------------------------
FLOW_NONE, FLOW_FULL, FLOW_COLLISION = 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000


def flow_ids(kind, n, bound, seed):
    """Host flow ids for n segments.  "hot": a few ids carry almost everything (ids that differ
    in one bit of every digit the sort takes, and a sprinkle of others and of ids at or above
    the bound: the ungrouped tail), so the head flags are sparse and whole rounds of the head
    scan pass the carry on unchanged.  "distinct": every segment its own id, shuffled (needs
    bound > n), with a few at or above the bound: more groups than one round of the scan."""
    rng = np.random.default_rng(seed)
    if kind == "hot":
        hot = np.array([5, 5 | (1 << 8), 5 | (1 << 16), bound - 1, 0], np.uint64) % np.uint64(bound)
        fid = hot[rng.integers(0, len(hot), n)]
        rare = rng.integers(0, 5000, n) == 0
        fid[rare] = rng.integers(0, bound, int(rare.sum())).astype(np.uint64)
    elif kind == "distinct":
        assert bound > n
        fid = rng.permutation(n).astype(np.uint64)
    else:
        raise ValueError(kind)
    tail = np.array([bound, bound + 1, FLOW_FULL, 5 | FLOW_COLLISION, FLOW_NONE], np.uint64)
    t = rng.integers(0, 100000, n) == 0
    t[[n // 3, n - 1]] = True
    fid[t] = tail[rng.integers(0, len(tail), int(t.sum()))]
    return fid.astype(np.uint32)


# ---- the stream builders: a period of connections, tiled ------------------------------------------
# A period is a grouped hand-off over one small batch: `main` connections (flow ids 0 .. main - 1,
# in group order) and one more, the unit (flow id `main`).  The tiled hand-off is the main part k
# times and then the unit u times, every replica under flow ids of its own and all of them
# pointing at the period's packets (the kernels only gather from where a record points), so any
# exact number of groups or of segments is reached.  The connections do not depend on each other,
# so the expectation is the oracle's output for the period, tiled the same way: record indices,
# stream offsets and flow ids shifted by each replica's base.
SMALL_WEIGHTS = (0.05, 0.30, 0.30, 0.30, 0.04, 0.004, 0.002, 0.002, 0.002)  # tcpstream_cases.PAYLOAD_LENS


def _tiled(a, k, shifts):
    """a tiled k times; shifts: {field: (origin, step)}: replica j's field = a[field] - origin + j * step."""
    out = np.tile(a, k)
    rep = np.repeat(np.arange(k, dtype=np.int64), len(a))
    for f, (origin, step) in shifts.items():
        out[f] = np.tile(a[f].astype(np.int64) - origin, k) + rep * step
    return out


def _shift(a, fields):
    for f, base in fields.items():
        a[f] = a[f].astype(np.int64) + base
    return a


def tile_hand_off(segs, groups, main, k, u):
    """(segs, groups) of the tiled hand-off."""
    S, G, idbase, segbase = [], [], 0, 0
    for (g0, g1), reps in (((0, main), k), ((main, len(groups)), u)):
        if reps == 0:
            continue
        gs = groups[g0:g1]
        assert list(gs["flow_id"]) == list(range(g0, g1))
        s0, s1 = int(gs["start"][0]), int(gs["start"][-1]) + int(gs["count"][-1])
        ng, ns = g1 - g0, s1 - s0
        S.append(_shift(_tiled(segs[s0:s1], reps, {"flow_id": (g0, ng)}), {"flow_id": idbase}))
        G.append(_shift(_tiled(gs, reps, {"flow_id": (g0, ng), "start": (s0, ns)}),
                        {"flow_id": idbase, "start": segbase}))
        idbase += reps * ng
        segbase += reps * ns
    return np.concatenate(S), np.concatenate(G)


def tile_streams(recs, streams, byts, main, k, u, per_rec=()):
    """(recs, streams, bytes, [per_rec arrays]) of the tiled output, from the period's: streams
    are in group order, their records and bytes laid out one after another."""
    R, St, B, X = [], [], [], [[] for _ in per_rec]
    idbase = recbase = bytebase = 0
    for (g0, g1), reps in (((0, main), k), ((main, len(streams)), u)):
        if reps == 0:
            continue
        st = streams[g0:g1]
        assert list(st["flow_id"]) == list(range(g0, g1))
        r0, r1 = int(st["first_rec"][0]), int(st["first_rec"][-1]) + int(st["nrec"][-1])
        b0, b1 = int(st["byte_off"][0]), int(st["byte_off"][-1]) + int(st["nbytes"][-1])
        ng, nr, nb = g1 - g0, r1 - r0, b1 - b0
        R.append(_shift(_tiled(recs[r0:r1], reps, {"stream_off": (b0, nb)}), {"stream_off": bytebase}))
        St.append(_shift(_tiled(st, reps, {"flow_id": (g0, ng), "first_rec": (r0, nr), "byte_off": (b0, nb)}),
                         {"flow_id": idbase, "first_rec": recbase, "byte_off": bytebase}))
        B.append(np.tile(byts[b0:b1], reps))
        for x, a in zip(X, per_rec):
            x.append(np.tile(a[r0:r1], reps))
        idbase += reps * ng
        recbase += reps * nr
        bytebase += reps * nb
    return (np.concatenate(R), np.concatenate(St), np.concatenate(B)) + tuple(np.concatenate(x) for x in X)


def tile_by_id(a, main, k, u):
    """An array indexed by flow id (connection state), tiled."""
    return np.concatenate([np.tile(a[:main], k), np.tile(a[main:main + 1], u)])


def _short_groups(rng, n):
    """n connections of one or two segments: in order behind a SYN, without a SYN (drained with a
    gap), out of order, with FIN or RST, with a gap, and payloads of one to three pages."""
    from tcpstream_cases import FIN, RST, START_SEQS, SYN
    out = []
    for j in range(n):
        s = int(START_SEQS[rng.integers(len(START_SEQS))])
        a, b, g = (int((1, 3, 10, 40)[rng.integers(4)]) for _ in range(3))
        M = lambda v: v & 0xFFFFFFFF
        kind = j % 8
        if j == 5:
            out.append([(s, 0, 4000)])                       # three pages
        elif j == 13:
            out.append([(s, SYN, 0), (M(s + 1), 0, 1901)])   # two pages
        elif kind == 0:
            out.append([(s, SYN, 0), (M(s + 1), 0, a)])
        elif kind == 1:
            out.append([(s, 0, a)])
        elif kind == 2:
            out.append([(M(s + a + g), 0, b), (s, 0, a)])
        elif kind == 3:
            out.append([(s, SYN, 0), (M(s + 1), FIN, a)])
        elif kind == 4:
            out.append([(s, SYN, a)])
        elif kind == 5:
            out.append([(s, SYN, 0), (M(s + 1 + g), 0, b)])
        elif kind == 6:
            out.append([(s, RST, 0)])
        else:
            out.append([(M(s + a), 0, b), (s, SYN | FIN, a)])
    return out


def stream_period(shape, seed, main=64):
    """(batch, segs, groups, main) for gpd_tcp_assemble.  "long": tcpstream_cases.gen_groups'
    connections of up to 200 segments (in order, out of order, without SYN, FIN, RST, overlaps)
    with mostly small payloads, a few of several pages; "short": one or two segments each."""
    from tcpstream_cases import SYN, crafted, gen_groups
    if shape == "long":
        groups = gen_groups(seed, main, 200, SMALL_WEIGHTS)
    else:
        groups = _short_groups(np.random.default_rng(seed), main)
    batch, segs, grp = crafted(groups + [[(77, SYN, 3)]], interleave_seed=seed)
    assert len(grp) == main + 1
    return batch, segs, grp, main


def asm_period(seed, main=64):
    """Two runs for the stateful assembler over the same connections, each a (batch, segs, groups):
    run 1 leaves out-of-order pages behind a gap (one page, two pages, none; with and without a
    SYN), run 2 fills the gap, or adds behind it, or ends the connection.  Every connection has a
    segment in both runs."""
    from tcpstream_cases import FIN, START_SEQS, SYN, crafted
    rng = np.random.default_rng(seed)
    run1, run2 = [], []
    M = lambda v: v & 0xFFFFFFFF
    for j in range(main):
        s = int(START_SEQS[rng.integers(len(START_SEQS))])
        a, b, g = (int((1, 3, 10, 40)[rng.integers(4)]) for _ in range(3))
        kind = j % 8
        if j == 11:      # two pages carried, then delivered behind the fill
            run1.append([(s, SYN, 0), (M(s + 1 + g), 0, 1901)])
            run2.append([(M(s + 1), 0, g)])
        elif kind in (0, 1, 2):  # one page carried, then delivered behind the fill
            run1.append([(s, SYN, 0), (M(s + 1 + g), 0, b)])
            run2.append([(M(s + 1), 0, g)])
        elif kind == 3:  # in-order data first; the fill, then FIN
            run1.append([(s, SYN, 0), (M(s + 1), 0, a), (M(s + 1 + a + g), 0, b)])
            run2.append([(M(s + 1 + a), 0, g), (M(s + 1 + a + g + b), FIN, 0)])
        elif kind == 4:  # no SYN: the page waits with no sequence number; the SYN comes in run 2
            run1.append([(M(s + 1 + g), 0, b)])
            run2.append([(s, SYN, 0), (M(s + 1), 0, g)])
        elif kind == 5:  # the gap stays: a second page behind the first
            run1.append([(s, SYN, 0), (M(s + 1 + g), 0, b)])
            run2.append([(M(s + 1 + g + b), 0, a)])
        elif kind == 6:  # nothing carried
            run1.append([(s, SYN, 0), (M(s + 1), 0, a)])
            run2.append([(M(s + 1 + a), 0, b)])
        else:            # the fill overlaps the carried page
            run1.append([(s, SYN, 0), (M(s + 1 + g), 0, b)])
            run2.append([(M(s + 1), 0, g + 1)])
    run1.append([(5, SYN, 0), (9, 0, 2)])
    run2.append([(6, 0, 3)])
    return crafted(run1, interleave_seed=seed), crafted(run2, interleave_seed=seed + 1), main


# ---- the IPv4 reassembly: a period of datagrams, tiled ----------------------------------------------
# Every frame of a period is a fragment (packet index == record index) of at most 64 bytes with
# no 802.1Q tag, so a replica's key is changed in place: replica j has src[0] = 11 + (j >> 16),
# dst[0] = (j >> 8) & 255 and its ids XOR (j & 255), in the frames' bytes and in the records alike.
_ID_AT, _SRC_AT, _DST_AT = 14 + 4, 14 + 12, 14 + 16


def reasm_period(seed, nkeys=32):
    """(call 1 frames, call 2 frames, the unit's frame): datagrams of 2, 3 and 8 fragments, in
    order and permuted.  One in four is complete in call 1; the others hold a fragment back (the
    last, the first, one in the middle) for call 2, so their lists are carried; a fragment that is
    too small is rejected.  The unit is one fragment of a datagram that never completes."""
    from ip4reasm_cases import frames_of, in_order, interleave, key_of, spec
    from test_defrag import ip4_frame
    rng = np.random.default_rng(seed)
    g1, g2 = [], []
    for k in range(nkeys):
        nf = (2, 3, 8)[k % 3]
        fr = frames_of(rng, in_order(rng, nf, lo=1, hi=2, tail=int(rng.integers(8, 25))), key_of(k))
        if k % 2:
            fr = [fr[i] for i in rng.permutation(nf)]
        hold = {0: None, 1: nf - 1, 2: 0, 3: nf // 2}[k % 4]
        g1.append([f for i, f in enumerate(fr) if i != hold])
        if hold is not None:
            g2.append([fr[hold]])
    src, dst, ident = key_of(nkeys)
    g1.append([ip4_frame(27, 1, 0, ident, proto=17, src=src, dst=dst)])  # too small: rejected
    unit = frames_of(rng, [spec(0, 8, True)], key_of(nkeys + 1))
    return interleave(rng, g1), interleave(rng, g2), unit


def _replica_key_bytes(j):
    j = np.asarray(j, np.int64)
    return (11 + (j >> 16)).astype(np.uint8), ((j >> 8) & 255).astype(np.uint8), (j & 255).astype(np.uint16)


def reasm_input(parts, stride=64):
    """parts: [(frames, recs, replica ids)], recs the defrag oracle's records of `frames` (one per
    frame).  Returns (batch, FRAG_DTYPE records) with every replica's key its own."""
    rows, recs, rep = [], [], []
    pool, base, pbase = [], 0, 0
    for frames, r, ids in parts:
        assert list(r["packet"]) == list(range(len(frames)))
        k = len(ids)
        rows.append(np.tile(np.arange(len(frames)), k) + pbase)
        t = np.tile(r, k)
        t["packet"] = base + np.arange(k * len(frames))
        recs.append(t)
        rep.append(np.repeat(np.asarray(ids, np.int64), len(frames)))
        pool += frames
        base += k * len(frames)
        pbase += len(frames)
    rep = np.concatenate(rep)
    batch = tile_frames(pool, np.concatenate(rows), stride)
    recs = np.concatenate(recs)
    s0, d0, x = _replica_key_bytes(rep)
    m = batch.data[:batch.n * stride].reshape(batch.n, stride)
    m[:, _SRC_AT], m[:, _DST_AT] = s0, d0
    m[:, _ID_AT] ^= (x >> 8).astype(np.uint8)
    m[:, _ID_AT + 1] ^= (x & 255).astype(np.uint8)
    recs["src"][:, 0], recs["dst"][:, 0] = s0, d0
    recs["id"] ^= x
    return batch, recs


def reasm_expected(parts):
    """parts: [(RefResult of the part's frames, frames per replica, replica ids)].  Returns
    (outcomes, dgrams, offset, caplen, bytes) of the tiled call: indices shifted by each replica's
    base, the datagrams' header bytes given the replica's key and their checksum again."""
    import ip4reasm_ref as RR
    O_, D_, B_ = [], [], []
    pkt = dg = byt = 0
    for e, nfr, ids in parts:
        k, nd, nb = len(ids), len(e.dgrams), len(e.bytes)
        rep = np.asarray(ids, np.int64)
        o = np.tile(e.outcomes, k)
        done = o["what"] == RR.COMPLETE
        o["datagram"][done] += (dg + np.repeat(np.arange(k), len(e.outcomes)) * nd)[done].astype(np.uint32)
        d = _tiled(e.dgrams, k, {"packet": (0, nfr), "frag": (0, nfr), "byte_off": (0, nb)})
        d = _shift(d, {"packet": pkt, "frag": pkt, "byte_off": byt})
        s0, d0, x = _replica_key_bytes(np.repeat(rep, nd))
        d["id"] ^= x
        b = np.tile(e.bytes, k)
        if nd:
            assert (e.dgrams["ihl"] == 5).all()
            at = d["byte_off"].astype(np.int64) - byt
            b[at + 12], b[at + 16] = s0, d0
            b[at + 4] ^= (x >> 8).astype(np.uint8)
            b[at + 5] ^= (x & 255).astype(np.uint8)
            b[at + 10] = b[at + 11] = 0
            h = b[at[:, None] + np.arange(20)].astype(np.uint32)
            s = ((h[:, 0::2] << 8) | h[:, 1::2]).sum(axis=1)
            s = (s & 0xFFFF) + (s >> 16)
            s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
            b[at + 10], b[at + 11] = (s >> 8).astype(np.uint8), (s & 255).astype(np.uint8)
        O_.append(o)
        D_.append(d)
        B_.append(b)
        pkt += k * nfr
        dg += k * nd
        byt += k * nb
    outcomes, dgrams, byts = np.concatenate(O_), np.concatenate(D_), np.concatenate(B_)
    lens = np.concatenate([np.tile(e.caplen, len(ids)) for e, _, ids in parts])
    return outcomes, dgrams, dgrams["byte_off"].astype(np.uint32), lens.astype(np.uint32), byts
