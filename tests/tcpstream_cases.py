"""Shared inputs of the stream-assembly tests (tests/test_tcpstream.py, tests/test_tcpstream_gpu.py):
the generator of random segment groups, and hand-offs built straight from segment lists (a raw
batch whose packets are filler plus payload, with the SEG / GROUP records the segment hand-off
would give), so that tests of the assembly need neither frames nor a decode."""
from __future__ import annotations

import numpy as np

import tcpseg_ref as TS
from gopacket_amd.batch import PacketBatch

FIN, SYN, RST = 1, 2, 4
START_SEQS = (5, 1000, 1 << 31, (1 << 32) - 50)
PAYLOAD_LENS = (0, 1, 3, 10, 100, 1460, 1900, 1901, 4000)
PAYLOAD_WEIGHTS = (0.05, 0.12, 0.12, 0.25, 0.25, 0.10, 0.04, 0.04, 0.03)


def gen_group(rng, max_segments=200, weights=PAYLOAD_WEIGHTS):
    """One group of 1..max_segments segments as (seq, flags, payload_len): a start sequence from
    START_SEQS, payload lengths from PAYLOAD_LENS with `weights` (0 only with a flag); after each
    segment the next seq is in order (80 %), a gap of 1, 7 or 3000 (10 %) or a step back of 1, 2, 5
    or 2000 (10 %); 3 % FIN, 2 % RST, 2 % SYN mid-stream; then local swaps within 3 positions."""
    n = int(rng.integers(1, max_segments + 1))
    seq = int(START_SEQS[rng.integers(len(START_SEQS))])
    segs = []
    for i in range(n):
        plen = int(PAYLOAD_LENS[rng.choice(len(PAYLOAD_LENS), p=weights)])
        flags = 0
        u = rng.random()
        if i == 0 and rng.random() < 0.6:
            flags |= SYN
        elif u < 0.03:
            flags |= FIN
        elif u < 0.05:
            flags |= RST
        elif u < 0.07:
            flags |= SYN
        if plen == 0 and not flags:
            flags = (SYN, FIN, RST)[rng.integers(3)]
        segs.append((seq & 0xFFFFFFFF, flags, plen))
        seq += plen + (1 if (flags & SYN and i == 0) else 0)
        u = rng.random()
        if u < 0.10:
            seq += (1, 7, 3000)[rng.integers(3)]
        elif u < 0.20:
            seq -= (1, 2, 5, 2000)[rng.integers(4)]
    for _ in range(n // 8):
        a = int(rng.integers(n))
        b = min(n - 1, a + int(rng.integers(1, 4)))
        segs[a], segs[b] = segs[b], segs[a]
    return segs


def gen_groups(seed, ngroups, max_segments=200, weights=PAYLOAD_WEIGHTS):
    rng = np.random.default_rng(seed)
    return [gen_group(rng, max_segments, weights) for _ in range(ngroups)]


def crafted(groups, keys=None, interleave_seed=None, fill_seed=1):
    """A raw batch and the grouped hand-off for `groups` (lists of (seq, flags, payload_len)),
    group j on flow id keys[j] (ascending; default j).  Packets are in capture order: the
    groups' segments interleaved at random when interleave_seed is given, else group after group.
    Packet i is (23 + i % 29) filler bytes, then its payload.  Returns (batch, segs, groups)."""
    keys = list(range(len(groups))) if keys is None else list(keys)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    owner = [j for j, g in enumerate(groups) for _ in g]
    if interleave_seed is not None:
        owner = list(np.random.default_rng(interleave_seed).permutation(owner))
    rng = np.random.default_rng(fill_seed)
    nxt = [0] * len(groups)
    pk, per = [], [[] for _ in groups]
    for i, j in enumerate(owner):
        seq, flags, plen = groups[j][nxt[j]]
        nxt[j] += 1
        off = 23 + i % 29
        pk.append(rng.bytes(off + plen))
        per[j].append((i, keys[j], seq, 0, off, plen, off - 20, flags | 0x10, int(not flags & SYN and plen == 0),
                       (0, 0, 0)))
    segs = np.array([r for rs in per for r in rs], TS.SEG_DTYPE)
    grp, at = [], 0
    for j, rs in enumerate(per):
        if rs:
            grp.append((keys[j], at, len(rs), rs[0][0]))
            at += len(rs)
    return PacketBatch.from_packets(pk), segs, np.array(grp, TS.GROUP_DTYPE)
