"""Shared inputs of the IPv4 defragmentation tests (tests/test_ip4reasm.py,
tests/test_ip4reasm_gpu.py): fragment groups as real frames.

A fragment is described in the space the reference counts in: its byte offset `off` (a multiple
of 8) and L = Length - 20, which is what fragmentList.insert adds to Highest and Current
(defrag.go:253) whatever the IHL.  On the wire it carries Length - 4*IHL payload bytes."""
import numpy as np

from test_defrag import ip4_frame, vxlan_frame


def spec(off, L, mf, ihl=5, cap=None, len0=False):
    return {"off": off, "L": L, "mf": mf, "ihl": ihl, "cap": cap, "len0": len0}


def in_order(rng, n, ihl=5, lo=1, hi=8, tail=None):
    """n fragments back to back from offset 0; all but the last are multiples of 8 long."""
    out, off = [], 0
    for k in range(n):
        last = k == n - 1
        L = 8 * int(rng.integers(lo, hi + 1))
        if last:
            L = tail if tail is not None else int(rng.integers(8, 70))
        out.append(spec(off, L + (4 * (ihl - 5) if last and tail is None else 0), not last, ihl))
        off += out[-1]["L"]
    return out


def quirk_complete(k, ihl=5, cap=None):
    """[16k, 32k) first, [0, 24k) in front of it, [40k, 48k) last: Highest == Current == 48k with
    an overlap and a hole; build's `currentOffset + FragOffset*8` (:298) lands on 40k and the
    datagram completes with 40k payload bytes (IHL 5)."""
    return [spec(16 * k, 16 * k, True, ihl, cap), spec(0, 24 * k, True, ihl), spec(40 * k, 8 * k, False, ihl)]


def short_slice(ihl=6):
    """[a, 2a) first, [0, 2a) in front of it, [3a, 4a) last: the overlap's startAt is a = its
    Length-20, but with IHL > 5 its payload is 4*(IHL-5) bytes shorter: Payload[startAt:] is out
    of range.  a: the smallest multiple of 8 that securityChecks admits at this IHL."""
    a = 8 * ((8 + 4 * (ihl - 5) + 7) // 8)
    return [spec(a, a, True, ihl), spec(0, 2 * a, True, ihl), spec(3 * a, a, False, ihl)]


def invalid(k=1):
    """[8, 16) first, [0, 40k) in front, [40k + 8, 40k + 16) last: startAt > Length-20."""
    return [spec(8, 8, True), spec(0, 40 * k, True), spec(40 * k + 8, 8, False)]


def hole_then_piece():
    """[0, 16); [8, 16) counted but not stored; [24, 32) last: Highest == Current == 32 over a
    hole.  The list stays; [16, 24) arrives, and a duplicate of [0, 16) is still a duplicate."""
    return [spec(0, 16, True), spec(8, 8, True), spec(24, 8, False), spec(16, 8, True), spec(0, 16, True)]


def gen_group(rng, kind=None):
    """One key's fragments in arrival order."""
    kind = int(rng.integers(0, 14)) if kind is None else kind
    n = int(rng.integers(2, 13))
    if kind == 0:
        return in_order(rng, n)
    if kind == 1:  # permuted
        g = in_order(rng, n)
        return [g[i] for i in rng.permutation(n)]
    if kind == 2:  # duplicates
        g = in_order(rng, n)
        g = [g[i] for i in rng.permutation(n)]
        for _ in range(int(rng.integers(1, 4))):
            j = int(rng.integers(0, len(g)))
            g.insert(j, dict(g[int(rng.integers(0, j + 1))]))
        return g
    if kind == 3:
        return quirk_complete(int(rng.integers(1, 6)))
    if kind == 4:
        return invalid(int(rng.integers(1, 4)))
    if kind == 5:
        return hole_then_piece()
    if kind == 6:  # the first or the last fragment missing
        g = in_order(rng, n + 1)
        return g[1:] if rng.random() < 0.5 else g[:-1]
    if kind == 7:  # id reuse: two datagrams of one key, the second possibly out of order
        a, b = in_order(rng, n), in_order(rng, int(rng.integers(2, 6)))
        return a + [b[i] for i in rng.permutation(len(b))]
    if kind == 8:  # IHL 6-15 with options
        return in_order(rng, n, ihl=int(rng.integers(6, 16)), lo=6)
    if kind == 9:
        return short_slice(int(rng.integers(6, 16)))
    if kind == 10:  # a truncated capture under the quirk: the overlapping fragment loses its tail
        k = int(rng.integers(1, 4))
        return quirk_complete(k, cap=14 + 20 + int(rng.integers(0, 8 * k)))
    if kind == 11:  # Length 0 on the wire: DecodeFromBytes takes len(data) = 36, L = 16
        g = [spec(0, 16, True, len0=True), spec(16, 16, True, len0=True), spec(32, 24, False)]
        return [g[i] for i in rng.permutation(3)]
    if kind == 12:  # random overlaps and gaps
        g, off = [], 0
        for k in range(n):
            L = 8 * int(rng.integers(1, 6))
            g.append(spec(max(0, off + 8 * int(rng.integers(-2, 2))), L, k != n - 1))
            off = g[-1]["off"] + L
        return [g[i] for i in rng.permutation(n)]
    g = in_order(rng, n)  # a truncated plain fragment: fewer payload bytes than Length says
    j = int(rng.integers(0, n))
    g[j]["cap"] = 14 + 20 + int(rng.integers(0, 8))
    return g


def key_of(k):
    """Group k's (src, dst, id): neighbours differ only in src, only in dst, or only in id."""
    q, v = divmod(k, 4)
    src, dst, ident = [10, 1, q >> 8 & 255, q & 255], [10, 2, q >> 8 & 255, q & 255], (q * 7 + 1) & 0xFFFF
    if v == 1:
        src[1] = 3
    elif v == 2:
        dst[1] = 4
    elif v == 3:
        ident ^= 0x8000
    return tuple(src), tuple(dst), ident


def frames_of(rng, g, key, vxlan=False, proto=17):
    src, dst, ident = key
    out = []
    for s in g:
        ihl = s["ihl"]
        length = s["L"] + 20
        n_body = max(0, length - 4 * ihl)
        body = rng.integers(0, 256, n_body, dtype=np.uint8).tobytes()
        f = ip4_frame(0 if s["len0"] else length, 1 if s["mf"] else 0, s["off"] // 8, ident, proto=proto, ihl=ihl,
                      src=src, dst=dst, body=body, cap=s["cap"])
        out.append(vxlan_frame(f) if vxlan else f)
    return out


def interleave(rng, groups):
    """The groups' frames in one arrival order that keeps every group's own order."""
    left = [list(g) for g in groups]
    live = [k for k, g in enumerate(left) if g]
    out = []
    while live:
        j = int(rng.integers(0, len(live)))
        k = live[j]
        out.append(left[k].pop(0))
        if not left[k]:
            live.pop(j)
    return out


def random_frames(seed, ngroups, whole_every=7):
    """ngroups generated groups (every kind at least once when ngroups >= 14) as one interleaved
    list of frames, a few unfragmented and rejected frames among them."""
    rng = np.random.default_rng(seed)
    groups = []
    for k in range(ngroups):
        g = gen_group(rng, k if k < 14 else None)
        groups.append(frames_of(rng, g, key_of(k), vxlan=(k % 11 == 5)))
    frames = interleave(rng, groups)
    out = []
    for k, f in enumerate(frames):
        out.append(f)
        if k % whole_every == 0:
            out.append(ip4_frame(60, 0, 0, k & 0xFFFF, src=(9, 9, 9, 9), dst=(8, 8, 8, 8)))  # not a fragment
        if k % 29 == 3:
            out.append(ip4_frame(27, 1, 0, 5, src=(9, 9, 9, 9), dst=(8, 8, 8, 8)))           # too small
    return out
