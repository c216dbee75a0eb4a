"""Time gpd_ip4_defrag_run (the IPv4 defragmentation).

Inputs, resident in HBM:
  * 2^20 fragments as datagrams of 2, 8 and 45 in-order fragments with 1,480-byte payloads (the
    hand-off is built here without a decode: one 1,520-byte slot per packet, random bytes; a
    45-fragment datagram's last fragment carries 408 bytes, so that it ends at 65,528), every
    datagram on its own key, datagram after datagram;
  * the same with 10 % of the fragments swapped with their successor;
  * 2^22 frames of the traffic mix (synth.make_traffic_mix, 3 % fragments), decoded and handed
    over by gpd_ip4_fragments.

Per input, in one process, after warm-up, medians of 10 HIP-event times around whole calls:

  sizing     the sizing call: grouping (table, sort, heads), walk, scans, totals
  floor      the sizing call on a copy of the hand-off with every verdict set to TOO_SMALL: no
             record joins a group, so the table and the walk drop out; sort, heads and scans stay
  records    the call without a byte buffer: sizing + outcomes, datagram records, the new carry
  whole      the call with the byte buffer: records + the gather and the header patches
  gather     whole - records, and its bytes (payload read, datagram written, 16-byte pieces read)
             per second as a fraction of
  d2d        a device-to-device copy of the same volume timed in this process

One JSON line per input.  For the in-order-run A/B build a second tree with
tools/ab_flags_build.sh . DIR "-DGPD_IP4R_NO_RUN" and run DIR/tools/ip4reasm_time.py.

    python tools/ip4reasm_time.py [--small] [--no-mix]     (--small: 2^16 fragments, 2^18 frames)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import defrag as DF, ip4reasm as I, layers as L, synth  # noqa: E402
from gopacket_amd import parser as P  # noqa: E402

SLOT, PAY = 1520, 1480


def median_ms(fn, s, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return round(ms[len(ms) // 2], 4)


def built_handoff(n, per, reorder):
    """n fragments as datagrams of `per` in-order fragments; reorder: the fraction swapped with
    their successor inside a datagram."""
    nd = n // per
    n = nd * per
    j = np.tile(np.arange(per), nd)
    dgram = np.repeat(np.arange(nd, dtype=np.uint32), per)
    recs = np.zeros(n, DF.FRAG_DTYPE)
    last = j == per - 1
    pay = np.where(last & (per * PAY > 65528), 65528 - (per - 1) * PAY, PAY)
    recs["net_off"], recs["ihl"] = 14, 5
    recs["src"] = dgram.view(np.uint8).reshape(n, 4)
    recs["dst"] = [10, 0, 0, 2]
    recs["id"] = dgram & 0xFFFF
    recs["frag_offset"] = j * (PAY // 8)
    recs["length"] = pay + 20
    recs["payload_len"] = pay
    recs["flags"] = np.where(last, 0, 1)
    order = np.arange(n)
    if reorder:
        rng = np.random.default_rng(1)
        pick = np.nonzero((rng.random(n) < reorder) & ~last)[0]
        pick = pick[np.concatenate(([True], np.diff(pick) > 1))]  # no overlapping swaps
        order[pick], order[pick + 1] = order[pick + 1].copy(), order[pick].copy()
    recs = recs[order]
    recs["packet"] = np.arange(n)
    data = torch.randint(0, 256, (n * SLOT + 64,), dtype=torch.uint8, device="cuda")
    off = torch.arange(n, dtype=torch.int64, device="cuda").mul_(SLOT).to(torch.int32)
    cap = torch.full((n,), 34 + PAY, dtype=torch.int32, device="cuda")
    db = P.DeviceBatch.from_tensors(data, n * SLOT, off, cap)
    return db, torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda(), n


def measure(p, db, frags, cnt, head):
    s = torch.cuda.current_stream()
    d = I.NewIPv4Defragmenter(p)
    rejected = frags.clone()
    rejected.view(-1, 32)[:, 28] = DF.FRAG_TOO_SMALL
    rc, out = d._run(db, frags, cnt, None, 0, None, None, 0, None, None, None, 0, s)
    assert rc == 0, rc
    nd, _, nb, nl = out
    oc = torch.empty(max(cnt, 2) * 8, dtype=torch.uint8, device="cuda")
    dg = torch.empty(max(nd, 1) * 32, dtype=torch.uint8, device="cuda")
    m = max((nd + 15) // 16 * 16, 16)
    desc = torch.zeros(2 * m, dtype=torch.int32, device="cuda")
    byts = torch.empty((max(nb, 1) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    keep = I.NewIPv4Defragmenter(p)  # a defragmenter per mode: each call starts from the same (empty) lists

    def call(mode, fr=frags, dd=d):
        if mode == "sizing":
            rc, o = dd._run(db, fr, cnt, None, 0, None, None, 0, None, None, None, 0, s)
        elif mode == "records":
            rc, o = dd._run(db, fr, cnt, None, 0, oc, dg, nd, None, None, None, 0, s)
        else:
            rc, o = dd._run(db, fr, cnt, None, 0, oc, dg, nd, desc[:m], desc[m:], byts, nb, s)
        assert rc == 0, (rc, o)
        return o
    if nl:  # lists stay behind (the traffic mix): time the first call's work by discarding them again
        def fresh(mode):
            o = call(mode, dd=keep)
            keep.DiscardOlderThan(1 << 62)
            return o
    else:
        fresh = call
    for _ in range(2):
        call("sizing"), fresh("records"), fresh("whole"), call("sizing", rejected)
    sizing = median_ms(lambda: call("sizing"), s)
    floor = median_ms(lambda: call("sizing", rejected), s)
    records = median_ms(lambda: fresh("records"), s)
    whole = median_ms(lambda: fresh("whole"), s)
    vol = max(nb, 1 << 20)
    a, b = torch.empty(vol, dtype=torch.uint8, device="cuda"), torch.empty(vol, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b.copy_(a)
    d2d = median_ms(lambda: b.copy_(a), s)
    h = np.zeros(0)
    if nd:
        h = dg[:nd * 32].cpu().numpy().view(I.DGRAM_DTYPE)
    npieces = int(h["nfrags"].sum()) + nd if nd else 0
    gather_ms = whole - records
    gather_bytes = 2 * nb + 16 * npieces
    gather_tbs = gather_bytes / gather_ms / 1e9 if gather_ms > 0 else None
    d2d_tbs = 2 * vol / d2d / 1e9
    print(json.dumps({
        **head, "fragments": cnt, "datagrams": nd, "bytes": nb, "lists_left": nl,
        "ms_sizing": sizing, "ms_floor_no_groups": floor, "ms_records": records, "ms_whole": whole,
        "ms_gather_by_difference": round(gather_ms, 4), "ns_per_fragment_sizing": round(sizing * 1e6 / max(cnt, 1), 2),
        "gather_bytes": gather_bytes, "gather_tbs_moved": round(gather_tbs, 3) if gather_tbs else None,
        "d2d_bytes": vol, "d2d_ms": d2d, "d2d_tbs_moved": round(d2d_tbs, 3),
        "gather_over_d2d": round(gather_tbs / d2d_tbs, 3) if gather_tbs else None}), flush=True)
    d.close()
    keep.close()


def main():
    small = "--small" in sys.argv
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    n = 1 << (16 if small else 20)
    for reorder in (0.0, 0.1):
        for per in (2, 8, 45):
            db, frags, cnt = built_handoff(n, per, reorder)
            measure(p, db, frags, cnt, {"input": "built", "per_datagram": per, "reordered": reorder})
            del db, frags
            torch.cuda.empty_cache()
    if "--no-mix" not in sys.argv:
        batch = synth.make_traffic_mix(1 << (18 if small else 22), 0x5EED0011)
        db = P.DeviceBatch(batch, 0)
        dr = P.DeviceResult(batch.n, 0)
        p.decode_device(db, dr)
        frags, cnt = DF.IPv4Fragments(p, db, dr)
        torch.cuda.synchronize()
        measure(p, db, frags, cnt, {"input": "traffic_mix", "frames": batch.n})


if __name__ == "__main__":
    main()
