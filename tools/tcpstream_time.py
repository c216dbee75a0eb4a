"""Time gpd_tcp_assemble (the TCP stream assembly) beside gpd_tcp_segments on the
batch of tools/tcpseg_time.py: 2^24 x 64-B Eth/IPv4/TCP frames resident in HBM, every one handed
over, with 2^10, 2^16 and 2^20 distinct connection keys.  Each key's segments are made one
in-order stream: its first packet carries SYN, the following ones the sequence numbers after it
(10 payload bytes each), so at 2^10 keys a group is 16K in-order segments and the wave's chain
run decides the walk's time.  Per key count, in one process, after warm-up, medians of 10
HIP-event times around whole calls on the call's stream:

  grouped    gpd_tcp_segments with the flow ids (the hand-off the assembly starts from)
  sizing     gpd_tcp_assemble's sizing call: page scan, walk, group scans, totals
  records    the call without a byte buffer: sizing + the records and streams placed
  whole      the call with the byte buffer: records + the gather
  gather     whole - records, and its bytes (payload read, stream written, 32-byte records read)
             per second as a fraction of
  d2d        a device-to-device copy of 1 GiB timed in this process

One JSON line per key count.  For the chain-run A/B build a second tree with
tools/ab_flags_build.sh . DIR "-DGPD_TSM_NO_CHAIN" and run DIR/tools/tcpstream_time.py.

--payload LEN times the assembly alone on a hand-off built without a decode: 2^20 packets of 54
filler bytes and LEN payload bytes (random, made on the device) in 16-byte-aligned slots, 2^16
keys, every key an in-order stream behind a SYN: the gather where a record spans many chunks.

    python tools/tcpstream_time.py [--small] [--keys LOG2 ...] [--payload LEN]   (--small: 2^18 packets)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import layers as L, synth  # noqa: E402
from gopacket_amd import parser as P, tcpassembly as T, tcpstream as S  # noqa: E402
from gopacket_amd.flows import NewFlowTable  # noqa: E402


def median_ms(fn, s, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return round(ms[len(ms) // 2], 4), round(ms[0], 4)


def with_streams(batch, log2_keys):
    """The batch with packet i's IPv4 source rewritten to one of 2^log2_keys values (as
    tools/tcpseg_time.py does) and each key's packets made one in-order stream: SYN on the key's
    first packet (its 10 bytes and the SYN take 11 sequence numbers), then
    seq = start + 1 + 10 * (packets of the key before it), in capture order.  The frames are
    64-byte rows with 10 payload bytes; checksums are not kept."""
    n = batch.n
    a = batch.data[:n * 64].reshape(n, 64)
    key = (synth.splitmix64(0x5EED0041, n, 7) % np.uint64(1 << log2_keys)).astype(np.uint32)
    a[:, 26:30] = key.byteswap().view(np.uint8).reshape(n, 4)
    a[:, 30:38] = a[0, 30:38]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    head = np.concatenate(([True], sk[1:] != sk[:-1]))
    first = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - first           # packets of the key before this one
    start = key.astype(np.int64) * 7919 + 1000   # the key's initial sequence number
    seq = (start + np.where(rank == 0, 0, 1 + 10 * rank)).astype(np.uint32)  # (the SYN's 10 bytes + 1)
    a[:, 38:42] = seq.byteswap().view(np.uint8).reshape(n, 4)
    a[:, 47] = np.where(rank == 0, 0x12, 0x10).astype(np.uint8)  # SYN|ACK on the first, ACK after
    return batch


def run(batch, log2_keys, reps=10):
    n = batch.n
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    db = P.DeviceBatch(with_streams(batch, log2_keys), 0)
    dr = P.DeviceResult(n, 0, records=True)
    p.decode_device(db, dr)
    table = NewFlowTable(p, 2 << log2_keys)
    ids = table.Insert(db, dr)
    torch.cuda.synchronize()
    bound = table.Stats()["capacity"]
    s = torch.cuda.current_stream()
    segs = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    groups = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    h = {}

    def handoff():
        rc, h["cnt"], h["ng"], h["un"] = T._call(p, db, dr, ids, bound, segs, groups, n, s)
        assert rc == 0, rc
    handoff()
    measure(p, db, segs, h["cnt"], groups, h["ng"], {"keys": 1 << log2_keys, "n": n}, handoff, reps)


def measure(p, db, segs, cnt, ng_groups, ng, head, handoff, reps):
    groups, s = ng_groups, torch.cuda.current_stream()
    rc, out = S._call(p, db, segs, cnt, groups, ng, None, 0, 0, False, None, 0, None, None, 0, s)
    assert rc == 0, rc
    nrecs, nstreams, nbytes, ncalls = out
    recs = torch.empty(max(nrecs, 1) * 32, dtype=torch.uint8, device="cuda")
    streams = torch.empty(max(ng, 1) * 48, dtype=torch.uint8, device="cuda")
    byts = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")

    def assemble(mode):
        r, b = (None, None) if mode == "sizing" else (recs, byts if mode == "whole" else None)
        rc, o = S._call(p, db, segs, cnt, groups, ng, None, 0, 0, False, r, nrecs if r is not None else 0,
                        streams if r is not None else None, b, nbytes if b is not None else 0, s)
        assert rc == 0 and o == out, (rc, o)
    for _ in range(2):
        handoff and handoff(), assemble("sizing"), assemble("records"), assemble("whole")
    grouped = median_ms(handoff, s, reps) if handoff else (None, None)
    sizing = median_ms(lambda: assemble("sizing"), s, reps)
    records = median_ms(lambda: assemble("records"), s, reps)
    whole = median_ms(lambda: assemble("whole"), s, reps)
    a, b = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"), torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b.copy_(a)
    d2d = median_ms(lambda: b.copy_(a), s, reps)
    st = S.streams_to_host(S.StreamResult(recs[:nrecs * 32], streams[:nstreams * 48], None, nrecs, nstreams, nbytes,
                                          ncalls)).streams
    gather_ms = whole[0] - records[0]
    gather_bytes = 2 * nbytes + 32 * nrecs
    d2d_tbs = 2 * (1 << 30) / d2d[0] / 1e9
    gather_tbs = gather_bytes / gather_ms / 1e9 if gather_ms > 0 else None
    print(json.dumps({
        **head, "segments": cnt, "groups": ng,
        "records": nrecs, "streams": nstreams, "stream_bytes": nbytes, "calls": ncalls,
        "open_streams": int(st["open"].sum()), "segments_per_group": round(cnt / max(ng, 1), 1),
        "ms_grouped": grouped[0], "ms_sizing": sizing[0], "ms_records": records[0], "ms_whole": whole[0],
        "ms_whole_min": whole[1], "ms_gather_by_difference": round(gather_ms, 4),
        "whole_over_grouped": round(whole[0] / grouped[0], 3) if handoff else None,
        "gather_bytes": gather_bytes, "gather_tbs_moved": round(gather_tbs, 3) if gather_tbs else None,
        "d2d_1gib_ms": d2d[0], "d2d_tbs_moved": round(d2d_tbs, 3),
        "gather_over_d2d": round(gather_tbs / d2d_tbs, 3) if gather_tbs else None}), flush=True)


def run_payload(plen, log2_n=20, log2_keys=16, reps=10):
    """The assembly alone over a hand-off built here: packet i belongs to key i mod 2^log2_keys."""
    n, K = 1 << log2_n, 1 << log2_keys
    slot = (54 + plen + 15) & ~15
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    data = torch.randint(0, 256, (n * slot + 64,), dtype=torch.uint8, device="cuda")
    off = torch.arange(n, dtype=torch.int64, device="cuda").mul_(slot).to(torch.int32)
    cap = torch.full((n,), 54 + plen, dtype=torch.int32, device="cuda")
    db = P.DeviceBatch.from_tensors(data, n * slot, off, cap)
    pkt = np.arange(n, dtype=np.uint32).reshape(n // K, K).T.reshape(-1)  # key after key, capture order inside
    rank = np.tile(np.arange(n // K, dtype=np.int64), K)
    key = np.repeat(np.arange(K, dtype=np.uint32), n // K)
    segs = np.zeros(n, T.SEG_DTYPE)
    segs["packet"], segs["flow_id"] = pkt, key
    segs["seq"] = (key.astype(np.int64) * 7919 + 1000 + np.where(rank == 0, 0, 1 + plen * rank)).astype(np.uint32)
    segs["payload_off"], segs["payload_len"], segs["tcp_off"] = 54, plen, 34
    segs["flags"] = np.where(rank == 0, 0x12, 0x10)
    groups = np.zeros(K, T.GROUP_DTYPE)
    groups["flow_id"], groups["start"], groups["count"] = np.arange(K), np.arange(K) * (n // K), n // K
    groups["first_packet"] = np.arange(K)
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
    measure(p, db, up(segs), n, up(groups), K, {"keys": K, "n": n, "payload": plen, "slot": slot}, None, reps)


if __name__ == "__main__":
    if "--payload" in sys.argv:
        run_payload(int(sys.argv[sys.argv.index("--payload") + 1]))
        sys.exit(0)
    n = 1 << (18 if "--small" in sys.argv else 24)
    keys = (10, 16, 20)
    if "--keys" in sys.argv:
        keys = [int(v) for v in sys.argv[sys.argv.index("--keys") + 1:] if v.isdigit()]
    batch = synth.make_tcp64(n)
    for k in keys:
        run(batch, k)
