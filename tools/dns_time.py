"""Time gpd_dns_decode (the DNS message decode) over a batch resident in HBM and
decoded once, outside the timed span.  Two shapes:

  queries    2^20 Eth/IPv4/UDP queries, all DNS (four name lengths, IDs from a hash of i)
  mixed      2^20 packets of which 1 % are compressed 300-byte responses (a question, eight
             answers whose names are pointers, with CNAME, A and TXT rdata), the rest non-DNS UDP

Per shape, in one process, after 5 warm-up calls, the median and the minimum of 100 HIP-event
times around the whole call on its stream (the sizing kernels, the host synchronisation, the
emit kernel) into arrays of exactly the needed capacity, so one call is one decode;
`ms_sizing_call` is the call with all capacities 0 (everything but the emit kernel).  `host` is
the only comparison: gpd_dns_decode_host over the same messages, one after another on one core of
the same box through its C entry point (ctypes, buffers allocated once; the loop's own overhead
is timed with a 12-byte message and reported beside it).  One JSON line per shape.

    python tools/dns_time.py [--small]          (--small: 2^14 packets)
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dns_cases as DC  # noqa: E402
from gopacket_amd import dns as D, layers as L, parser as P  # noqa: E402
from gopacket_amd.batch import PAD, PacketBatch  # noqa: E402


def response_300():
    m = DC.hdr(1, 8) + DC.q(DC.name(b"www", b"a-rather-long-label-for-the-zone", b"example", b"org"))
    at = len(m) + 12  # the CNAME's rdata: the target the A records' names point to
    m += DC.rr(DC.ptr(12), 5, DC.name(b"edge", b"cdn-frontend-pool")[:-1] + DC.ptr(16))
    for k in range(6):
        m += DC.rr(DC.ptr(at), 1, bytes([192, 0, 2, k]))
    return m + DC.rr(DC.ptr(16), 16, b"\x3f" + b"t" * 63)


def tiled(frames, kinds, n, slot):
    period = np.zeros((len(frames), slot), np.uint8)
    for k, f in enumerate(frames):
        period[k, :len(f)] = np.frombuffer(f, np.uint8)
    data = period[kinds]
    ids = (np.arange(n, dtype=np.uint32) * 40503) & 0xFFFF
    data[:, 42], data[:, 43] = ids >> 8, ids & 0xFF
    caplen = np.array([len(f) for f in frames], np.uint32)[kinds]
    return PacketBatch.from_arrays(np.concatenate([data.reshape(-1), np.zeros(PAD, np.uint8)]),
                                   np.arange(n, dtype=np.uint64) * slot, caplen, data_len=n * slot)


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


def host_seconds(msgs, reps=1):
    """gpd_dns_decode_host over the messages, one core; buffers allocated once."""
    lib = D.dns_lib()
    bufs = [np.frombuffer(m, np.uint8) for m in msgs]
    ptrs = [b.ctypes.data_as(C.c_void_p) for b in bufs]
    lens = [len(m) for m in msgs]
    msg = np.zeros(1, D.MSG_DTYPE)
    ents, names = np.zeros(64, D.ENTRY_DTYPE), np.zeros(4096, np.uint8)
    pm, pe, pn = (a.ctypes.data_as(C.c_void_p) for a in (msg, ents, names))
    cnt = D.GpdDnsCounts()
    fn, ref = lib.gpd_dns_decode_host, C.byref(cnt)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        for p, ln in zip(ptrs, lens):
            fn(p, ln, 0, pm, pe, 64, pn, 4096, ref)
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best


def run(name, batch, reps=100, warm=5):
    n = batch.n
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(n, 0, records=True)
    p.decode_device(db, dr)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    first = D.DecodeDNS(p, db, dr)
    caps = (first.count, first.n_entries, first.name_bytes)
    msgs, entries, names = first.msgs, first.entries, first.names

    def call():
        rc, c = D._call(p, db, dr, D.MAX_WORK_DEFAULT, msgs, entries, names, caps, s)
        assert rc == 0 and c["msgs"] == caps[0], (rc, c)

    def sizing():
        rc, c = D._call(p, db, dr, D.MAX_WORK_DEFAULT, None, None, None, (0, 0, 0), s)
        assert c["msgs"] == caps[0]
    for _ in range(warm):
        call(), sizing()
    full = median_ms(call, s, reps)
    size = median_ms(sizing, s, reps)
    hm = first.to_host()[0]
    host_msgs = [batch.packet(int(m["packet"]))[int(m["data_off"]):int(m["data_off"]) + int(m["data_len"])] for m in hm]
    empty = host_seconds([DC.hdr()] * len(host_msgs))
    host = host_seconds(host_msgs)
    print(json.dumps({
        "shape": name, "n": n, "messages": caps[0], "entries": caps[1], "name_bytes": caps[2], "deferred": first.deferred,
        "packet_bytes": int(batch.caplen.sum()), "message_bytes": int(hm["data_len"].sum()),
        "ms_call": full[0], "ms_call_min": full[1], "ms_sizing_call": size[0],
        "messages_per_s": round(caps[0] / full[0] * 1e3), "packets_per_s": round(n / full[0] * 1e3),
        "host_s_one_core": round(host, 4), "host_s_loop_overhead": round(empty, 4),
        "host_messages_per_s": round(caps[0] / host), "call_over_host": round(full[0] / 1e3 / host, 5)}), flush=True)


if __name__ == "__main__":
    n = 1 << (14 if "--small" in sys.argv else 20)
    labels = (b"a", b"bcd", b"efghi", b"jk")
    queries = [DC.eth(DC.ip4(DC.udp(DC.hdr(1, flags=0x0100) + DC.q(DC.name(x, b"example", b"org"))), 17)) for x in labels]
    run("queries", tiled(queries, np.arange(n) % 4, n, 96))
    resp = DC.eth(DC.ip4(DC.udp(response_300(), sport=53, dport=40000), 17))
    other = DC.eth(DC.ip4(DC.udp(b"x" * 260, dport=5000), 17))
    kinds = (np.arange(n) % 100 == 50).astype(np.int64)
    run("mixed_1pct_responses", tiled([other, resp], kinds, n, 352))
