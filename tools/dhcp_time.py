"""Time the DHCP message decode over data resident in HBM, decoded once outside the
timed span.  Two shapes:

  discover    2^20 Eth/IPv4/UDP frames from port 68 to 67, DISCOVER-sized DHCPv4 messages (four
              option lists of 6 to 9 options, the Xid from a hash of i): every packet a candidate
  one_percent 2^20 frames of which 1 in 100 is such a message (and one in 400 a DHCPv6 SOLICIT to
              port 547), the rest 64-byte UDP to another port: what a capture looks like

Per shape, in one process, after 10 warm-up calls, the median and the minimum of 100 HIP-event times
around the whole gpd_dhcp_decode call on its stream (the compaction, the locate step, the sizing
walk, the scan, the host synchronisation, the emit walk) into arrays of exactly the needed capacity;
`ms_sizing_call` is the call with all capacities 0 (everything but the emit kernel).  `host_1` is
gpd_dhcp_decode_host over the same messages on one core, message by message through ctypes (buffers
allocated once); `host_1_loop_overhead_s` is the same loop over empty messages, what the calling
loop itself costs.  One JSON line per shape.

    python tools/dhcp_time.py [--log2n 20] [--shape S] [--reps 100]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import dhcp_cases as TC  # noqa: E402
from gopacket_amd.batch import PAD, PacketBatch  # noqa: E402


# ---------------------------------------------------------------- the shapes
def discover_messages():
    """Four DHCPv4 messages of 6 to 9 options, 280 to 300 bytes."""
    h = TC.bootp()
    base = TC.o4(53, b"\x01") + TC.o4(61, b"\x01" + bytes(range(0x20, 0x26))) + TC.o4(50, bytes([10, 0, 0, 9]))
    tails = [TC.o4(12, b"host-a") + TC.o4(60, b"MSFT 5.0") + TC.o4(55, bytes([1, 3, 6, 15, 31, 33, 43, 44])),
             TC.o4(12, b"printer-12") + b"\x00" + TC.o4(55, bytes([1, 3, 6, 12, 15, 28, 42])) + TC.o4(57, b"\x05\xdc"),
             TC.o4(12, b"ap") + TC.o4(60, b"udhcp 1.30.1") + TC.o4(55, bytes([1, 3, 6, 12, 15, 28, 42, 121])) +
             TC.o4(57, b"\x02\x40") + b"\x00\x00",
             TC.o4(55, bytes(range(1, 17))) + TC.o4(81, b"\x00\x00\x00laptop.example.org") + TC.o4(60, b"dhcpcd-9")]
    return [(4, h + base + t + b"\xff") for t in tails]


def frame(vm):
    return TC.ENCAPS["eth_ip4_udp"](vm)


def tiled(frames, kinds, n, slot):
    period = np.zeros((len(frames), slot), np.uint8)
    for k, f in enumerate(frames):
        assert len(f) <= slot
        period[k, :len(f)] = np.frombuffer(f, np.uint8)
    data = period[kinds]
    caplen = np.array([len(f) for f in frames], np.uint32)[kinds]
    return PacketBatch.from_arrays(np.concatenate([data.reshape(-1), np.zeros(PAD, np.uint8)]),
                                   np.arange(n, dtype=np.uint64) * slot, caplen, data_len=n * slot)


def shape_batch(shape, n):
    """(batch, the distinct DHCP messages as (version, bytes))."""
    msgs = discover_messages()
    slot = 352
    if shape == "discover":
        frames = [frame(vm) for vm in msgs]
        kinds = np.arange(n) % 4
    else:
        msgs = msgs + [(6, TC.SOLICIT)]
        other = TC.eth(TC.ip4(TC.udp(bytes(22), dport=5000), 17))
        frames = [frame(vm) for vm in msgs] + [other]
        i = np.arange(n)
        kinds = np.where(i % 100 == 7, (i // 100) % 4, 5)
        kinds = np.where(i % 400 == 211, 4, kinds)
    batch = tiled(frames, kinds.astype(np.int64), n, slot)
    v = batch.data[:n * slot].reshape(n, slot)
    is4 = kinds < 4
    xid = (np.arange(n, dtype=np.uint32) * 40503) & 0xFFFF  # Xid's low bytes (46..49 of the frame is Xid)
    v[is4, 48], v[is4, 49] = (xid >> 8)[is4], (xid & 0xFF)[is4]
    return batch, msgs


# ---------------------------------------------------------------- the host walker on one core
def host_seconds(msgs, calls):
    """gpd_dhcp_decode_host `calls` times over the distinct messages in turn, on this core."""
    from gopacket_amd import dhcp as T
    lib = T.dhcp_lib()
    bufs = [np.frombuffer(m, np.uint8) for _, m in msgs]
    ptrs = [b.ctypes.data_as(C.c_void_p) if len(b) else None for b in bufs]
    lens = [len(m) for _, m in msgs]
    vers = [v for v, _ in msgs]
    msg, opts = np.zeros(1, T.MSG_DTYPE), np.zeros(64, T.OPT_DTYPE)
    pm, po = msg.ctypes.data_as(C.c_void_p), opts.ctypes.data_as(C.c_void_p)
    cnt = T.GpdDhcpCounts()
    fn, ref, k = lib.gpd_dhcp_decode_host, C.byref(cnt), len(msgs)
    t0 = time.perf_counter()
    for i in range(calls):
        j = i % k
        fn(vers[j], ptrs[j], lens[j], 0, pm, po, 64, ref)
    return time.perf_counter() - t0


# ---------------------------------------------------------------- timing
def median_ms(fn, s, reps):
    import torch
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


def run_shape(shape, log2n, reps, warm):
    import torch
    from gopacket_amd import dhcp as T, layers as L, parser as P
    n = 1 << log2n
    batch, msgs = shape_batch(shape, n)
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    s = torch.cuda.current_stream()
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(n, 0, records=True)
    p.decode_device(db, dr)
    torch.cuda.synchronize()
    b, r = db.c_batch(), dr.c_result()

    def call(m, o, caps):
        out = T.GpdDhcpOut(T._ptr(m), caps[0], T._ptr(o), caps[1])
        cnt = T.GpdDhcpCounts()
        rc = T.dhcp_lib().gpd_dhcp_decode(p.ctx().h, C.byref(b), C.byref(r), None, C.byref(out), C.byref(cnt),
                                          C.c_void_p(s.cuda_stream))
        return rc, T._counts(cnt)
    first = T.DecodeDHCP(p, db, dr)
    caps = (first.count, first.n_options)

    def full():
        rc, c = call(first.msgs, first.opts, caps)
        assert rc == 0 and c["msgs"] == caps[0], (rc, c)

    def sizing():
        rc, c = call(None, None, (0, 0))
        assert c["msgs"] == caps[0]
    for _ in range(warm):
        full(), sizing()
    t_full, t_size = median_ms(full, s, reps), median_ms(sizing, s, reps)
    verdicts = np.bincount(first.to_host()[0]["verdict"], minlength=11)[:11].tolist()
    torch.cuda.synchronize()
    host = host_seconds(msgs, first.count)
    empty = host_seconds([(4, b""), (6, b"")], first.count)
    print(json.dumps({
        "shape": shape, "n": n, "messages": first.count, "options": first.n_options, "deferred": first.deferred,
        "verdicts_0_to_10": verdicts, "input_bytes": int(batch.caplen.sum()), "reps": reps,
        "ms_call": t_full[0], "ms_call_min": t_full[1], "ms_sizing_call": t_size[0],
        "packets_per_s": round(n / t_full[0] * 1e3), "messages_per_s": round(first.count / t_full[0] * 1e3),
        "options_per_s": round(first.n_options / t_full[0] * 1e3),
        "host_1_s": round(host, 4), "host_1_loop_overhead_s": round(empty, 4),
        "host_1_messages_per_s": round(first.count / host)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--shape", choices=("discover", "one_percent"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warm", type=int, default=10)
    a = ap.parse_args()
    for shape in ([a.shape] if a.shape else ["discover", "one_percent"]):
        run_shape(shape, a.log2n, a.reps, a.warm)
