"""Time gpd_tcp_segments (the tcpassembly hand-off) on the tcp64 batch: 2^24 x 64-B
Eth/IPv4/TCP frames resident in HBM, every one handed over, with 2^10, 2^16 and 2^20 distinct
connection keys (the source address of packet i is rewritten to a hash of i modulo the key
count; ports and destination are one value).  Per key count, in one process, after warm-up,
medians of HIP-event times around whole calls on the call's stream:

  sizing     the sizing call: count + scan
  records    the call without flow ids: count + scan + index + record
  grouped    the call with the flow ids of gpd_flow_insert: records + sort passes + groups
  insert     gpd_flow_insert of the same batch into the table that already holds its keys
  host       the alternative the grouping replaces: flow_id device-to-host, then
             numpy.argsort(kind="stable") (host clock, 3 runs)
  d2d        a device-to-device copy of 1 GiB, the box's streaming rate this process reached

and the bytes each sort pass moves by the algorithm (8-byte pairs read by the histogram, read
and written by the scatter; the last scatter gathers and writes the 32-byte records and writes
the 4-byte keys).  One JSON line per key count.  The split of `grouped` into kernels comes from
a kernel trace of `--once K` (one warm call, one traced call), run under the profiler on its own.

    python tools/tcpseg_time.py [--small] [--once LOG2_KEYS]     (--small: 2^18 packets)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import layers as L, synth  # noqa: E402
from gopacket_amd import parser as P, tcpassembly as T  # noqa: E402
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


def with_keys(batch, log2_keys):
    """The batch with packet i's IPv4 source rewritten to one of 2^log2_keys values, and one
    destination and port pair for all (the frames are 64-byte rows; checksums are not kept)."""
    n = batch.n
    a = batch.data[:n * 64].reshape(n, 64)
    key = (synth.splitmix64(0x5EED0041, n, 7) % np.uint64(1 << log2_keys)).astype(np.uint32)
    a[:, 26:30] = key.byteswap().view(np.uint8).reshape(n, 4)
    a[:, 30:38] = a[0, 30:38]
    return batch


def sort_passes(bound):
    return max(1, (int(bound).bit_length() + 7) // 8)


def run(batch, log2_keys, reps=10, once=False):
    n = batch.n
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    db = P.DeviceBatch(with_keys(batch, log2_keys), 0)
    dr = P.DeviceResult(n, 0, records=True)
    p.decode_device(db, dr)
    table = NewFlowTable(p, 2 << log2_keys)
    ids = table.Insert(db, dr)
    torch.cuda.synchronize()
    st = table.Stats()
    bound = st["capacity"]
    s = torch.cuda.current_stream()
    segs = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    groups = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    res = {}

    def call(fid, out):
        rc, cnt, ng, un = T._call(p, db, dr, fid, bound, segs if out else None, groups if out else None,
                                  n if out else 0, s)
        assert rc == 0, rc
        res["cnt"], res["ng"], res["un"] = cnt, ng, un
    call(ids, True)
    if once:
        call(ids, True)
        print(json.dumps({"keys": 1 << log2_keys, "n": n, "segments": res["cnt"], "groups": res["ng"]}), flush=True)
        return
    for _ in range(2):
        call(None, False), call(None, True), call(ids, True), table.Insert(db, dr, flow_id=ids)
    sizing = median_ms(lambda: call(None, False), s, reps)
    records = median_ms(lambda: call(None, True), s, reps)
    grouped = median_ms(lambda: call(ids, True), s, reps)
    cnt, ng, un = res["cnt"], res["ng"], res["un"]
    insert = median_ms(lambda: table.Insert(db, dr, flow_id=ids), s, reps)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        h = ids.cpu().numpy().view(np.uint32)
        t1 = time.perf_counter()
        order = np.argsort(h, kind="stable")
        t2 = time.perf_counter()
        host.append((t2 - t0, t1 - t0, t2 - t1))
    host.sort()
    a, b = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"), torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b.copy_(a)
    d2d = median_ms(lambda: b.copy_(a), s, reps)
    passes = sort_passes(bound)
    mid = 8 * cnt + 2 * 8 * cnt            # histogram read; scatter read + write
    last = 8 * cnt + 8 * cnt + 2 * 32 * cnt + 4 * cnt  # histogram; pairs, records in and out, keys
    sort_ms = grouped[0] - records[0]      # sort passes + groups, by difference
    d2d_tbs = 2 * (1 << 30) / d2d[0] / 1e9
    print(json.dumps({
        "keys": 1 << log2_keys, "n": n, "segments": cnt, "groups": ng, "ungrouped": un, "id_bound": bound,
        "sort_passes": passes, "flows_in_table": st["flows"],
        "ms_sizing": sizing[0], "ms_records": records[0], "ms_grouped": grouped[0], "ms_grouped_min": grouped[1],
        "ms_sort_and_groups": round(sort_ms, 4), "ms_flow_insert": insert[0],
        "host_s_total": round(host[1][0], 4), "host_s_d2h": round(host[1][1], 4), "host_s_argsort": round(host[1][2], 4),
        "grouped_over_host": round(grouped[0] / 1e3 / host[1][0], 5),
        "bytes_mid_pass": mid, "bytes_last_pass": last, "bytes_sort": (passes - 1) * mid + last,
        "d2d_1gib_ms": d2d[0], "d2d_tbs_moved": round(d2d_tbs, 3),
        "sort_tbs_by_difference": round(((passes - 1) * mid + last) / sort_ms / 1e9, 3) if sort_ms > 0 else None,
        "order_checksum": int(order[:1024].sum())}), flush=True)


if __name__ == "__main__":
    n = 1 << (18 if "--small" in sys.argv else 24)
    batch = synth.make_tcp64(n)
    if "--once" in sys.argv:
        run(batch, int(sys.argv[sys.argv.index("--once") + 1]), once=True)
    else:
        for k in (10, 16, 20):
            run(batch, k)
