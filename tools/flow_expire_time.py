"""Time flow expiry (gpd_flow_expire) and what tombstones cost an insert.

A table of 2^20 records at half load: 2^19 minimal Eth/IPv4/TCP frames of distinct keys
(tests/tcptrack_cases.py frames), resident in HBM, decoded once outside the timed spans.

  expire   the table is reset and filled (packet i is sequence number i), then Expire(cutoff) with
           cutoff at 10 %, 50 % and 100 % of the packets is timed: mark, compaction, removal, sweep
           and the stream synchronisation of the call, ids for the whole capacity allocated outside.
  insert   the even keys' packets are inserted again (every packet finds its flow): into the table
           as filled, and after half of the odd keys' records were removed; the tombstones the
           sweep left (runs that end at a record) are counted by Load and reported.  The first runs
           the kernels of a table without removals, the second the tombstone-aware ones.

Medians (and minima) of HIP-event times, REPS timed calls after WARM warm-up calls.  One JSON line.

    python tools/flow_expire_time.py [--log2 K]     (K: log2 of the capacity, default 20)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "gopacket_amd" not in sys.modules:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import flowexpire as FE  # noqa: E402
from gopacket_amd import layers as L  # noqa: E402
from gopacket_amd import parser as P  # noqa: E402
from gopacket_amd.flows import NewFlowTable  # noqa: E402

WARM, REPS = 3, 15


def timed(fn, s, prepare=None):
    """(median, minimum) ms of fn() over REPS calls after WARM; prepare() runs untimed before each."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for k in range(WARM + REPS):
        if prepare:
            prepare()
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        if k >= WARM:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return round(ms[len(ms) // 2], 4), round(ms[0], 4)


def device_batch(p, j):
    from tcptrack_cases import ACK, frames
    j = np.asarray(j, np.uint32)
    b = frames(0x0A000000 + j, np.full(len(j), 0xC0A80001, np.uint32), 1024 + j % 60000, np.full(len(j), 80),
               np.full(len(j), ACK))
    db, dr = P.DeviceBatch(b, 0), P.DeviceResult(b.n, 0)
    p.decode_device(db, dr)
    return db, dr


def main(log2):
    cap, n = 1 << log2, 1 << (log2 - 1)
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    table = NewFlowTable(p, cap)
    s = torch.cuda.current_stream()
    db, dr = device_batch(p, np.arange(n))
    fid = torch.empty(n, dtype=torch.int32, device="cuda")
    ids = torch.empty(cap, dtype=torch.int32, device="cuda")
    out = {"capacity": cap, "records": n, "warm": WARM, "reps": REPS}

    def fill():
        table.Reset()
        table.Insert(db, dr, fid, 0)

    out["ms_fill"] = timed(fill, s)
    for pct in (10, 50, 100):
        cutoff = n * pct // 100
        count = [0]

        def expire():
            rc, count[0] = FE.expire_raw(table, cutoff, None, 0, ids, cap)
            assert rc == 0
        out[f"ms_expire_{pct}pct"] = timed(expire, s, prepare=fill)
        assert count[0] == cutoff
        out[f"load_after_expire_{pct}pct"] = FE.Load(table)
    pairs = [0]

    def expire_pairs():
        rc, pairs[0] = FE.expire_raw(table, n // 2, None, FE.EXPIRE_PAIRS, ids, cap)
        assert rc == 0
    out["ms_expire_50pct_pairs"] = timed(expire_pairs, s, prepare=fill)
    assert pairs[0] == n // 2  # (no key's reverse is in the table: every pair is complete)

    # the insert of existing flows, without and with tombstones
    even = np.arange(0, n, 2)
    eb, er = device_batch(p, even)
    efid = torch.empty(len(even), dtype=torch.int32, device="cuda")
    fill()
    first = table.Insert(eb, er, efid, n).clone()
    base = [2 * n]

    def again():
        table.Insert(eb, er, efid, base[0])
        base[0] += len(even)
    out["load_no_tombstones"] = FE.Load(table)
    out["ms_insert_existing_no_tombstones"] = timed(again, s)
    odd_ids = table.Insert(*device_batch(p, np.arange(1, n, 2)), None, base[0])
    base[0] += n // 2
    FE.Remove(table, odd_ids[::2].contiguous())
    out["load_half_of_the_others_removed"] = FE.Load(table)
    out["ms_insert_existing_with_tombstones"] = timed(again, s)
    assert torch.equal(efid, first) and table.Stats()["flows"] == n - n // 4
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[sys.argv.index("--log2") + 1]) if "--log2" in sys.argv else 20)
