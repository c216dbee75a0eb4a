"""Time gpd_tcp_tracker_run (TCP connection tracking) beside the grouped
gpd_tcp_segments call on the same batch: the hand-off runs the same ordered compaction and the
same sort passes, and gathers 32-byte records where the tracker scans maps.

The batch is the size case of tests/test_tcptrack_gpu.py (tests/tcptrack_cases.py size_case):
n minimal Eth/IPv4/TCP frames resident in HBM, decoded and keyed once outside the timed span;
"uniform" is 2^16 small connections and one connection with a quarter of the packets, "one" is
every packet on one connection.  Medians (and minima) of HIP-event times around whole calls, 100
calls after 5 warm-up calls; every call synchronises its stream itself.  One JSON line per shape.

    python tools/tcptrack_time.py [--n N] [--handoff-only]

--handoff-only times gpd_tcp_segments alone: the form a tree without the tracker can run (put
that tree's package first on sys.path and import this file).
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

from gopacket_amd import layers as L  # noqa: E402
from gopacket_amd import parser as P, tcpassembly as T  # noqa: E402
from gopacket_amd.flows import NewFlowTable  # noqa: E402

WARM, REPS = 5, 100
SORT_SCAN_ROUND = 16384  # [digit][tile] counts the sort's scan takes between barriers (256 per tile)
SCAN_TILE, AGG_ROUND = 2048, 256  # gopacket_amd.tcptrack's, restated for a tree without it


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


def default_n():
    return max(SORT_SCAN_ROUND // 256 * T.SORT_TILE, AGG_ROUND * SCAN_TILE) + 1


def run(shape, n, handoff_only):
    from tcptrack_cases import size_case
    batch, _, _ = size_case(n, one=(shape == "one"))
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    table = NewFlowTable(p, 1 << 18)
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(n, 0)
    p.decode_device(db, dr)
    ids = table.Insert(db, dr)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    cap = table.Stats()["capacity"]
    segs = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    groups = torch.empty(n * 16, dtype=torch.uint8, device="cuda")

    def handoff():
        rc, cnt, ng, un = T._call(p, db, dr, ids, cap, segs, groups, n, s)
        assert rc == 0 and un == 0
        return cnt, ng
    for _ in range(WARM):
        cnt, ng = handoff()
    out = {"shape": shape, "n": n, "capacity": cap, "handoff_segments": cnt, "handoff_groups": ng}
    out["ms_tcp_segments_grouped"], out["ms_tcp_segments_grouped_min"] = median_ms(handoff, s, REPS)
    if not handoff_only:
        from gopacket_amd import tcptrack as M
        tr = M.NewConnTracker(p, table)

        def track():
            return tr.TrackBatch(db, dr, ids)
        for _ in range(WARM):
            r = track()
        out.update(tracked=r.tracked, accepted=r.accepted, connections=r.connections)
        out["ms_track_batch"], out["ms_track_batch_min"] = median_ms(track, s, REPS)
        out["ms_track_batch_with_conn_id"] = median_ms(lambda: tr.TrackBatch(db, dr, ids, want_conn_id=True), s, REPS)[0]
        out["track_over_handoff"] = round(out["ms_track_batch"] / out["ms_tcp_segments_grouped"], 3)
        out["ms_tcp_segments_grouped_again"] = median_ms(handoff, s, REPS)[0]  # (the spread of the yardstick)
        tr.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    n = int(sys.argv[sys.argv.index("--n") + 1]) if "--n" in sys.argv else default_n()
    for shape in ("uniform", "one"):
        run(shape, n, "--handoff-only" in sys.argv)
