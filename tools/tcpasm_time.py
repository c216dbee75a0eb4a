"""Time gpd_tcp_assembler_run (the stateful TCP assembler) on the workload of
tools/tcpstream_time.py: 2^24 x 64-B Eth/IPv4/TCP frames with 10 payload bytes resident in HBM,
2^10 / 2^16 / 2^20 connection keys, every key one in-order stream behind a SYN.  Medians of 10
HIP-event times around whole calls after warm-up, and a device-to-device copy of 1 GiB timed in
the same process.

  (a) no carry   the whole batch in one run, nothing displaced: gpd_tcp_assembler_run (object
                 reset before every call, outside the timed span) beside gpd_tcp_assemble on the
                 same hand-off; the ratio.  The new entry point does strictly more: timestamps,
                 the item selection, a carry pass that finds nothing.
  (b) carry      the batch cut in two halves of packets; 1 % of the first half's segments (taken
                 from the last 2 % of its packets, never a SYN) are displaced to the front of the
                 second half.  Run 1 buffers what follows the gaps; stats() between the runs; run
                 2 (timed; reset + run 1 before every repetition, untimed) fills them.  Reported:
                 run 2's time, the carry-gather bytes (pages read from the old store or the batch
                 and written to the new store, twice their bytes, plus 16-byte pieces) and rate.

One JSON line per key count and part.  For an A/B of the walk's in-order run build a second tree
with tools/ab_flags_build.sh . DIR "-DGPD_TAM_NO_CHAIN" and run DIR/tools/tcpasm_time.py (not
measured yet).

    python tools/tcpasm_time.py [--small] [--keys LOG2 ...] [--part a|b]   (--small: 2^18 packets)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import layers as L, synth  # noqa: E402
from gopacket_amd import parser as P, tcpasm as M, tcpassembly as T, tcpstream as S  # noqa: E402
from gopacket_amd.batch import PacketBatch  # noqa: E402
from gopacket_amd.flows import NewFlowTable  # noqa: E402
from tcpstream_time import median_ms, with_streams  # noqa: E402


def d2d_tbs(s, reps):
    a, b = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"), torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b.copy_(a)
    ms = median_ms(lambda: b.copy_(a), s, reps)[0]
    return ms, 2 * (1 << 30) / ms / 1e9


class Handoff:
    """A batch on the device, decoded, keyed by `table` and handed over."""

    def __init__(self, p, table, batch):
        self.n = batch.n
        self.db = P.DeviceBatch(batch, 0)
        dr = P.DeviceResult(self.n, 0, records=True)
        p.decode_device(self.db, dr)
        ids = table.Insert(self.db, dr)
        torch.cuda.synchronize()
        self.segs = torch.empty(self.n * 32, dtype=torch.uint8, device="cuda")
        self.groups = torch.empty(self.n * 16, dtype=torch.uint8, device="cuda")
        rc, self.cnt, self.ng, self.un = T._call(p, self.db, dr, ids, table.Stats()["capacity"], self.segs, self.groups,
                                                 self.n, torch.cuda.current_stream())
        assert rc == 0 and self.un == 0, (rc, self.un)


class Buffers:
    def __init__(self, out):
        self.nr, self.ns, self.nb = out[0], out[1], out[2]
        self.recs = torch.empty(max(self.nr, 1) * 32, dtype=torch.uint8, device="cuda")
        self.seen = torch.empty(max(self.nr, 1), dtype=torch.int64, device="cuda")
        self.streams = torch.empty(max(self.ns, 1) * 48, dtype=torch.uint8, device="cuda")
        self.byts = torch.empty(max(self.nb, 16), dtype=torch.uint8, device="cuda")


def asm_run(asm, h, ts, buf=None, flush=(0, False, False)):
    if buf is None:
        rc, out = asm.run_raw(h.db, h.segs, h.cnt, h.groups, h.ng, ts, 0, flush, None, 0, None, None, 0, None, 0)
    else:
        rc, out = asm.run_raw(h.db, h.segs, h.cnt, h.groups, h.ng, ts, 0, flush, buf.recs, buf.nr, buf.seen, buf.streams,
                              buf.ns, buf.byts, buf.nb)
    assert rc == 0, rc
    return out


def timed(fn, before, s, reps):
    """median_ms of fn with `before` run (and synchronised) outside the timed span."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        before()
        torch.cuda.synchronize()
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return round(ms[len(ms) // 2], 4), round(ms[0], 4)


def part_a(batch, log2_keys, reps):
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    table = NewFlowTable(p, 2 << log2_keys)
    h = Handoff(p, table, batch)
    s = torch.cuda.current_stream()
    ts = torch.arange(h.n, dtype=torch.int64, device="cuda")
    # the existing entry point, whole (records, streams, bytes), no state
    rc, o = S._call(p, h.db, h.segs, h.cnt, h.groups, h.ng, None, 0, 0, False, None, 0, None, None, 0, s)
    assert rc == 0
    old = Buffers(o)

    def assemble():
        rc, o2 = S._call(p, h.db, h.segs, h.cnt, h.groups, h.ng, None, 0, 0, False, old.recs, old.nr, old.streams,
                         old.byts, old.nb, s)
        assert rc == 0 and o2 == o
    asm = M.NewAssembler(p, table)
    out = asm_run(asm, h, ts)
    buf = Buffers(out)
    for _ in range(2):
        assemble()
        asm.reset()
        asm_run(asm, h, ts, buf)
    ms_old = median_ms(assemble, s, reps)
    ms_size = timed(lambda: asm_run(asm, h, ts), asm.reset, s, reps)
    ms_new = timed(lambda: asm_run(asm, h, ts, buf), asm.reset, s, reps)
    d2d_ms, d2d = d2d_tbs(s, reps)
    print(json.dumps({"part": "a", "keys": 1 << log2_keys, "n": h.n, "segments": h.cnt, "groups": h.ng,
                      "records": out[0], "streams": out[1], "stream_bytes": out[2], "calls": out[3],
                      "connections_after": out[4], "pages_after": out[5], "old_records": o[0], "old_bytes": o[2],
                      "ms_tcp_assemble_whole": ms_old[0], "ms_assembler_sizing": ms_size[0],
                      "ms_assembler_run": ms_new[0], "ms_assembler_run_min": ms_new[1],
                      "run_over_assemble": round(ms_new[0] / ms_old[0], 3), "d2d_1gib_ms": d2d_ms,
                      "d2d_tbs_moved": round(d2d, 3)}), flush=True)
    asm.close()


def part_b(batch, log2_keys, reps):
    n = batch.n
    rows = batch.data[:n * 64].reshape(n, 64)
    half = n // 2
    rng = np.random.default_rng(0x5EED0061)
    tail = np.arange(half - half // 50, half)                      # the last 2 % of the first half
    tail = tail[rows[tail, 47] & 0x02 == 0]                        # never a SYN
    moved = np.sort(rng.choice(tail, min(half // 100, len(tail)), replace=False))
    keep = np.ones(half, bool)
    keep[moved] = False
    first = np.ascontiguousarray(rows[:half][keep])
    second = np.ascontiguousarray(np.concatenate([rows[moved], rows[half:]]))

    def as_batch(a):
        m = a.shape[0]
        return PacketBatch.from_arrays(a.reshape(-1), np.arange(m, dtype=np.uint32) * 64, np.full(m, 64, np.uint32),
                                       data_len=m * 64)
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    table = NewFlowTable(p, 2 << log2_keys)
    h1, h2 = Handoff(p, table, as_batch(first)), Handoff(p, table, as_batch(second))
    s = torch.cuda.current_stream()
    ts1 = torch.arange(h1.n, dtype=torch.int64, device="cuda")
    ts2 = torch.arange(h2.n, dtype=torch.int64, device="cuda") + h1.n
    asm = M.NewAssembler(p, table)
    out1 = asm_run(asm, h1, ts1)
    b1 = Buffers(out1)
    asm_run(asm, h1, ts1, b1)
    between = asm.stats()
    out2 = asm_run(asm, h2, ts2)
    b2 = Buffers(out2)

    def prepare():
        asm.reset()
        asm_run(asm, h1, ts1, b1)
    for _ in range(2):
        prepare()
        asm_run(asm, h2, ts2, b2)
    after = asm.stats()
    ms1 = timed(lambda: asm_run(asm, h1, ts1, b1), asm.reset, s, reps)
    ms2 = timed(lambda: asm_run(asm, h2, ts2, b2), prepare, s, reps)
    d2d_ms, d2d = d2d_tbs(s, reps)
    print(json.dumps({"part": "b", "keys": 1 << log2_keys, "n": n, "displaced": int(len(moved)),
                      "run1_segments": h1.cnt, "run2_segments": h2.cnt, "run1_out": list(out1), "run2_out": list(out2),
                      "stats_between": between, "stats_after": after, "ms_run1": ms1[0], "ms_run2": ms2[0],
                      "ms_run2_min": ms2[1],
                      "carry_gather_bytes_run1": 2 * between["page_bytes"] + 16 * between["pages"],
                      "carry_gather_bytes_run2": 2 * after["page_bytes"] + 16 * after["pages"],
                      "carried_records_run2_bytes_from_store": between["page_bytes"] - after["page_bytes"],
                      "d2d_1gib_ms": d2d_ms, "d2d_tbs_moved": round(d2d, 3)}), flush=True)
    asm.close()


if __name__ == "__main__":
    n = 1 << (18 if "--small" in sys.argv else 24)
    keys = (10, 16, 20)
    if "--keys" in sys.argv:
        keys = [int(v) for v in sys.argv[sys.argv.index("--keys") + 1:] if v.isdigit()]
    parts = sys.argv[sys.argv.index("--part") + 1] if "--part" in sys.argv else "ab"
    base = synth.make_tcp64(n)
    for k in keys:
        batch = with_streams(base, k)
        if "a" in parts:
            part_a(batch, k, 10)
        if "b" in parts:
            part_b(batch, k, 10)
