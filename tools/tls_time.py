"""Time the TLS record decode over data resident in HBM, decoded once outside the
timed span.  Three shapes:

  appdata_1   2^22 Eth/IPv4/TCP frames to port 443, one application-data record each (four
              body lengths, versions from a hash of i): gpd_tls_decode
  mix_cont    2^22 frames: messages of 1 to 4 records (handshake, change cipher spec, application
              data, alert) and, one in four, a segment that continues a record begun in an earlier
              one (its first bytes are body bytes): gpd_tls_decode
  streams     2^16 streams of 16 KiB, twelve records each, back to back in one buffer:
              gpd_tls_decode_ranges

Modes:

  time  (default)  per shape, in one process, after 5 warm-up calls, the median and the minimum of
                   50 HIP-event times around the whole call on its stream (the sizing kernels, the
                   host synchronisation, the emit kernel) into arrays of exactly the needed
                   capacity; `ms_sizing_call` is the call with all capacities 0 (everything but the
                   emit kernel).  `host_16` is gpd_tls_decode_host over the same messages from 16
                   processes of the same box, each calling it message by message through ctypes
                   (buffers allocated once; `host_16_loop_overhead_s` is the same loops over empty
                   messages, what the calling loops themselves cost).  One JSON line per shape;
                   appdata_1 is also run at 2^20, the candidate count of tools/dns_time.py.
  split            the per-kernel split: per shape one child process (`run`) under
                   rocprofv3 --kernel-trace, the median time of every tls_* kernel from its trace.
  run --shape S    what `split` profiles: 3 warm-up and 10 timed calls of one shape.

    python tools/tls_time.py [time|split|run] [--log2n 22] [--shape S] [--out DIR]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import multiprocessing as mp
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import tls_cases as TC  # noqa: E402
from gopacket_amd.batch import PAD, PacketBatch  # noqa: E402

STREAM_BYTES = 16384


# ---------------------------------------------------------------- the shapes
def frame(m):
    return TC.eth(TC.ip4(TC.tcp(m), 6))


def appdata_frames():
    return [frame(TC.rec(TC.APP, bytes(range(k)))) for k in (32, 48, 57, 64)]


def mix_frames():
    body = lambda k: bytes((7 * i + 3) & 0xFF for i in range(k))
    return [frame(TC.rec(TC.APP, body(90))),
            frame(TC.rec(TC.HS, body(70), ver=0x0301) + TC.rec(TC.CCS, b"\x01", ver=0x0301)),
            frame(TC.rec(TC.HS, body(40)) + TC.rec(TC.CCS, b"\x01") + TC.rec(TC.HS, body(40))),
            frame(TC.rec(TC.APP, body(20)) + TC.rec(TC.APP, body(30)) + TC.rec(TC.APP, body(25)) + TC.rec(TC.ALERT, b"\x01\x00")),
            frame(b"\x00\x9a" + body(110)),                       # a continuation: body bytes first
            frame(TC.rec(TC.APP, body(60)) + TC.rec(TC.APP, body(300))[:40]),  # a record, and one begun
            frame(b"\x17" + body(100)),                           # a continuation that looks like a header
            frame(TC.rec(TC.APP, body(120)))]


def tiled(frames, kinds, n, slot):
    period = np.zeros((len(frames), slot), np.uint8)
    for k, f in enumerate(frames):
        assert len(f) <= slot
        period[k, :len(f)] = np.frombuffer(f, np.uint8)
    data = period[kinds]
    caplen = np.array([len(f) for f in frames], np.uint32)[kinds]
    return PacketBatch.from_arrays(np.concatenate([data.reshape(-1), np.zeros(PAD, np.uint8)]),
                                   np.arange(n, dtype=np.uint64) * slot, caplen, data_len=n * slot)


def stream_templates():
    """Four 16 KiB streams of twelve records: eleven of one length and one that ends the stream."""
    out = []
    for k, ln in enumerate((1400, 1350, 1290, 1200)):
        s = TC.rec(TC.APP, bytes(ln)) * 11
        s += TC.rec(TC.APP if k & 1 else TC.HS, bytes(STREAM_BYTES - len(s) - 5))
        assert len(s) == STREAM_BYTES
        out.append(s)
    return out


# ---------------------------------------------------------------- the host walker on 16 cores
def _host_worker(args):
    msgs, calls = args
    from gopacket_amd import tls as T
    lib = T.tls_lib()
    bufs = [np.frombuffer(m, np.uint8) for m in msgs]
    ptrs = [b.ctypes.data_as(C.c_void_p) if len(b) else None for b in bufs]
    lens = [len(m) for m in msgs]
    msg, recs = np.zeros(1, T.MSG_DTYPE), np.zeros(64, T.REC_DTYPE)
    pm, pr = msg.ctypes.data_as(C.c_void_p), recs.ctypes.data_as(C.c_void_p)
    cnt = T.GpdTlsCounts()
    fn, ref, k = lib.gpd_tls_decode_host, C.byref(cnt), len(msgs)
    t0 = time.perf_counter()
    for i in range(calls):
        j = i % k
        fn(ptrs[j], lens[j], 0, pm, pr, 64, ref)
    return time.perf_counter() - t0


def host_seconds(msgs, total, procs=16):
    """gpd_tls_decode_host `total` times over the distinct messages in turn, split over `procs`
    processes (spawned: none of them opens the GPU); the slowest worker's loop time."""
    with mp.get_context("spawn").Pool(procs) as pool:
        return max(pool.map(_host_worker, [(msgs, total // procs)] * procs))


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


def setup(shape, log2n):
    """(call(msgs, recs, caps) -> (rc, counts), n, first TLSResult, distinct host messages, bytes)."""
    import torch
    from gopacket_amd import layers as L, parser as P, tls as T
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    s = torch.cuda.current_stream()
    if shape == "streams":
        n = 1 << max(log2n - 6, 4)
        tm = stream_templates()
        tmpl = torch.from_numpy(np.frombuffer(b"".join(tm), np.uint8).copy()).to("cuda:0")
        buf = tmpl.repeat(n // len(tm))
        off = torch.arange(n, dtype=torch.int64, device="cuda:0") * STREAM_BYTES
        ln = torch.full((n,), STREAM_BYTES, dtype=torch.int32, device="cuda:0")
        rg = T.GpdTlsRanges(buf.data_ptr(), buf.numel(), off.data_ptr(), ln.data_ptr(), n)
        keep = (buf, off, ln, p)

        def call(msgs, recs, caps):
            out = T.GpdTlsOut(T._ptr(msgs), caps[0], T._ptr(recs), caps[1])
            cnt = T.GpdTlsCounts()
            rc = T.tls_lib().gpd_tls_decode_ranges(p.ctx().h, C.byref(rg), None, C.byref(out), C.byref(cnt),
                                                   C.c_void_p(s.cuda_stream))
            return rc, T._counts(cnt)
        first = T.DecodeTLSRanges(p, buf, off, ln)
        return call, n, first, tm, n * STREAM_BYTES, keep
    n = 1 << log2n
    if shape == "appdata_1":
        frames, slot = appdata_frames(), 128
        kinds = np.arange(n) % 4
    else:
        frames, slot = mix_frames(), 192
        kinds = (np.arange(n, dtype=np.uint64) * 2654435761 >> 7) % 8
    batch = tiled(frames, kinds.astype(np.int64), n, slot)
    if shape == "appdata_1":  # the record's version from a hash of i (bytes 55..56 of the frame)
        v = batch.data[:n * slot].reshape(n, slot)
        v[:, 56] = (np.arange(n, dtype=np.uint32) * 40503 >> 3) & 3
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(n, 0, records=True)
    p.decode_device(db, dr)
    torch.cuda.synchronize()
    b, r = db.c_batch(), dr.c_result()
    keep = (db, dr, p)

    def call(msgs, recs, caps):
        out = T.GpdTlsOut(T._ptr(msgs), caps[0], T._ptr(recs), caps[1])
        cnt = T.GpdTlsCounts()
        rc = T.tls_lib().gpd_tls_decode(p.ctx().h, C.byref(b), C.byref(r), None, C.byref(out), C.byref(cnt),
                                        C.c_void_p(s.cuda_stream))
        return rc, T._counts(cnt)
    first = T.DecodeTLS(p, db, dr)
    return call, n, first, [f[54:] for f in frames], int(batch.caplen.sum()), keep


def timed_calls(shape, log2n, reps, warm):
    import torch
    call, n, first, host_msgs, nbytes, keep = setup(shape, log2n)
    caps = (first.count, first.n_records)
    s = torch.cuda.current_stream()

    def full():
        rc, c = call(first.msgs, first.recs, caps)
        assert rc == 0 and c["msgs"] == caps[0], (rc, c)

    def sizing():
        rc, c = call(None, None, (0, 0))
        assert c["msgs"] == caps[0]
    for _ in range(warm):
        full(), sizing()
    return n, first, host_msgs, nbytes, median_ms(full, s, reps), median_ms(sizing, s, reps)


def mode_time(a):
    import torch
    shapes = [("appdata_1", a.log2n), ("mix_cont", a.log2n), ("streams", a.log2n)]
    if a.log2n != 20:
        shapes.insert(1, ("appdata_1", 20))
    if a.shape:
        shapes = [(a.shape, a.log2n)]
    for shape, log2n in shapes:
        n, first, host_msgs, nbytes, full, size = timed_calls(shape, log2n, 50, 5)
        verdicts = np.bincount(first.to_host()[0]["verdict"], minlength=8)[:8].tolist()
        torch.cuda.synchronize()
        host = host_seconds(host_msgs, first.count)
        empty = host_seconds([b""], first.count)
        print(json.dumps({
            "shape": shape, "n": n, "messages": first.count, "records": first.n_records, "deferred": first.deferred,
            "verdicts_0_to_7": verdicts, "input_bytes": nbytes,
            "ms_call": full[0], "ms_call_min": full[1], "ms_sizing_call": size[0],
            "messages_per_s": round(first.count / full[0] * 1e3), "records_per_s": round(first.n_records / full[0] * 1e3),
            "input_GB_per_s": round(nbytes / full[0] / 1e6, 1),
            "host_16_s": round(host, 4), "host_16_loop_overhead_s": round(empty, 4),
            "host_16_messages_per_s": round(first.count / host), "call_over_host_16": round(full[0] / 1e3 / host, 5)}),
            flush=True)


def mode_run(a):
    n, first, _, _, full, size = timed_calls(a.shape, a.log2n, 10, 3)
    print(json.dumps({"shape": a.shape, "n": n, "messages": first.count, "ms_call": full[0], "ms_sizing_call": size[0]}))


def mode_split(a):
    for shape in ([a.shape] if a.shape else ["appdata_1", "mix_cont", "streams"]):
        out = os.path.join(os.path.abspath(a.out), shape)
        os.makedirs(out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "run", "--shape", shape, "--log2n", str(a.log2n)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.exit("rocprofv3 failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        kern = {}
        for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    low = {k.lower(): v for k, v in row.items()}
                    m = re.search(r"tls_[a-z0-9]+_kernel", low.get("kernel_name", low.get("name", "")))
                    if m:
                        kern.setdefault(m.group(0), []).append(int(low["end_timestamp"]) - int(low["start_timestamp"]))
        # a full call runs every kernel, a sizing call all but the emit kernel: the median of each
        us = {k: round(float(np.median(v)) / 1e3, 1) for k, v in sorted(kern.items())}
        print(json.dumps({"mode": "split", "shape": shape, "child": r.stdout.strip().splitlines()[-1:],
                          "kernel_us_median": us, "launches": {k: len(v) for k, v in sorted(kern.items())},
                          "kernels_us_sum": round(sum(us.values()), 1)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="time", choices=("time", "split", "run"))
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--shape", choices=("appdata_1", "mix_cont", "streams"))
    ap.add_argument("--out", default="tls_split_out")
    ap.add_argument("--timeout", type=int, default=400)
    a = ap.parse_args()
    if a.mode == "run" and not a.shape:
        ap.error("run needs --shape")
    {"time": mode_time, "split": mode_split, "run": mode_run}[a.mode](a)
