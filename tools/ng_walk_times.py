#!/usr/bin/env python3
"""Timings of the pcapng device walk (gpd_decode_pcapng, gpd_ngwalk.hip) on the GPU; each mode
prints one JSON line.

  rate   [--blocks N] [--reps R]   PCIe-inclusive: capture bytes per second of gpd_decode_pcapng
                                   over N 64-byte frames in enhanced packet blocks (96-byte
                                   stride) from a registered buffer, and gpd_decode_pcap over the
                                   same frames as pcap records (80-byte stride) in the same
                                   process — the yardstick
  chunks [--blocks N] [--out DIR] [--parse-only]
                                   per 64 MiB chunk: ng_walk, ng_stitch, ng_fill kernel times and
                                   the chunk's H2D copy time, from one rocprofv3 run
                                   (--kernel-trace --memory-copy-trace --stats) of the `run` mode
                                   started as a child process
  run    [--blocks N]              what `chunks` profiles: one warm-up and two timed decodes

A host clock around calls that end synchronised times `rate`; kernel and copy times come from
the profiler's trace, in a run of its own.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser_():
    from gopacket_amd import layers as L
    from gopacket_amd import parser as P
    return P.NewDecodingLayerParser(L.LayerTypeEthernet, P.Ethernet(), P.Dot1Q(), P.IPv4(), P.IPv6(),
                                    P.IPv6ExtensionSkipper(), P.TCP(), P.UDP(), P.VXLAN(), P.Payload(),
                                    P.Fragment())


def frames64(n):
    """n x 64 bytes of config-2 frames (64-B Ethernet/IPv4/UDP), generated in slices."""
    from gopacket_amd import synth
    out = np.empty((n, 64), np.uint8)
    step = 1 << 20
    for lo in range(0, n, step):
        b = synth.make_udp64(min(step, n - lo), seed=0x5EED0002 + lo)
        assert (b.caplen == 64).all()
        idx = b.offset.astype(np.int64)[:, None] + np.arange(64)[None, :]
        out[lo:lo + b.n] = b.data[idx]
    return out


def capture_ng(fr):
    """Section header, one Ethernet interface, then frame i as a little-endian enhanced packet
    block {6, 96, 0, ts_high, ts_low = i, 64, 64, bytes, 96}."""
    from gopacket_amd import pcapng
    from gopacket_amd.batch import PAD
    n = fr.shape[0]
    pre = pcapng.section_block() + pcapng.interface_block(1, 0)
    cap = np.zeros(len(pre) + 96 * n + PAD, np.uint8)
    cap[:len(pre)] = np.frombuffer(pre, np.uint8)
    body = cap[len(pre):len(pre) + 96 * n].reshape(n, 96)
    hdr = np.zeros((n, 7), np.uint32)
    hdr[:, 0], hdr[:, 1], hdr[:, 5], hdr[:, 6] = 6, 96, 64, 64
    hdr[:, 4] = np.arange(n, dtype=np.uint64).astype(np.uint32)
    body[:, :28] = hdr.view(np.uint8).reshape(n, 28)
    body[:, 28:92] = fr
    body[:, 92:96] = np.frombuffer(np.uint32(96).tobytes(), np.uint8)
    return cap


def capture_pcap(fr):
    import struct
    from gopacket_amd import pcap
    from gopacket_amd.batch import PAD
    n = fr.shape[0]
    cap = np.zeros(24 + 80 * n + PAD, np.uint8)
    cap[:24] = np.frombuffer(struct.pack("<IHHiIII", pcap.MAGIC_MICRO, 2, 4, 0, 0, 262144, 1), np.uint8)
    body = cap[24:24 + 80 * n].reshape(n, 80)
    hdr = np.zeros((n, 4), np.uint32)
    idx = np.arange(n, dtype=np.uint64)
    hdr[:, 0], hdr[:, 1], hdr[:, 2], hdr[:, 3] = idx // 1000000, idx % 1000000, 64, 64
    body[:, :16] = hdr.view(np.uint8).reshape(n, 16)
    body[:, 16:] = fr
    return cap


def result(n):
    from gopacket_amd.results import BatchResult
    return BatchResult(np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64),
                       np.zeros(n, np.uint64), np.zeros(n, np.uint32), None, np.zeros(n, np.uint32), None)


def register(p, arrays):
    from gopacket_amd._lib import check, lib
    for a in arrays:
        check(lib.gpd_host_register(p.ctx().h, a.ctypes.data, a.nbytes), "gpd_host_register")


def decode_ng(p, cap, res, n):
    from gopacket_amd import pcapng
    from gopacket_amd.batch import PAD
    rd = pcapng.NgReader(cap)
    t0 = time.perf_counter()
    _, k, stop, err = p.DecodePcapNg(rd, max_n=n + 1, out=res)
    dt = time.perf_counter() - t0
    assert (k, stop, err) == (n, pcapng.STOP_EOF, None), (k, stop, err)
    return dt, cap.shape[0] - PAD, pcapng.last_walk_counts()


def decode_pcap(p, cap, res, n):
    from gopacket_amd.batch import PAD
    t0 = time.perf_counter()
    _, k, err = p.DecodePcap(cap, max_n=n + 1, out=res)
    dt = time.perf_counter() - t0
    assert (k, err) == (n, None), (k, err)
    return dt, cap.shape[0] - PAD


def mode_rate(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.blocks
    fr = frames64(n)
    ng, pc = capture_ng(fr), capture_pcap(fr)
    del fr
    p = parser_()
    res = result(n + 1)
    register(p, [ng, pc, res.status, res.layers, res.net_hash, res.tp_hash, res.csum, res.hdr_off])
    t_ng, t_pc, counts = [], [], None
    ref = None
    for rep in range(a.reps + 1):  # the first pass of each warms up; then alternating
        dt, nbytes_pc = decode_pcap(p, pc, res, n)
        if ref is None:
            ref = [x[:n].copy() for x in (res.status, res.layers, res.net_hash, res.tp_hash, res.csum, res.hdr_off)]
        if rep:
            t_pc.append(dt)
        dt, nbytes_ng, counts = decode_ng(p, ng, res, n)
        if rep:
            t_ng.append(dt)
        else:  # the same frames: the same results
            for x, y in zip(ref, (res.status, res.layers, res.net_hash, res.tp_hash, res.csum, res.hdr_off)):
                assert np.array_equal(x, y[:n])
    med = lambda v: float(np.median(v))
    print(json.dumps({
        "mode": "rate", "blocks": n, "reps": a.reps,
        "pcapng": {"bytes": nbytes_ng, "ms": [round(t * 1e3, 2) for t in t_ng],
                   "GBps": round(nbytes_ng / med(t_ng) / 1e9, 2), "Mpps": round(n / med(t_ng) / 1e6, 1),
                   "walk_counts": counts},
        "pcap": {"bytes": nbytes_pc, "ms": [round(t * 1e3, 2) for t in t_pc],
                 "GBps": round(nbytes_pc / med(t_pc) / 1e9, 2), "Mpps": round(n / med(t_pc) / 1e6, 1)},
        "pcapng_over_pcap_bytes_per_s": round((nbytes_ng / med(t_ng)) / (nbytes_pc / med(t_pc)), 3)}))


def mode_run(a):
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.blocks
    ng = capture_ng(frames64(n))
    p = parser_()
    res = result(n + 1)
    register(p, [ng, res.status, res.layers, res.net_hash, res.tp_hash, res.csum, res.hdr_off])
    for _ in range(3):
        dt, nbytes, counts = decode_ng(p, ng, res, n)
    print(json.dumps({"mode": "run", "blocks": n, "bytes": nbytes, "last_ms": round(dt * 1e3, 2),
                      "walk_counts": counts}))


def mode_chunks(a):
    out = os.path.abspath(a.out)
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "run", "--blocks", str(a.blocks)]
    child = []
    if not a.parse_only:  # (--parse-only: read the traces an earlier run left in --out)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.exit("rocprofv3 failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        child = r.stdout.strip().splitlines()[-1:]

    def rows(pattern):
        for f in glob.glob(os.path.join(out, "**", pattern), recursive=True):
            with open(f, newline="") as fh:
                yield from csv.DictReader(fh)

    def col(row, *names):
        low = {k.lower(): v for k, v in row.items()}
        for nme in names:
            if nme in low:
                return low[nme]
        raise KeyError(names)

    kern = {}
    for row in rows("*kernel_trace.csv"):
        name = col(row, "kernel_name", "name")
        for k in ("ng_walk", "ng_stitch", "ng_fill"):
            if k in name:
                kern.setdefault(k, []).append(int(col(row, "end_timestamp")) - int(col(row, "start_timestamp")))
    h2d = []
    for row in rows("*memory_copy_trace.csv"):
        if "HOST_TO_DEVICE" in col(row, "direction", "kind", "name").upper():
            h2d.append(int(col(row, "end_timestamp")) - int(col(row, "start_timestamp")))
    # the chunks' copies: those of the longest class (control-block copies are microseconds); a
    # copy's time varies with what else the link carries, so the fastest one is the bound to beat
    full = [t for t in h2d if t >= 0.4 * max(h2d)] if h2d else []
    us = lambda v: round(float(np.median(v)) / 1e3, 1) if v else None
    walk = {k: us(v) for k, v in kern.items()}
    total = sum(x for x in walk.values() if x)
    print(json.dumps({"mode": "chunks", "blocks": a.blocks, "child": child,
                      "us_per_64MiB_chunk": walk, "launches": {k: len(v) for k, v in kern.items()},
                      "walk_stitch_fill_us": round(total, 1), "h2d_us_median": us(full),
                      "h2d_us_min": round(min(full) / 1e3, 1) if full else None, "h2d_copies": len(full),
                      "hidden_behind_copy": bool(full) and total < min(full) / 1e3}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "chunks", "run"))
    ap.add_argument("--blocks", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="ng_chunks_out")
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--parse-only", action="store_true")
    a = ap.parse_args()
    {"rate": mode_rate, "chunks": mode_chunks, "run": mode_run}[a.mode](a)
