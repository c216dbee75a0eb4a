"""Time gpd_bpf_filter on an HBM-resident batch: 2^24 x 64-B UDP frames (config 2's
batch) and 2^22 IMIX frames, for four programs: `ret #1` (the launch and store floor), the
13-instruction `ip and tcp and port 80` (which UDP frames leave at its fourth instruction), the
same for UDP (which they run to the end), and a 13-instruction variant of that which keeps the
protocol byte in M.  HIP events on the call's stream, the median of 20 calls after warm-up, keep and ret
both written.  Beside each, in the same process on the same batch: gpd_decode in the record
form, and the read-only streaming probe (libgpd_probe.so) over the bytes the filter touches —
per 64-packet tile, 8 B of descriptors per packet plus the 64-B sectors that hold bytes 12..37
of each packet (counted from the batch's offsets).  One JSON line each.

    python tools/bpf_time.py [--small]      (--small: 2^18 / 2^16 packets, a quick check)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import bpf as B, layers as L, synth  # noqa: E402
from gopacket_amd import parser as P  # noqa: E402

PORT80 = [(0x28, 0, 0, 12), (0x15, 0, 10, 0x800), (0x30, 0, 0, 23), (0x15, 0, 8, 6), (0x28, 0, 0, 20),
          (0x45, 6, 0, 0x1fff), (0xb1, 0, 0, 14), (0x48, 0, 0, 14), (0x15, 2, 0, 80), (0x48, 0, 0, 16),
          (0x15, 0, 1, 80), (0x06, 0, 0, 262144), (0x06, 0, 0, 0)]
# the same decision for UDP, with the protocol byte parked in M[1] and compared from there
PORT80_M = [(0x28, 0, 0, 12), (0x15, 0, 10, 0x800), (0x30, 0, 0, 23), (0x02, 0, 0, 1), (0x28, 0, 0, 20),
            (0x45, 6, 0, 0x1fff), (0xb1, 0, 0, 14), (0x60, 0, 0, 1), (0x15, 0, 3, 17), (0x48, 0, 0, 16),
            (0x15, 0, 1, 80), (0x06, 0, 0, 262144), (0x06, 0, 0, 0)]
# `udp and port 80` in the same 13 instructions: on UDP frames every lane runs to the port compares
UDP80 = [q if i != 3 else (0x15, 0, 8, 17) for i, q in enumerate(PORT80)]
PROGRAMS = [("ret #1", [(0x06, 0, 0, 1)], 0), ("ip and tcp and port 80", PORT80, 26),
            ("ip and udp and port 80", UDP80, 26), ("udp dst port 80, protocol via M", PORT80_M, 26)]


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
    return ms[len(ms) // 2], ms[0]


def probe_ms(ntiles, per_tile):
    """The read-only streaming probe's mean launch time for ntiles tiles of per_tile bytes."""
    path = os.path.join(ROOT, "gopacket_amd", "libgpd_probe.so")
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    lib.gpd_probe_stream2.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_int,
                                      C.POINTER(C.c_float)]
    ms = C.c_float()
    rc = lib.gpd_probe_stream2(0, ntiles, per_tile, 20, 150.0, 2, C.byref(ms))
    return float(ms.value) if rc == 0 else None


def run(name, batch, reps=20):
    n = batch.n
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    db = P.DeviceBatch(batch, 0)
    s = torch.cuda.current_stream()
    dr = P.DeviceResult(n, 0, hdr_off=False, records=True)
    for _ in range(3):
        p.decode_device(db, dr)
    decode, _ = median_ms(lambda: p.decode_device(db, dr), s, reps)
    del dr
    # 64-B sectors holding bytes [12, 38) of each packet that has them
    off, cap = batch.offset.astype(np.int64), batch.caplen.astype(np.int64)
    has = cap >= 38
    sectors = int((((off + 37) // 64 - (off + 12) // 64 + 1) * has).sum())
    ntiles = (n + 63) // 64
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    ret = torch.empty(n, dtype=torch.int32, device="cuda")
    lib, b = B.bpf_lib(), db.c_batch()
    for pname, prog, touched in PROGRAMS:
        f = B.NewBPFInstructionFilter(prog, p)

        def call():
            rc = lib.gpd_bpf_filter(f.h, C.byref(b), None, C.c_void_p(keep.data_ptr()), C.c_void_p(ret.data_ptr()),
                                    C.c_void_p(s.cuda_stream))
            assert rc == 0, lib.gpd_last_error_string()
        for _ in range(3):
            call()
        ms, ms_min = median_ms(call, s, reps)
        matched = int(keep.sum())
        rd = 8 * n + (64 * sectors if touched else 0)
        wr = 5 * n
        pm = probe_ms(ntiles, max(16, (rd + ntiles - 1) // ntiles))
        tbs = lambda byts, t: round(byts / t / 1e9, 3) if t and t > 0 else None
        print(json.dumps({
            "workload": name, "program": pname, "insns": len(prog), "n": n, "matched": matched,
            "ms_filter": round(ms, 4), "ms_filter_min": round(ms_min, 4), "gpps": round(n / ms / 1e6, 2),
            "read_bytes_model": rd, "write_bytes": wr, "tbs_model": tbs(rd + wr, ms),
            "ms_decode_records": round(decode, 4), "filter_over_decode": round(ms / decode, 3),
            "ms_probe_read_only": round(pm, 4) if pm else None, "probe_tbs": tbs(rd, pm),
            "filter_over_probe": round(ms / pm, 2) if pm else None}), flush=True)


if __name__ == "__main__":
    small = "--small" in sys.argv
    run("udp64 2^%d" % (18 if small else 24), synth.make_udp64(1 << (18 if small else 24)))
    run("imix 2^%d" % (16 if small else 22), synth.make_imix(1 << (16 if small else 22)))
