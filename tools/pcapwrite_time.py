"""Time gpd_pcap_write on an HBM-resident batch: 2^24 x 64-B UDP frames and 2^22
IMIX frames, each with every packet kept, a random 1/8 mask and a one-flow mask (the packets
whose FastHash pair equals packet 0's).  HIP events on the call's stream after warm-up: the whole
call, and the sizing call (the scan alone) whose time is taken off for the copy.  Beside each, a
device-to-device hipMemcpyAsync of as many bytes as the stream has, in the same process.  The
algorithmic bytes are reads of 21 B of descriptors per packet (offset, caplen, ts, length, keep)
plus the kept packets' bytes, and writes of 16 B + caplen per kept packet.  One JSON line each.

    python tools/pcapwrite_time.py [--small]      (--small: 2^18 / 2^16 packets, a quick check)
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import layers as L, synth  # noqa: E402
from gopacket_amd import parser as P, pcapwrite as PW  # noqa: E402


def hip_runtime():
    """The HIP runtime this process already runs on (the one torch loaded), by its mapped path."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime mapped")


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


def run(name, batch, reps=20):
    n = batch.n
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = 0xFFF
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(n, 0, hdr_off=False)
    p.decode_device(db, dr)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    ts = torch.from_numpy((np.arange(n, dtype=np.int64) * 1000)).cuda()
    length = db.caplen.clone()
    one_flow = ((dr.net_hash == dr.net_hash[0]) & (dr.tp_hash == dr.tp_hash[0])).to(torch.uint8)
    masks = {"all": torch.ones(n, dtype=torch.uint8, device="cuda"),
             "random 1/8": torch.from_numpy((rng.integers(0, 8, n) == 0).astype(np.uint8)).cuda(),
             "one flow": one_flow}
    del dr
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    s = torch.cuda.current_stream()
    lib, h, b = PW.pw_lib(), p.ctx().h, db.c_batch()
    caplen_sum = int(db.caplen.to(torch.int64).sum())
    out = torch.empty(24 + 16 * n + caplen_sum + 16, dtype=torch.uint8, device="cuda")
    src = torch.empty_like(out)
    nw, nb, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for mname, keep in masks.items():
        def call(dst, cap):
            rc = lib.gpd_pcap_write(h, C.byref(b), ptr(ts), ptr(length), ptr(keep), PW.GPD_PCAPW_FILE_HEADER,
                                    262144, 1, dst, cap, C.byref(nw), C.byref(nb), C.byref(bad),
                                    C.c_void_p(s.cuda_stream))
            assert rc == 0, lib.gpd_last_error_string()
        for _ in range(3):
            call(ptr(out), out.numel())
        total, total_min = median_ms(lambda: call(ptr(out), out.numel()), s, reps)
        scan, _ = median_ms(lambda: call(None, 0), s, reps)
        nbytes, kept = nb.value, nw.value
        copy_fn = lambda: hip.hipMemcpyAsync(ptr(out), ptr(src), nbytes, 3, C.c_void_p(s.cuda_stream))
        for _ in range(3):
            copy_fn()
        d2d, _ = median_ms(copy_fn, s, reps)
        kept_bytes = nbytes - 24 - 16 * kept
        rd, wr = 21 * n + kept_bytes, 16 * kept + kept_bytes
        tbs = lambda byts, ms: round(byts / ms / 1e9, 3) if ms > 0 else None
        print(json.dumps({
            "workload": name, "mask": mname, "n": n, "kept": kept, "stream_bytes": nbytes,
            "ms_call": round(total, 4), "ms_call_min": round(total_min, 4), "ms_scan": round(scan, 4),
            "ms_copy": round(total - scan, 4), "read_bytes": rd, "write_bytes": wr,
            "tbs_call": tbs(rd + wr, total), "tbs_copy_pass": tbs(rd + wr, total - scan),
            "d2d_ms": round(d2d, 4), "d2d_tbs_moved": tbs(2 * nbytes, d2d),
            "call_over_d2d": round(total / d2d, 2) if d2d > 0 else None}), flush=True)


if __name__ == "__main__":
    small = "--small" in sys.argv
    run("udp64 2^%d" % (18 if small else 24), synth.make_udp64(1 << (18 if small else 24)))
    run("imix 2^%d" % (16 if small else 22), synth.make_imix(1 << (16 if small else 22)))
