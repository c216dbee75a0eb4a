"""Time gpd_pcapng_write beside gpd_pcap_write on the same HBM-resident batch in
one process: 2^24 x 64-B UDP frames and 2^22 IMIX frames, each with every packet kept and with a
random 1/8 mask (the workloads of §5g's table, tools/pcapwrite_time.py).  HIP events on the call's
stream after warm-up, the median of 20: the whole call, and the sizing call (the scan alone)
whose time is taken off for the copy.  Beside each, a device-to-device hipMemcpyAsync of as many
bytes as the pcapng stream has.  The pcapng call carries a prefix (a section block and two
interface blocks) and an interface index per packet.  The algorithmic bytes are reads of 25 B of
descriptors per packet (offset, caplen, ts, length, ifindex, keep; 21 B for the pcap form) plus
the kept packets' bytes, and writes of the stream.  One JSON line per workload and mask.

    python tools/pcapngwrite_time.py [--small]      (--small: 2^18 / 2^16 packets, a quick check)
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopacket_amd import layers as L, pcapng as NG, synth  # noqa: E402
from gopacket_amd import parser as P, pcapwrite as PW  # noqa: E402
from pcapwrite_time import hip_runtime, median_ms  # noqa: E402


def run(name, batch, reps=20):
    n = batch.n
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    db = P.DeviceBatch(batch, 0)
    rng = np.random.default_rng(1)
    ts = torch.from_numpy((np.arange(n, dtype=np.int64) * 1000)).cuda()
    length = db.caplen.clone()
    ifx = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32)).cuda()
    masks = {"all": torch.ones(n, dtype=torch.uint8, device="cuda"),
             "random 1/8": torch.from_numpy((rng.integers(0, 8, n) == 0).astype(np.uint8)).cuda()}
    prefix = (PW.ng_section_block(PW.DefaultNgWriterOptions.SectionInfo) +
              PW.ng_interface_block(PW.DefaultNgInterface) + PW.ng_interface_block(NG.NgInterface(Name=b"intf1")))
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    s = torch.cuda.current_stream()
    lib, h, b = PW.ngw_lib(), p.ctx().h, db.c_batch()
    PW.pw_lib()
    padded_sum = int(((db.caplen.to(torch.int64) + 3) & ~3).sum())
    out = torch.empty(len(prefix) + 32 * n + padded_sum + 16, dtype=torch.uint8, device="cuda")
    src = torch.empty_like(out)
    nw, nb, bad, why = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(s.cuda_stream)
    for mname, keep in masks.items():
        def ng(dst, cap):
            rc = lib.gpd_pcapng_write(h, C.byref(b), ptr(ts), ptr(length), ptr(ifx), 2, ptr(keep), prefix, len(prefix),
                                      dst, cap, C.byref(nw), C.byref(nb), C.byref(bad), C.byref(why), st)
            assert rc == 0, lib.gpd_last_error_string()

        def pc(dst, cap):
            rc = lib.gpd_pcap_write(h, C.byref(b), ptr(ts), ptr(length), ptr(keep), PW.GPD_PCAPW_FILE_HEADER,
                                    262144, 1, dst, cap, C.byref(nw), C.byref(nb), C.byref(bad), st)
            assert rc == 0, lib.gpd_last_error_string()
        res = {}
        for form, call in (("pcapng", ng), ("pcap", pc)):
            for _ in range(3):
                call(ptr(out), out.numel())
            total, total_min = median_ms(lambda: call(ptr(out), out.numel()), s, reps)
            scan, _ = median_ms(lambda: call(None, 0), s, reps)
            res[form] = (total, total_min, scan, nb.value, nw.value)
        total, total_min, scan, nbytes, kept = res["pcapng"]
        p_total, p_min, p_scan, p_bytes, _ = res["pcap"]
        copy_fn = lambda: hip.hipMemcpyAsync(ptr(out), ptr(src), nbytes, 3, st)
        for _ in range(3):
            copy_fn()
        d2d, _ = median_ms(copy_fn, s, reps)
        kept_bytes = p_bytes - 24 - 16 * kept
        rd, wr = 25 * n + kept_bytes, nbytes
        tbs = lambda byts, ms: round(byts / ms / 1e9, 3) if ms > 0 else None
        print(json.dumps({
            "workload": name, "mask": mname, "n": n, "kept": kept, "stream_bytes": nbytes,
            "ms_call": round(total, 4), "ms_call_min": round(total_min, 4), "ms_scan": round(scan, 4),
            "ms_copy": round(total - scan, 4), "read_bytes": rd, "write_bytes": wr,
            "tbs_call": tbs(rd + wr, total), "d2d_ms": round(d2d, 4), "d2d_tbs_moved": tbs(2 * nbytes, d2d),
            "call_over_d2d": round(total / d2d, 2) if d2d > 0 else None,
            "pcap_stream_bytes": p_bytes, "pcap_ms_call": round(p_total, 4), "pcap_ms_call_min": round(p_min, 4),
            "pcap_ms_scan": round(p_scan, 4),
            "ns_per_stream_byte": round(total * 1e6 / nbytes, 6), "pcap_ns_per_stream_byte": round(p_total * 1e6 / p_bytes, 6),
            "per_byte_ratio_ng_over_pcap": round((total / nbytes) / (p_total / p_bytes), 3)}), flush=True)


if __name__ == "__main__":
    small = "--small" in sys.argv
    run("udp64 2^%d" % (18 if small else 24), synth.make_udp64(1 << (18 if small else 24)))
    run("imix 2^%d" % (16 if small else 22), synth.make_imix(1 << (16 if small else 22)))
