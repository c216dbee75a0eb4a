"""The per-packet result arrays through every staged entry point, one array set at a time.

The host runtime handles each result array (status, layers, net_hash, tp_hash, csum, hdr_off,
ext, detail) in several places per pipeline: device buffers, pinned staging, the "every array
registered?" test, the device-to-host copies and the drain into the caller's arrays.  The other
GPU tests pass every array, staged or all registered.  Here each entry point runs with the
optional arrays absent, with all of them, with only two of them registered (so the results
are staged although some arrays could take a direct copy), with all of them registered
(direct), and, for gpd_decode_host, with ext records beside registered arrays.

Every passed array must equal the CPU oracle's.  Every passed array is 64 elements longer than
the call needs and pre-filled with 0xA5; the 64 extra elements must come back untouched, which
a wrong element width or offset for one array would break.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ng_synth as S
import oracle_ref as O
from gopacket_amd import layers as L
from gopacket_amd import pcap as NP
from gopacket_amd import synth
from gopacket_amd.batch import PAD, PacketBatch
from gopacket_amd.results import DETAIL_DTYPE, EXT_DTYPE

pytestmark = pytest.mark.gpu

ALL = 0xFFF   # every decoder (gpd.h GPD_DEC_ALL)
N = 3000      # packets per call: the logic under test is per array, not per packet
GUARD = 64    # extra elements behind each array
CHUNK = 65536  # pcapng chunk_bytes: the capture spans several chunks on both slots

DTYPES = {"status": np.uint32, "layers": np.uint64, "net_hash": np.uint64, "tp_hash": np.uint64,
          "csum": np.uint32, "ext": EXT_DTYPE, "hdr_off": np.uint32, "detail": DETAIL_DTYPE}
SOA = ("status", "layers", "net_hash", "tp_hash", "csum", "hdr_off")
SETS = {  # name: (arrays passed, arrays registered)
    "core": (("status", "layers"), ()),
    "all": (SOA + ("detail",), ()),
    "partial": (SOA + ("detail",), ("status", "csum")),
    "direct": (SOA + ("detail",), SOA + ("detail",)),
    "ext": (SOA + ("detail", "ext"), SOA + ("detail",)),
}
ENTRIES = ("host_span", "host_repack", "pcap_host_walk", "pcap_device_walk", "pcapng",
           "tpv3_host_walk", "tpv3_device_walk")


@functools.lru_cache(maxsize=None)
def _parser():
    from gopacket_amd import parser as P
    p = P.DecodingLayerParser(L.LayerTypeEthernet)
    p._mask = ALL
    return p


@functools.lru_cache(maxsize=None)
def _inputs():
    """The batch (error packets among it, so detail has content), its oracle decode, and the
    same packets as a shuffled batch, a pcap capture, a pcapng capture and a TPACKET_V3 ring."""
    import error_sites as ES
    sites = ES.packets()
    m = synth.make_mixed(N - len(sites))
    pk = [m.packet(i) for i in range(m.n)]
    for k, p in enumerate(sites):  # one packet per reference error site, spread among the rest
        pk.insert(23 * k + 7, p)
    b = PacketBatch.from_packets(pk)
    assert b.n == N
    ref = O.decode(b, L.LayerTypeEthernet, ALL, 0, ext=True, nthreads=8)
    perm = np.random.default_rng(7).permutation(N)
    shuffled = PacketBatch(b.data, b.data_len, b.offset[perm].copy(), b.caplen[perm].copy())
    pk = [b.packet(i) for i in range(N)]
    cap = NP.synth_capture(b)
    ng = NP.capture_array(S.shb() + S.idb("<", 1, 0) + b"".join(S.epb(p, ts=i) for i, p in enumerate(pk)))
    assert ng.nbytes > 3 * CHUNK
    ring, used = synth.make_tpv3_ring(pk, 1 << 16, 64)
    return b, ref, perm, shuffled, cap, ng, ring


def _array(name):
    """N + GUARD elements of 0xA5 bytes, page-aligned in pages of their own (registrable)."""
    nbytes = (N + GUARD) * np.dtype(DTYPES[name]).itemsize
    raw = np.empty(nbytes + 2 * 4096, np.uint8)
    lo = -raw.ctypes.data % 4096
    a = raw[lo:lo + nbytes]
    a[:] = 0xA5
    return a.view(DTYPES[name])


def _call(entry, r):
    """Runs the entry point over the N packets into the gpd_result r; returns the oracle order."""
    from gopacket_amd import afpacket, pcapng
    from gopacket_amd._lib import GpdBatch, check, lib
    b, ref, perm, shuffled, cap, ng, ring = _inputs()
    p = _parser()
    n, nxt, stop, nb = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint32()
    order = np.arange(N)
    if entry.startswith("host"):
        src = b if entry == "host_span" else shuffled
        if src is shuffled:
            order = perm
        gb = GpdBatch(src.data.ctypes.data, src.data_len, src.offset.ctypes.data, src.caplen.ctypes.data, N)
        check(lib.gpd_decode_host(p.ctx().h, C.byref(gb), C.byref(r)), entry)
        return order
    if entry.startswith("pcap_"):
        p.Tuning = {"device_walk": int(entry == "pcap_device_walk")}
        dl = cap.shape[0] - PAD
        info = NP.header(cap, dl)
        check(lib.gpd_decode_pcap_at(p.ctx().h, cap.ctypes.data, dl, C.byref(info), 24, N, C.byref(r),
                                     C.byref(n), C.byref(nxt), C.byref(stop), 8), entry)
        wc = np.zeros(7, np.uint32)
        lib.gpd_decode_pcap_last_walk_counts(wc.ctypes.data)
        assert (wc[0] > 0) == (entry == "pcap_device_walk") and wc[1] == 0, wc
        assert n.value == N
        return order
    if entry == "pcapng":
        rd = pcapng.NgReader(ng, pcapng.NgReaderOptions(device_walk=-1, chunk_bytes=CHUNK))
        check(pcapng.ng_lib().gpd_decode_pcapng(p.ctx().h, rd.h, N, C.byref(r), C.byref(n), C.byref(stop), 8),
              entry)
        c = pcapng.last_walk_counts()
        assert n.value == N and c[0] >= 3 and c[1] == 0, c  # three chunks or more, all the device's
        return order
    dw = int(entry == "tpv3_device_walk")
    p.Tuning = {"device_walk": dw}
    tr = afpacket.TPv3Ring(ring, 1 << 16, 64)
    check(lib.gpd_decode_tpv3(p.ctx().h, C.byref(tr.c), 0, 64, 0, N, C.byref(r), None, C.byref(n),
                              C.byref(nb), 8), entry)
    assert n.value == N and lib.gpd_decode_tpv3_last_path() == dw
    return order


@pytest.mark.parametrize("rset", ["core", "all", "partial", "direct"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_result_arrays(entry, rset):
    _run(entry, rset)


@pytest.mark.parametrize("entry", ["host_span", "host_repack"])
def test_ext_beside_registered_arrays(entry):
    _run(entry, "ext")


def _run(entry, rset):
    from gopacket_amd._lib import GpdResult, check, lib
    from test_parity_gpu import detail_rows
    passed, registered = SETS[rset]
    ref = _inputs()[1]
    arr = {f: _array(f) for f in passed}
    ptr = lambda f: arr[f].ctypes.data if f in arr else None
    r = GpdResult(ptr("status"), ptr("layers"), ptr("net_hash"), ptr("tp_hash"), ptr("csum"), ptr("ext"),
                  ptr("hdr_off"), None, ptr("detail"))
    h = _parser().ctx().h
    done = []
    try:
        for f in registered:
            check(lib.gpd_host_register(h, arr[f].ctypes.data, arr[f].nbytes), "register " + f)
            done.append(f)
        order = _call(entry, r)
    finally:
        for f in done:
            lib.gpd_host_unregister(h, arr[f].ctypes.data)
    for f in passed:
        guard = arr[f][N:].view(np.uint8)
        assert (guard == 0xA5).all(), f"{f}: the {GUARD} elements behind the array were written"
        got = arr[f][:N].view(np.uint8).reshape(N, -1)
        if f == "detail":  # written for decode errors and deep stacks only: the ext record's head
            rows = detail_rows(ref.status[order])
            assert len(rows) > 0
            want = ref.ext[order].view(np.uint8).reshape(N, -1)[:, :DETAIL_DTYPE.itemsize]
            got, want = got[rows], want[rows]
        else:
            want = np.ascontiguousarray(getattr(ref, f)[order]).view(np.uint8).reshape(N, -1)
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        assert len(bad) == 0, f"{f} differs from the oracle at {len(bad)} packets, first {int(bad[0])}"
