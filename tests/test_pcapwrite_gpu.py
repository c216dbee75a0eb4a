"""gpd_pcap_write / gpd_batch_select on the device against the checker (tests/pcapwrite_ref.py):
every comparison is exact equality, and every output buffer is carved from a larger one filled
with 0xA5 whose bytes at or beyond the reported length must survive the call.

The scan's workgroup takes SCAN_BLOCK packets (kScanBlock, gpd_write_scan.h) and the kernel
that scans the block totals takes 1024 of them per round, so the sizes at which the code takes
another path are 64 (a wave), SCAN_BLOCK, and 1024 * SCAN_BLOCK packets.

On the input side the bounds are checked by reading the code (src16_of issues a load only where it
starts inside [0, round_up(data_len, 16))); the "end" layout documents the case: its last packet
ends exactly at data_len and the device buffer ends at round_up(data_len, 16).
"""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

import golden_cases as G
import oracle_ref as O
import pcapwrite_ref as WR
from gopacket_amd import layers as L
from gopacket_amd import pcap, synth
from gopacket_amd.batch import PacketBatch
from test_parity_gpu import ALL, _parser, assert_same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "pcapgo_write_vectors.json")))
CAPTURES = ["test_dns.pcap", "test_ethernet.pcap", "test_loopback.pcap"]
SCAN_BLOCK = 1024
GUARD = 64
GPD_ERR_INVALID, GPD_ERR_PCAP = -1, -5
NANOS, FILE_HEADER = 1, 2


def _mods():
    import torch
    from gopacket_amd import parser as P
    from gopacket_amd import pcapwrite as PW
    return torch, P, PW


def _t(a):
    """A numpy array on the device (unsigned types as their signed twins)."""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    twin = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(twin) if twin else a).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Dev:
    """A batch, its capture infos and a context on the device, for raw C-ABI calls."""

    def __init__(self, batch, ts, length=None, exact_buffer=False):
        torch, P, PW = _mods()
        self.lib, self.p = PW.pw_lib(), _parser()
        if exact_buffer:  # the device buffer ends at round_up(data_len, 16)
            lim = (batch.data_len + 15) // 16 * 16
            batch = PacketBatch(batch.data[:lim], batch.data_len, batch.offset, batch.caplen)
            self.db = P.DeviceBatch.from_tensors(_t(batch.data), batch.data_len, _t(batch.offset),
                                                 _t(batch.caplen))
        else:
            self.db = P.DeviceBatch(batch)
        self.batch, self.ts, self.length = batch, ts, length
        self.d_ts, self.d_len = _t(ts), _t(length)

    def write(self, keep=None, flags=0, header=(0, 0), cap=None, use_length=True):
        """(rc, records, bytes, bad index, the whole guarded buffer on the host)."""
        torch = _mods()[0]
        if cap is None:  # exactly what the checker's stream takes
            cap = len(WR.write(self.batch, self.ts, self.length if use_length else None, keep,
                               bool(flags & NANOS), header if flags & FILE_HEADER else None)[0])
        big = torch.full(((cap + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        nw, nb, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
        b = self.db.c_batch()
        d_keep = _t(keep)
        rc = self.lib.gpd_pcap_write(self.p.ctx().h, C.byref(b), _ptr(self.d_ts),
                                     _ptr(self.d_len) if use_length else None, _ptr(d_keep), flags,
                                     header[0], header[1], _ptr(big), cap, C.byref(nw), C.byref(nb), C.byref(bad),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, nw.value, nb.value, bad.value, big.cpu().numpy()

    def check_write(self, keep=None, flags=0, header=(0, 0), use_length=True):
        ref, rn, rbad = WR.write(self.batch, self.ts, self.length if use_length else None, keep,
                                 bool(flags & NANOS), header if flags & FILE_HEADER else None)
        rc, nw, nb, bad, buf = self.write(keep, flags, header, cap=len(ref), use_length=use_length)
        assert rc == (GPD_ERR_PCAP if rbad != WR.NO_BAD else 0), self.lib.gpd_last_error_string()
        assert (nw, nb, bad) == (rn, len(ref), rbad)
        assert buf[:nb].tobytes() == ref
        assert (buf[nb:] == 0xA5).all(), "a byte at or beyond *bytes was written"
        return ref

    def select(self, keep=None, cap=None, max_out=None):
        """(rc, packets, bytes, guarded data buffer, offsets, caplens, indices)."""
        torch = _mods()[0]
        data, off, ln, idx = WR.select(self.batch, keep)
        cap = len(data) if cap is None else cap
        m = len(idx) if max_out is None else max_out
        big = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        o, c, x = (torch.full((m + 4,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
        k, nb = C.c_uint64(), C.c_uint64()
        b = self.db.c_batch()
        d_keep = _t(keep)
        rc = self.lib.gpd_batch_select(self.p.ctx().h, C.byref(b), _ptr(d_keep), _ptr(big), cap, _ptr(o), _ptr(c),
                                       _ptr(x), m, C.byref(k), C.byref(nb),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        u = lambda t: t.cpu().numpy().view(np.uint32)
        return rc, k.value, nb.value, big.cpu().numpy(), u(o), u(c), u(x)

    def check_select(self, keep=None):
        data, off, ln, idx = WR.select(self.batch, keep)
        rc, k, nb, buf, o, c, x = self.select(keep)
        assert rc == 0, self.lib.gpd_last_error_string()
        assert (k, nb) == (len(idx), len(data))
        assert buf[:nb].tobytes() == data
        assert (buf[nb:] == 0xA5).all(), "a byte at or beyond round_up(*bytes, 16) was written"
        assert (o[:k] == off).all() and (c[:k] == ln).all() and (x[:k] == idx).all()
        assert (o[k:] == 0xFFFFFFFF).all() and (c[k:] == 0xFFFFFFFF).all() and (x[k:] == 0xFFFFFFFF).all()
        assert (o[:k] % 16 == 0).all() and (np.diff(o[:k].astype(np.int64)) >= 0).all()


# ---- 1. the reference's record vector -----------------------------------------------------------
def test_reference_record_vector_on_device():
    v = VEC["packet"]
    b = PacketBatch.from_packets([bytes.fromhex(v["data"])])
    d = Dev(b, np.array([v["ts_ns"]], np.uint64), np.array([v["length"]], np.uint32))
    want = bytes.fromhex(v["hex"])
    assert d.check_write() == want
    assert d.check_write(flags=NANOS) == want[:4] + (0xAA * 1000).to_bytes(4, "little") + want[8:]


# ---- 2. the golden captures, byte for byte ------------------------------------------------------
@pytest.mark.parametrize("name", CAPTURES)
def test_golden_capture_roundtrips_through_device(name):
    torch, P, PW = _mods()
    raw = open(os.path.join(HERE, "golden", name), "rb").read()
    p = pcap.index(pcap.capture_array(raw))
    d = Dev(p.batch, p.ts_ns, p.length)
    assert d.check_write(flags=FILE_HEADER, header=(p.snaplen, p.linktype)) == raw
    # and through the Python surface: file header by the Writer, records by the device
    buf = io.BytesIO()
    w = PW.NewWriter(buf)
    w.WriteFileHeader(p.snaplen, p.linktype)
    assert w.WritePackets(d.db, p.ts_ns, p.length, parser=d.p) == p.batch.n
    assert buf.getvalue() == raw
    stream, n = PW.write_device(d.p, d.db, d.d_ts, d.d_len, None, file_header=(p.snaplen, p.linktype))
    assert n == p.batch.n and stream.is_cuda and stream.cpu().numpy().tobytes() == raw


# ---- 3. + 4. the shape sweep, with guard bytes ---------------------------------------------------
CAPLENS = [0, 1, 15, 16, 17, 48, 64, 1500, 65535]
COUNTS = [0, 1, 63, 64, 65, 4097, 2 * SCAN_BLOCK + 77]
LAYOUTS = ["aligned16", "packed1", "shuffled", "overlapping", "ends_at_data_len"]


def _sweep_batch(n, layout):
    """n packets with caplens drawn from CAPLENS; from 63 packets on every one of them is
    present (the large ones twice only, so that the batch stays small) with one 70,000-byte
    packet."""
    rng = np.random.default_rng(1000 * n + LAYOUTS.index(layout))
    lens = [CAPLENS[j] for j in rng.integers(0, 9 if n < 63 else 7, n)]
    if n >= 63:
        for j, c in enumerate(CAPLENS + [70000, 65535, 1500]):
            lens[n * (j + 1) // 14] = c
    if layout == "ends_at_data_len" and n:
        lens[-1] = max(lens[-1], 5)  # the packet whose 16-byte reads hang over data_len
    pk = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in lens]
    if layout == "aligned16":
        return PacketBatch.from_packets(pk)
    b = PacketBatch.from_packets(pk, align=1)
    if layout == "shuffled":
        order = rng.permutation(n)
        return PacketBatch(b.data, b.data_len, b.offset[order].copy(), b.caplen[order].copy())
    if layout == "overlapping":  # every odd descriptor on the bytes of the one before it
        off, ln = b.offset.copy(), b.caplen.copy()
        m = n // 2
        off[1:2 * m:2], ln[1:2 * m:2] = off[0:2 * m:2], ln[0:2 * m:2]
        return PacketBatch(b.data, b.data_len, off, ln)
    return b


def _masks(n):
    rng = np.random.default_rng(n)
    z = lambda: np.zeros(n, np.uint8)
    m_alt, m_first, m_last, m_run, m_vals = z(), z(), z(), np.ones(n, np.uint8), z()
    m_alt[::2] = 1
    m_first[:1] = 1
    m_last[-1:] = 1
    m_run[20:220] = 0  # 200 unkept packets: whole waves with nothing to do
    m_vals[::3], m_vals[1::3] = 0x80, 0xFF
    return {"null": None, "ones": np.ones(n, np.uint8), "zeros": z(), "alternating": m_alt,
            "first": m_first, "last": m_last, "random8": (rng.integers(0, 8, n) == 0).astype(np.uint8),
            "run200": m_run, "values": m_vals}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", COUNTS)
def test_shape_sweep(n, layout):
    b = _sweep_batch(n, layout)
    if layout == "ends_at_data_len" and n:
        assert int(b.offset[-1]) + int(b.caplen[-1]) == b.data_len
    rng = np.random.default_rng(n + 5)
    ts = rng.integers(0, 1 << 62, n).astype(np.uint64)
    length = b.caplen + rng.integers(0, 3, n).astype(np.uint32)
    d = Dev(b, ts, length, exact_buffer=(layout == "ends_at_data_len"))
    for name, keep in _masks(n).items():
        for flags in (0, NANOS, FILE_HEADER, NANOS | FILE_HEADER):  # records start at 0 and at 8 mod 16
            d.check_write(keep, flags, (262144, 1), use_length=(name != "ones"))
        d.check_select(keep)


@pytest.mark.parametrize("n", [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_scan_block_edge(n):
    """One block, one block exactly, and a second block of one packet (COUNTS steps from 65 to
    4097).  The selection reads the shared scan's block and wave prefixes of the kept counts."""
    b = _sweep_batch(n, "packed1")
    rng = np.random.default_rng(n + 6)
    ts = rng.integers(0, 1 << 62, n).astype(np.uint64)
    d = Dev(b, ts, b.caplen + rng.integers(0, 3, n).astype(np.uint32))
    masks = _masks(n)
    for name in ("null", "alternating", "last"):
        for flags in (0, FILE_HEADER):
            d.check_write(masks[name], flags, (262144, 1))
        d.check_select(masks[name])


def test_scan_carry_beyond_1024_blocks():
    """More than 1024 * SCAN_BLOCK packets: the block totals' scan takes a second round, its
    carry forwards (positions) and backwards (the next kept packet)."""
    n = 1024 * SCAN_BLOCK + 1500
    rng = np.random.default_rng(11)
    ln = np.array([0, 1, 15, 16, 17], np.uint32)[rng.integers(0, 5, n)]
    off = np.zeros(n, np.int64)
    np.cumsum(ln[:-1], out=off[1:])
    total = int(off[-1] + ln[-1])
    data = rng.integers(0, 256, total + 64, dtype=np.uint8)
    b = PacketBatch(data, total, off.astype(np.uint32), ln)
    keep = (rng.integers(0, 8, n) == 0).astype(np.uint8)
    keep[SCAN_BLOCK * 1020:SCAN_BLOCK * 1024 + 700] = 0  # the next kept packet lies a round away
    d = Dev(b, rng.integers(0, 1 << 62, n).astype(np.uint64), None)
    d.check_write(keep, FILE_HEADER, (65535, 1))
    d.check_select(keep)


# ---- 5. stop semantics ----------------------------------------------------------------------------
def test_stop_at_first_kept_packet_with_caplen_above_length():
    torch, P, PW = _mods()
    rng = np.random.default_rng(3)
    n = 700
    pk = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 90, n)]
    b = PacketBatch.from_packets(pk, align=1)
    ts = rng.integers(0, 1 << 62, n).astype(np.uint64)
    length = b.caplen.copy()
    length[333] -= 1
    d = Dev(b, ts, length)
    ref = d.check_write()  # asserts GPD_ERR_PCAP, bad index 333, 333 records, prefix, guard bytes
    assert len(ref) == 16 * 333 + int(b.caplen[:333].sum())
    text = d.lib.gpd_last_error_string().decode()
    assert text == (f"invalid capture info (packet 333: capture length {int(b.caplen[333])}, "
                    f"length {int(length[333])}):  capture length > length")
    keep = np.ones(n, np.uint8)
    keep[333] = 0
    d.check_write(keep)  # the same packet unkept: no error
    rc, nw, nb, bad, _ = d.write(keep)
    assert (rc, nw, bad) == (0, n - 1, WR.NO_BAD)
    length2 = length.copy()
    length2[100] = 0
    length2[650] = 0
    d2 = Dev(b, ts, length2)
    rc, nw, nb, bad, _ = d2.write()
    assert (rc, nw, bad) == (GPD_ERR_PCAP, 100, 100)  # the lowest of three
    d2.check_write(flags=NANOS | FILE_HEADER, header=(1, 1))
    keep = np.ones(n, np.uint8)
    keep[100] = 0
    rc, nw, nb, bad, _ = d2.write(keep)
    assert (rc, nw, bad) == (GPD_ERR_PCAP, 332, 333)
    # the Python surface: the records before the rejected packet are written, then the error
    buf = io.BytesIO()
    with pytest.raises(pcap.PcapError) as e:
        PW.NewWriter(buf).WritePackets(d.db, ts, d.length, parser=d.p)
    assert buf.getvalue() == ref and e.value.bad_index == 333 and e.value.n_written == 333
    with pytest.raises(Exception):  # ts_ns = NULL is refused
        PW.write_device(d.p, d.db, None)


# ---- 6. capacity ----------------------------------------------------------------------------------
def test_capacity_one_byte_short_writes_nothing():
    rng = np.random.default_rng(4)
    pk = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 200, 300)]
    b = PacketBatch.from_packets(pk)
    d = Dev(b, rng.integers(0, 1 << 62, 300).astype(np.uint64))
    ref, rn, _ = WR.write(b, d.ts, None, None, False, (9, 1))
    rc, nw, nb, bad, buf = d.write(flags=FILE_HEADER, header=(9, 1), cap=len(ref) - 1)
    assert rc == GPD_ERR_INVALID and (nw, nb, bad) == (rn, len(ref), WR.NO_BAD)
    text = d.lib.gpd_last_error_string().decode()
    assert str(len(ref)) in text and str(len(ref) - 1) in text
    assert (buf == 0xA5).all()
    data, off, ln, idx = WR.select(b, None)
    rc, k, nb, buf, o, c, x = d.select(None, cap=len(data) - 16)
    assert rc == GPD_ERR_INVALID and (k, nb) == (300, len(data))
    assert (buf == 0xA5).all() and (o == 0xFFFFFFFF).all()
    rc, k, nb, buf, o, c, x = d.select(None, max_out=299)
    assert rc == GPD_ERR_INVALID and (buf == 0xA5).all() and (o == 0xFFFFFFFF).all()


# ---- 7. select ------------------------------------------------------------------------------------
def test_select_golden_packets_and_decode_parity():
    torch, P, PW = _mods()
    from gopacket_amd.results import BatchResult
    pk = [G.case_bytes(c) for c in G.load()["cases"]] * 3
    b = PacketBatch.from_packets(pk, align=1)
    keep = (np.random.default_rng(5).integers(0, 3, b.n) == 0).astype(np.uint8)
    d = Dev(b, np.zeros(b.n, np.uint64))
    d.check_select(keep)
    d.check_select(None)
    sel, index = PW.select(d.p, d.db, keep)
    idx = np.nonzero(keep)[0]
    assert sel.n == len(idx) and (index.cpu().numpy() == idx).all()
    off, ln = sel.offset.cpu().numpy().view(np.uint32), sel.caplen.cpu().numpy().view(np.uint32)
    data = sel.data.cpu().numpy()
    assert sel.caplen.data_ptr() == sel.offset.data_ptr() + 4 * (sel.n + (-sel.n) % 16)
    for j, i in enumerate(idx):
        assert data[off[j]:off[j] + ln[j]].tobytes() == pk[i]
    # decoding the selected batch on the device = the oracle's results for those packets
    ref = O.decode(b, L.LayerTypeEthernet, ALL, 0, ext=False, nthreads=8)
    sub = BatchResult(*[None if a is None else a[idx] for a in
                        (ref.status, ref.layers, ref.net_hash, ref.tp_hash, ref.csum, None, ref.hdr_off, None)])
    dres = P.DeviceResult(sel.n)
    d.p.decode_device(sel, dres)
    torch.cuda.synchronize()
    assert_same(dres.to_host(), sub, ext=False)


def test_select_empty():
    torch, P, PW = _mods()
    b = PacketBatch.from_packets([b"abc", b"defg"])
    d = Dev(b, np.zeros(2, np.uint64))
    d.check_select(np.zeros(2, np.uint8))
    sel, index = PW.select(d.p, d.db, np.zeros(2, np.uint8))
    assert sel.n == 0 and sel.data_len == 0 and index.numel() == 0
    e = Dev(PacketBatch.from_packets([]), np.zeros(0, np.uint64))
    rc, k, nb, buf, o, c, x = e.select(None)
    assert (rc, k, nb) == (0, 0, 0) and (buf == 0xA5).all()
    sel, index = PW.select(e.p, e.db, None)
    assert sel.n == 0 and index.numel() == 0


# ---- 8. read-back property (the one larger size) ---------------------------------------------------
def test_readback_imix_one_eighth():
    torch, P, PW = _mods()
    n = 1 << 16
    b = synth.make_imix(n)
    rng = np.random.default_rng(8)
    ts = (rng.integers(0, 1 << 31, n).astype(np.uint64) * np.uint64(1000000000)
          + rng.integers(0, 1000000000, n).astype(np.uint64))
    length = b.caplen + rng.integers(0, 100, n).astype(np.uint32)
    keep = (rng.integers(0, 8, n) == 0).astype(np.uint8)
    idx = np.nonzero(keep)[0]
    p = _parser()
    db = P.DeviceBatch(b)
    for nanos in (False, True):
        stream, nw = PW.write_device(p, db, ts, length, keep, nanos=nanos, file_header=(262144, 1))
        raw = stream.cpu().numpy()
        assert nw == len(idx)
        got = pcap.index(pcap.capture_array(raw))
        assert got.err is None and got.batch.n == len(idx) and got.nano == nanos
        assert (got.batch.caplen == b.caplen[idx]).all() and (got.length == length[idx]).all()
        want_ts = ts[idx] if nanos else ts[idx] // np.uint64(1000) * np.uint64(1000)
        assert (got.ts_ns == want_ts).all()
        for j, i in enumerate(idx):
            o, s, k = int(got.batch.offset[j]), int(b.offset[i]), int(b.caplen[i])
            assert (raw[o:o + k] == b.data[s:s + k]).all(), i
        assert raw.tobytes() == WR.write(b, ts, length, keep, nanos, (262144, 1))[0]


# ---- 9. flow filter -------------------------------------------------------------------------------
def test_flow_filter_writes_one_flow_in_order():
    torch, P, PW = _mods()
    from gopacket_amd import flows
    mix = synth.make_traffic_mix(300)
    pick = np.random.default_rng(9).integers(0, 40, 3000) * 7  # 40 distinct packets, many times each
    b = PacketBatch.from_packets([mix.packet(int(i)) for i in pick])
    p = _parser()
    db, dr = P.DeviceBatch(b), P.DeviceResult(b.n)
    p.decode_device(db, dr)
    ids = flows.NewFlowTable(p, 1 << 14).Insert(db, dr)
    torch.cuda.synchronize()
    valid = ids[ids >= 0]  # (the GPD_FLOW_* values are negative as int32)
    assert valid.numel() > 0
    k = int(torch.bincount(valid.to(torch.int64)).argmax())
    keep = ids == k  # a bool tensor on the device
    ts = np.arange(b.n, dtype=np.uint64) * np.uint64(1000)
    stream, nw = PW.write_device(p, db, ts, None, keep)
    host_keep = keep.cpu().numpy().astype(np.uint8)
    assert nw == int(host_keep.sum()) and nw > 1
    assert stream.cpu().numpy().tobytes() == WR.write(b, ts, None, host_keep)[0]
