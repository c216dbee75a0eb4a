"""gpd_pcapng_write on the device against the checker (tests/pcapngwrite_ref.py): every
comparison is exact equality, and every output buffer is carved from a larger one filled with
0xA5 whose bytes at or beyond the reported length must survive the call.

The scan's workgroup takes SCAN_BLOCK packets (kScanBlock, gpd_write_scan.h) and the kernel
that scans the block totals takes 1024 of them per round, so the sizes at which the code takes
another path are 64 (a wave), SCAN_BLOCK, and 1024 * SCAN_BLOCK packets.  A record is a multiple
of 4 bytes, so the first record starts at prefix_len mod 16 in {0, 4, 8, 12}.

On the input side the bounds are checked by reading the code (src16_of issues a load only where it
starts inside [0, round_up(data_len, 16))); the "end" layout documents the case.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

import pcapngwrite_ref as R
import pcapwrite_ref as WR
from gopacket_amd.batch import PacketBatch
from test_parity_gpu import _parser

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCAN_BLOCK = 1024
GUARD = 64
GPD_ERR_INVALID, GPD_ERR_PCAP = -1, -5
REAL_PREFIX = (R.section_block(b"amd64", b"linux", b"gopacket") + R.interface_block(1, 0, b"intf0", os_=b"linux") +
               R.interface_block(0, 96, b"lo", filter_=b"none", tsoffset=100))
PREFIXES = [b"", bytes(range(1, 5)), bytes(range(1, 9)), bytes(range(1, 13)), bytes(range(1, 17)),
            bytes(range(1, 21)), REAL_PREFIX]


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

    def __init__(self, batch, ts, length=None, ifindex=None, exact_buffer=False, parser=None):
        torch, P, PW = _mods()
        self.lib, self.p = PW.ngw_lib(), parser or _parser()
        if exact_buffer:  # the device buffer ends at round_up(data_len, 16)
            lim = (batch.data_len + 15) // 16 * 16
            batch = PacketBatch(batch.data[:lim], batch.data_len, batch.offset, batch.caplen)
            self.db = P.DeviceBatch.from_tensors(_t(batch.data), batch.data_len, _t(batch.offset),
                                                 _t(batch.caplen))
        else:
            self.db = P.DeviceBatch(batch)
        self.batch, self.ts, self.length, self.ifindex = batch, ts, length, ifindex
        self.d_ts, self.d_len, self.d_ifx = _t(ts), _t(length), _t(ifindex)

    def write(self, keep=None, n_ifaces=1, prefix=b"", cap=0, sizing=False, prefix_len=None):
        """(rc, records, bytes, bad index, bad reason, the whole guarded buffer on the host)."""
        torch = _mods()[0]
        big = torch.full(((cap + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        nw, nb, bad, why = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        b = self.db.c_batch()
        d_keep = _t(keep)
        rc = self.lib.gpd_pcapng_write(self.p.ctx().h, C.byref(b), _ptr(self.d_ts), _ptr(self.d_len),
                                       _ptr(self.d_ifx), n_ifaces, _ptr(d_keep), prefix if prefix else None,
                                       len(prefix) if prefix_len is None else prefix_len,
                                       None if sizing else _ptr(big), cap, C.byref(nw), C.byref(nb),
                                       C.byref(bad), C.byref(why), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, nw.value, nb.value, bad.value, why.value, big.cpu().numpy()

    def check_write(self, keep=None, n_ifaces=1, prefix=b""):
        ref, rn, rbad, rwhy = R.write(self.batch, self.ts, self.length, self.ifindex, n_ifaces, keep, prefix)
        rc, nw, nb, bad, why, buf = self.write(keep, n_ifaces, prefix, cap=len(ref))
        assert rc == (GPD_ERR_PCAP if rbad != R.NO_BAD else 0), self.lib.gpd_last_error_string()
        assert (nw, nb, bad, why) == (rn, len(ref), rbad, rwhy)
        got = buf[:nb].tobytes()
        if got != ref:
            k = next(j for j in range(len(ref)) if got[j] != ref[j])
            raise AssertionError(f"first difference at byte {k} of {len(ref)} (prefix {len(prefix)}): "
                                 f"{got[k & ~15:(k & ~15) + 16].hex()} != {ref[k & ~15:(k & ~15) + 16].hex()}")
        assert (buf[nb:] == 0xA5).all(), "a byte at or beyond *bytes was written"
        return ref


# every residue mod 4 and mod 16 of the capture length, 0 included, and a few longer ones
CAPLENS = list(range(0, 20)) + [31, 32, 33, 48, 63, 64, 65, 127, 1500]
COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025]


def _batch(n, seed, lens=None, align=1):
    rng = np.random.default_rng(seed)
    if lens is None:
        lens = [CAPLENS[j] for j in rng.integers(0, len(CAPLENS), n)]
        for j, c in enumerate(CAPLENS):  # from 63 packets on every one of them is present
            if n >= 63:
                lens[n * j // len(CAPLENS)] = c
    pk = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in lens]
    return PacketBatch.from_packets(pk, align=align), rng


def _masks(n):
    rng = np.random.default_rng(n)
    z = lambda: np.zeros(n, np.uint8)
    m_alt, m_first, m_last, m_mid, m_w017 = z(), z(), z(), z(), z()
    m_alt[::2] = 1
    m_first[:1] = 1
    m_last[-1:] = 1
    m_mid[n // 2:n // 2 + 1] = 1  # (512 of 1024: the middle of a block)
    m_w017[5:9] = 1               # wave 0 ...
    m_w017[17 * 64 + 3:17 * 64 + 6] = 1  # ... and wave 17: a run boundary over 16 empty waves
    return {"null": None, "ones": np.ones(n, np.uint8), "zeros": z(), "alternating": m_alt, "first": m_first,
            "last": m_last, "middle": m_mid, "random8": (rng.integers(0, 8, n) == 0).astype(np.uint8),
            "waves0and17": m_w017}


# ---- 1. counts, capture lengths, masks, interfaces ----------------------------------------------
@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_count_sweep(n, align):
    b, rng = _batch(n, 100 * n + align, align=align)
    ts = rng.integers(0, 1 << 64, n, dtype=np.uint64)  # raw bit patterns, the top bit included
    length = b.caplen + rng.integers(0, 3, n).astype(np.uint32)
    for n_ifaces, ifx in ((1, None), (1, np.zeros(n, np.uint32)), (3, rng.integers(0, 3, n).astype(np.uint32))):
        d = Dev(b, ts, length if n_ifaces == 3 else None, ifx)
        for name, keep in _masks(n).items():
            d.check_write(keep, n_ifaces, PREFIXES[(n + len(name)) % 7])


def test_masks_across_waves_and_blocks():
    n = 2 * SCAN_BLOCK + 77
    b, rng = _batch(n, 7)
    d = Dev(b, rng.integers(0, 1 << 64, n, dtype=np.uint64), None, rng.integers(0, 3, n).astype(np.uint32))
    for name, keep in _masks(n).items():
        d.check_write(keep, 3, REAL_PREFIX if name != "alternating" else b"")


def test_all_zero_length_packets():
    for n in (1, 130, SCAN_BLOCK + 1):
        b, rng = _batch(n, n, lens=[0] * n)
        d = Dev(b, rng.integers(0, 1 << 64, n, dtype=np.uint64))
        for prefix in (b"", PREFIXES[1], PREFIXES[3]):
            ref = d.check_write(None, 1, prefix)
            assert len(ref) == len(prefix) + 32 * n
        d.check_write(_masks(n)["alternating"], 1, PREFIXES[2])


def test_mixed_lengths_to_1600():
    n = 3000
    rng = np.random.default_rng(1600)
    b, _ = _batch(n, 1600, lens=rng.integers(0, 1601, n))
    ts = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    d = Dev(b, ts, b.caplen + rng.integers(0, 100, n).astype(np.uint32), rng.integers(0, 3, n).astype(np.uint32))
    d.check_write(None, 3, REAL_PREFIX)
    d.check_write(_masks(n)["random8"], 3, PREFIXES[1])


# ---- 2. the first chunk: every prefix_len mod 16 --------------------------------------------------
@pytest.mark.parametrize("first_kept", [0, 200, SCAN_BLOCK + 70])  # wave 0; a later wave; a later block
def test_prefix_residues(first_kept):
    n = SCAN_BLOCK + 200
    b, rng = _batch(n, 31 + first_kept)
    d = Dev(b, rng.integers(0, 1 << 64, n, dtype=np.uint64))
    keep = np.zeros(n, np.uint8)
    keep[first_kept:] = 1
    for prefix in PREFIXES:
        ref = d.check_write(keep, 1, prefix)
        assert ref[:len(prefix)] == prefix
    for prefix in PREFIXES:  # a prefix and no record at all
        d.check_write(np.zeros(n, np.uint8), 1, prefix)


def test_prefix_on_an_empty_batch():
    e = Dev(PacketBatch.from_packets([]), np.zeros(0, np.uint64))
    for prefix in PREFIXES:
        assert e.check_write(None, 1, prefix) == prefix
        rc, nw, nb, bad, why, buf = e.write(None, 1, prefix, sizing=True)
        assert (rc, nw, nb, bad, why) == (0, 0, len(prefix), R.NO_BAD, 0) and (buf == 0xA5).all()


# ---- 3. stop semantics ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stop_batch():
    n = SCAN_BLOCK + 500
    b, rng = _batch(n, 3, lens=np.random.default_rng(3).integers(1, 90, n))
    return b, rng.integers(0, 1 << 62, n).astype(np.uint64), rng.integers(0, 3, n).astype(np.uint32)


@pytest.mark.parametrize("reason", [R.BAD_IFACE, R.BAD_LENGTH])
@pytest.mark.parametrize("k", [0, 64, 1024, -1])
def test_stop_at_the_first_rejected_kept_packet(stop_batch, k, reason):
    b, ts, ifx = stop_batch
    k %= b.n
    length, ifx = b.caplen.copy(), ifx.copy()
    if reason == R.BAD_IFACE:
        ifx[k] = 3
    else:
        length[k] -= 1
    d = Dev(b, ts, length, ifx)
    ref = d.check_write(None, 3, PREFIXES[2])  # asserts GPD_ERR_PCAP, index, reason, k records, guard bytes
    assert len(ref) == 8 + sum(32 + (int(c) + 3) // 4 * 4 for c in b.caplen[:k])
    text = d.lib.gpd_last_error_string().decode()
    if reason == R.BAD_IFACE:
        assert text == R.IFACE_TEXT % (3, 3) == "Can't send statistics for non existent interface 3; have only 3 interfaces"
    else:
        assert text == R.LENGTH_TEXT % (k, int(b.caplen[k]), int(length[k]))
    keep = np.ones(b.n, np.uint8)
    keep[k] = 0
    d.check_write(keep, 3)  # the same packet unkept: no error
    rc, nw, nb, bad, why, _ = d.write(keep, 3, sizing=True)
    assert (rc, nw, bad, why) == (0, b.n - 1, R.NO_BAD, R.BAD_NONE)


def test_stop_lowest_index_wins_whatever_the_reason(stop_batch):
    torch, P, PW = _mods()
    b, ts, ifx0 = stop_batch
    for lo_reason in (R.BAD_IFACE, R.BAD_LENGTH):
        length, ifx = b.caplen.copy(), ifx0.copy()
        i_if, i_len = (300, 1100) if lo_reason == R.BAD_IFACE else (1100, 300)
        ifx[i_if] = 7
        length[i_len] = 0
        d = Dev(b, ts, length, ifx)
        d.check_write(None, 3, PREFIXES[1])
        rc, nw, nb, bad, why, _ = d.write(None, 3, sizing=True)
        assert (rc, nw, bad, why) == (GPD_ERR_PCAP, 300, 300, lo_reason)
        keep = np.ones(b.n, np.uint8)
        keep[300] = 0
        d.check_write(keep, 3)
        rc, nw, nb, bad, why, _ = d.write(keep, 3, sizing=True)
        assert (rc, nw, bad, why) == (GPD_ERR_PCAP, 1099, 1100, 3 - lo_reason)
    # one packet that fails both checks: the interface check comes first (ngwrite.go:357-365)
    length, ifx = b.caplen.copy(), ifx0.copy()
    ifx[40], length[40] = 3, 0
    d = Dev(b, ts, length, ifx)
    d.check_write(None, 3)
    assert d.write(None, 3, sizing=True)[4] == R.BAD_IFACE
    # ifindex NULL with no interface added: packet 0 is on an interface that does not exist
    d0 = Dev(b, ts)
    d0.check_write(None, 0, PREFIXES[3])
    assert d0.lib.gpd_last_error_string().decode() == R.IFACE_TEXT % (0, 0)
    # the Python surface: the records before the rejected packet are written, then the error
    from gopacket_amd import pcap
    buf = io.BytesIO()
    w = PW.NewNgWriter(buf, 1)
    head = buf.getvalue()
    with pytest.raises(pcap.PcapError) as e:
        w.WritePackets(d.db, ts, length, ifx0 * 0, parser=d.p)
    want = R.write(b, ts, length, None, 1)[0]
    assert buf.getvalue() == head + want and e.value.bad_index == 40 and e.value.n_written == 40
    assert e.value.bad_reason == R.BAD_LENGTH and "capture length > length" in str(e.value)
    with pytest.raises(pcap.PcapError) as e:
        w.WritePackets(d.db, ts, None, ifx0, parser=d.p)  # only interface 0 was added
    assert str(e.value) == R.IFACE_TEXT % (int(ifx0[ifx0 > 0][0]), 1)


# ---- 4. capacity ----------------------------------------------------------------------------------
def test_capacity_sizing_and_scratch_reuse():
    b, rng = _batch(3000, 4)
    d = Dev(b, rng.integers(0, 1 << 62, 3000).astype(np.uint64))
    ref, rn, _, _ = R.write(b, d.ts, prefix=REAL_PREFIX)
    rc, nw, nb, bad, why, buf = d.write(prefix=REAL_PREFIX, cap=len(ref) - 1)
    assert rc == GPD_ERR_INVALID and (nw, nb, bad, why) == (rn, len(ref), R.NO_BAD, 0)
    text = d.lib.gpd_last_error_string().decode()
    assert str(len(ref)) in text and str(len(ref) - 1) in text
    assert (buf == 0xA5).all()  # nothing written, the prefix included
    rc, nw, nb, bad, why, buf = d.write(prefix=REAL_PREFIX, sizing=True)
    assert (rc, nw, nb) == (0, rn, len(ref)) and (buf == 0xA5).all()
    # a small call on the scratch the large one left, and the large one again
    small, srng = _batch(5, 44)
    s = Dev(small, srng.integers(0, 1 << 62, 5).astype(np.uint64), parser=d.p)
    d.check_write(None, 1, REAL_PREFIX)
    s.check_write(None, 1, PREFIXES[1])
    d.check_write(_masks(3000)["random8"], 1, b"")


# ---- 5. the input's end ---------------------------------------------------------------------------
def test_last_packet_ends_at_data_len_and_descriptors_are_clamped():
    rng = np.random.default_rng(5)
    for tail in (1, 5, 16, 21):
        b, _ = _batch(70, tail, lens=[int(x) for x in rng.integers(0, 40, 69)] + [tail])
        assert int(b.offset[-1]) + int(b.caplen[-1]) == b.data_len
        d = Dev(b, rng.integers(0, 1 << 64, 70, dtype=np.uint64), exact_buffer=True)
        d.check_write(None, 1, PREFIXES[1])
        d.check_write(_masks(70)["last"], 1, b"")
    data_len = 100
    data = rng.integers(1, 256, 112, dtype=np.uint8)
    off = np.array([0, 90, 99, 100, 101, 0xFFFFFFF0, 50], np.uint32)
    cap = np.array([100, 20, 5, 1, 1, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    d = Dev(PacketBatch(data, data_len, off, cap), np.arange(7, dtype=np.uint64), exact_buffer=True)
    ref = d.check_write(None, 1, PREFIXES[2])
    assert len(ref) == 8 + sum(32 + (c + 3) // 4 * 4 for c in (100, 10, 1, 0, 0, 0, 50))


# ---- 6. timestamps --------------------------------------------------------------------------------
def test_timestamps_are_written_raw():
    b, _ = _batch(4, 6, lens=[3, 3, 3, 3])
    ts = np.array([0, (1 << 32) + 5, 1519128000195312500, (1 << 63) | (7 << 32) | 9], np.uint64)
    ref = Dev(b, ts).check_write()
    words = np.frombuffer(ref, "<u4").reshape(4, 9)  # 28 + 3 bytes and 1 of padding + 4
    assert words[:, 3].tolist() == [0, 1, 1519128000195312500 >> 32, (1 << 31) | 7]
    assert words[:, 4].tolist() == [0, 5, 1519128000195312500 & 0xFFFFFFFF, 9]


# ---- 7. the block totals' second round -------------------------------------------------------------
def test_scan_carry_beyond_1024_blocks():
    """1024 * SCAN_BLOCK + 1 packets of 0..7 bytes: the block totals' scan takes a second round,
    its carry forwards (positions) and backwards (the next kept packet).  The checker's loop over
    every packet of this batch takes 2.7 s on the CPU and 0.3 s over one in eight, so the mask
    keeps one in eight."""
    n = 1024 * SCAN_BLOCK + 1
    rng = np.random.default_rng(11)
    ln = rng.integers(0, 8, n).astype(np.uint32)
    off = np.zeros(n, np.int64)
    np.cumsum(ln[:-1], out=off[1:])
    total = int(off[-1] + ln[-1])
    data = rng.integers(0, 256, total + 64, dtype=np.uint8)
    b = PacketBatch(data, total, off.astype(np.uint32), ln)
    keep = (rng.integers(0, 8, n) == 0).astype(np.uint8)
    keep[SCAN_BLOCK * 1020:] = 0  # the next kept packet lies a round away ...
    keep[-1] = 1                  # ... and is the second round's only one
    d = Dev(b, rng.integers(0, 1 << 64, n, dtype=np.uint64))
    d.check_write(keep, 1, PREFIXES[1])


def test_next_kept_record_whole_blocks_away():
    """The three record forms on one batch of 3 * SCAN_BLOCK packets of 5 bytes (a pcap record is
    21 bytes, a pcapng record 40: a run of one record ends inside a chunk).  Only packets 1023 and
    2048 are kept: block 1 is empty, so the header that completes the last chunk of block 0's run
    is found through the block's next-kept index, not through a later wave of the block.  With
    1023 alone there is no next record and that chunk is the stream's ragged end."""
    from test_pcapwrite_gpu import FILE_HEADER, Dev as PcapDev
    n = 3 * SCAN_BLOCK
    b, rng = _batch(n, 12, lens=[5] * n)
    ts = rng.integers(0, 1 << 62, n).astype(np.uint64)
    blocks = (R.section_block(b"amd64", b"linux", b"gopacket") + R.interface_block(1, 0, b"intf0", os_=b"linux") +
              R.interface_block(1, 0, b"intf1"))  # a section and two interfaces: records start at 8 mod 16
    assert len(blocks) == 168 and len(PREFIXES[1]) == 4
    pc, ng = PcapDev(b, ts), Dev(b, ts)
    for kept in ((1023, 2048), (1023,)):
        keep = np.zeros(n, np.uint8)
        keep[list(kept)] = 1
        for flags in (0, FILE_HEADER):
            ref = pc.check_write(keep, flags, (65535, 1))
            assert len(ref) == (24 if flags else 0) + 21 * len(kept)
        pc.check_select(keep)
        for prefix in (blocks, PREFIXES[1]):
            ref = ng.check_write(keep, 1, prefix)
            assert len(ref) == len(prefix) + 40 * len(kept)


# ---- 8. end to end ---------------------------------------------------------------------------------
def test_read_filter_write_read_back():
    """A committed capture with three interfaces of two link types: NewNgReader -> BPF on the
    device -> NgWriter.WritePackets -> NewNgReader.  Interface 1 is given a timestamp offset."""
    torch, P, PW = _mods()
    from dataclasses import replace
    from gopacket_amd import bpf as B
    from gopacket_amd import pcapng as NG
    raw = open(os.path.join(HERE, "golden", "pcapng", "le", "test101.pcapng"), "rb").read()
    opts = NG.NgReaderOptions(WantMixedLinkType=True)
    r = NG.NewNgReader(raw, opts)
    src = r.ReadAll()
    assert src.err is None and r.NInterfaces() == 3 and sorted(set(src.ifindex.tolist())) == [0, 1, 2]
    ifaces = [r.Interface(i) for i in range(3)]
    ifaces[1] = replace(ifaces[1], TimestampOffset=100)
    ts_ns = src.ts_sec.astype(np.uint64) * np.uint64(1000000000) + src.ts_nsec.astype(np.uint64)
    p = _parser()
    db = P.DeviceBatch(src.batch)
    longest = int(src.length.max())
    f = B.NewBPFInstructionFilter([(0x80, 0, 0, 0), (0x35, 1, 0, longest), (0x06, 0, 0, 0xFFFF),
                                   (0x06, 0, 0, 0)], p)  # ld len; jge longest -> ret 0; ret 0xFFFF
    keep = f.match_device(db, length=src.length)
    kept = np.nonzero(src.length < longest)[0]
    assert 0 < len(kept) < src.batch.n and (keep.cpu().numpy() != 0).nonzero()[0].tolist() == kept.tolist()
    buf = io.BytesIO()
    w = PW.NewNgWriterInterface(buf, ifaces[0], PW.NgWriterOptions(r.SectionInfo()))
    assert [w.AddInterface(i) for i in ifaces[1:]] == [1, 2]
    assert w.WritePackets(db, ts_ns, src.length, src.ifindex, keep, parser=p) == len(kept)
    w.Flush()
    back = NG.NewNgReader(buf.getvalue(), opts)
    got = back.ReadAll()
    assert got.err is None and got.batch.n == len(kept) and back.NInterfaces() == 3
    assert back.SectionInfo() == r.SectionInfo()
    for i in range(3):
        assert back.Interface(i) == replace(ifaces[i], TimestampResolution=9)
    assert (got.length == src.length[kept]).all() and (got.ifindex == src.ifindex[kept]).all()
    assert (got.linktype == src.linktype[kept]).all()
    got_ns = got.ts_sec.astype(np.uint64) * np.uint64(1000000000) + got.ts_nsec.astype(np.uint64)
    shift = np.where(src.ifindex[kept] == 1, 100 * 1000000000, 0).astype(np.uint64)
    assert (src.ifindex[kept] == 1).any() and (got_ns == ts_ns[kept] + shift).all()
    for j, i in enumerate(kept):
        assert got.batch.packet(j) == src.batch.packet(int(i))


# ---- 9. the pcap form on the same context ------------------------------------------------------------
def test_pcap_writer_after_ng_writer_on_one_context():
    torch, P, PW = _mods()
    b, rng = _batch(2500, 9)
    ts = rng.integers(0, 1 << 62, 2500).astype(np.uint64)
    keep = _masks(2500)["random8"]
    d = Dev(b, ts)
    d.check_write(keep, 1, REAL_PREFIX)
    stream, nw = PW.write_device(d.p, d.db, ts, None, keep, file_header=(65535, 1))
    want, wn, _ = WR.write(b, ts, None, keep, False, (65535, 1))
    assert nw == wn and stream.cpu().numpy().tobytes() == want
    d.check_write(None, 1, PREFIXES[3])
    stream, nw = PW.write_device_ng(d.p, d.db, ts, keep=keep, prefix=REAL_PREFIX)
    assert stream.cpu().numpy().tobytes() == R.write(b, ts, keep=keep, prefix=REAL_PREFIX)[0]
