"""Checksum arithmetic at its extremes, on the device: every family of tests/csum_cases.py
through the generic decoder and through every fast kernel and tuning, against the oracle (all
result words) and against the checker's checksum words (tests/test_csum_extremes.py pins the
checker on the CPU), with the fast / generic split of each fast-path launch asserted as an
equality with the count the design gives (csum_cases.designed_fallback) — a family that went to
the generic decoder whole would test nothing new.  Then the same expectations through the host
path, a pcap-record layout and the defragmented route."""
import ctypes as C

import numpy as np
import pytest

import csum_cases as CC
import oracle_ref as O
from gopacket_amd import layers as L
from gopacket_amd.batch import PacketBatch
from test_parity_gpu import ALL, _parser, assert_same, run_both

pytestmark = pytest.mark.gpu

TUNINGS = CC.TUNINGS


def assert_checker(res, name, what=""):
    """The result's checksum words and their status bits against the checker's."""
    _, cs, bits = CC.reference(name)
    assert np.array_equal(res.status & (3 << 18), bits), (name, what, "which checksums exist")
    bad = np.nonzero(res.csum != cs)[0]
    if len(bad):
        i = int(bad[0])
        b = CC.family(name).batch
        raise AssertionError(f"{name} {what}: csum differs from the checker at {len(bad)} packets; first i={i}: "
                             f"dev={int(res.csum[i]):#x} want={int(cs[i]):#x} offset={int(b.offset[i])} "
                             f"caplen={int(b.caplen[i])} pkt={b.packet(i)[:96].hex()}")


def fast_run(batch, tuning, records):
    """One timed fast-path launch: (the result on the host, the packets it left to the generic
    decoder — gpd_last_launch_split)."""
    import torch
    from gopacket_amd import parser as P
    from gopacket_amd._lib import check, lib
    p = _parser()
    p.Tuning = tuning
    db = P.DeviceBatch(batch, 0)
    dr = P.DeviceResult(batch.n, 0, detail=True, records=records)
    h = p.ctx().h
    check(lib.gpd_ctx_set_timing(h, 1), "timing")
    p.decode_device(db, dr)
    torch.cuda.synchronize()
    fb, f, l_ = C.c_uint64(), C.c_float(), C.c_float()
    check(lib.gpd_last_launch_split(h, C.byref(fb), C.byref(f), C.byref(l_)), "split")
    return dr.to_host(), int(fb.value)


@pytest.mark.parametrize("name", CC.NAMES)
def test_generic_decoder(name):
    """ext records force decode_kernel for every packet (be16_sum over LDS windows, and over
    global memory for the frames larger than a window); run_both then repeats the batch on the
    automatic fast path in both result forms."""
    dev = run_both(CC.family(name).batch, ext=True)
    assert_checker(dev, name, "ext")


@pytest.mark.parametrize("tname,tuning", TUNINGS, ids=[t for t, _ in TUNINGS])
@pytest.mark.parametrize("name", CC.NAMES)
def test_fast_kernels(name, tname, tuning):
    """Each family under each tuning, SoA and gpd_record forms: every result word equals the
    oracle's, the checksum words the checker's, and the launch left exactly the designed number of
    packets to the generic decoder — 0 for the short-frame families under the 4 KiB register
    loop and for the long-frame families under the rounds; the frames past the window under the
    windowed kernels and the split kernel; the whole family for the jumbograms, and for VXLAN
    under the rounds; under the windowed header-once kernel the VXLAN frames of the windows that
    hold 16 or fewer."""
    fam = CC.family(name)
    ref, _, _ = CC.reference(name)
    for records in (False, True):
        res, fb = fast_run(fam.batch, tuning, records)
        what = f"{tname} records={records} kernel={CC.kernel_of(fam.batch, tuning, records)}"
        assert_same(res, ref, fam.batch, ext=False)
        assert_checker(res, name, what)
        want = CC.designed_fallback(fam, tuning, records)
        print(f"{name} {what}: fallback {fb} of {fam.batch.n}, designed {want}")
        assert fb == want, (name, what, fb, want)


@pytest.mark.parametrize("name", CC.NAMES)
def test_host_path(name):
    """gpd_decode_host stages the same bytes at other base addresses (span and repack)."""
    fam = CC.family(name)
    ref, _, _ = CC.reference(name)
    host = _parser().DecodeBatchHost(fam.batch, detail=True)
    assert_same(host, ref, fam.batch, ext=False)
    assert_checker(host, name, "host path")


@pytest.mark.parametrize("name", ["fills_short", "edge_masks", "folds", "fills_long"])
def test_pcap_record_layout(name):
    """The same frames as pcap records (16-byte record headers between them: offsets 8 mod 16
    and every other residue): the checker's words do not change, the kernels must not either."""
    from gopacket_amd import pcap as NP
    fam = CC.family(name)
    _, cs, bits = CC.reference(name)
    b = NP.index(NP.synth_capture(fam.batch)).batch
    assert b.n == fam.batch.n and np.array_equal(b.caplen, fam.batch.caplen)
    ref = O.decode(b, L.LayerTypeEthernet, ALL, 0, ext=True, nthreads=8)
    cs2, bits2 = CC.expected(b, ref)
    assert np.array_equal(cs2, cs) and np.array_equal(bits2, bits)
    for _, t in TUNINGS[:1] + TUNINGS[2:3] + TUNINGS[5:6] + TUNINGS[8:]:
        for records in (False, True):
            res, _ = fast_run(b, t, records)
            assert_same(res, ref, b, ext=False)
            assert np.array_equal(res.csum, cs), (name, t, records)


def test_defragmented_route():
    """The IPv4 frames of the long fills, cut into three or four fragments each, rebuilt by
    DefragBatch and decoded from the datagram batch (first layer IPv4): the checker's words over
    the rebuilt datagrams, which differ from the frames sent only in Id, flags and header
    checksum."""
    import torch
    from gopacket_amd import ip4reasm as I
    from gopacket_amd import parser as P
    from test_ip4reasm_gpu import Pair, _fragment
    fam = CC.family("fills_long")
    frames = [fam.batch.packet(i) for i in range(fam.batch.n)]
    frames = [f for f in frames if f[12:14] == b"\x08\x00"]
    assert len(frames) >= 60
    sent = []
    for k, f in enumerate(frames):
        sent += _fragment(f, 1 + k, [8 * (20 + k % 50), 8 * (3 + k % 7), 8 * (60 + k % 11)])
    parser = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    parser._mask = ALL
    pair = Pair(parser)
    try:
        batch, db, out, cnt, recs = pair.handoff(sent, align=1)
        assert cnt == len(sent)
        res = pair.dev.DefragBatch(db, out, cnt)
        h = I.defrag_to_host(res)
        assert res.ndgrams == len(frames)
        hb = PacketBatch.from_arrays(h.bytes, h.offset, h.caplen, data_len=len(h.bytes))
        ref = O.decode(hb, L.LayerTypeIPv4, ALL, 0, ext=True)
        cs, bits = CC.expected(hb, ref)
        assert (bits >> 19).all() and (bits >> 18 & 1).all()
        # the transport checksum is the sent frame's: the pseudo-header and the segment are unchanged
        _, cs0, _ = CC.reference("fills_long")
        v4 = [i for i in range(fam.batch.n) if fam.batch.packet(i)[12:14] == b"\x08\x00"]
        by_id = {int(g["id"]): k for k, g in enumerate(h.dgrams)}
        for k, i in enumerate(v4):
            assert int(cs[by_id[1 + k]]) >> 16 == int(cs0[i]) >> 16
        p4 = P.NewDecodingLayerParser(L.LayerTypeIPv4)
        p4._mask = ALL
        for records in (False, True):
            dr = P.DeviceResult(res.batch.n, 0, records=records)
            p4.decode_device(res.batch, dr)
            torch.cuda.synchronize()
            got = dr.to_host()
            assert_same(got, ref, hb, ext=False)
            assert np.array_equal(got.csum, cs) and np.array_equal(got.status & (3 << 18), bits)
    finally:
        pair.close()
