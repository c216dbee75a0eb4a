"""The checksum families of tests/csum_cases.py pinned without a GPU: the checker against the
oracle on every frame of every family, and against the reference's known answers in
tests/golden/golden.json — so a wrong checker cannot agree with a wrong kernel through the
oracle alone.  Building a family also runs its own assertions (pair coverage, wrap points, fold
targets, the jumbogram sum above 2^32)."""
import numpy as np
import pytest

import csum_cases as CC
import errpath_cases as EC
import golden_cases as G
import oracle_ref as O
from gopacket_amd.batch import PacketBatch

META = G.load()
CASES = {c["name"]: c for c in META["cases"]}


@pytest.mark.parametrize("name", CC.NAMES)
def test_checker_equals_oracle(name):
    """Every frame: the checker's IPv4 and transport checksums, and which of them exist, equal
    the oracle's csum word and status bits 18-19."""
    fam = CC.family(name)
    ref, cs, bits = CC.reference(name)
    assert fam.batch.n >= 12
    assert np.array_equal(bits, ref.status & (3 << 18)), "which checksums exist"
    bad = np.nonzero(cs != ref.csum)[0]
    assert len(bad) == 0, (name, int(bad[0]), hex(int(cs[bad[0]])), hex(int(ref.csum[bad[0]])))
    assert (bits >> 19).any(), "the family carries transport checksums"


@pytest.mark.parametrize("name", CC.NAMES)
def test_family_is_what_the_design_table_assumes(name):
    """The frames a family marks as outside the straight-line envelope are the ones the oracle
    decodes with an error, with IPv4 options or with a hop-by-hop header; the VXLAN marks are
    the frames whose decoded list holds VXLAN; everything else is a clean TCP / UDP stack."""
    from gopacket_amd import layers as L
    fam = CC.family(name)
    ref, _, _ = CC.reference(name)
    for i in range(fam.batch.n):
        d = ref.decoded(i)
        assert (L.LayerTypeVXLAN in d) == bool(fam.vxlan[i]), (name, i)
        r4 = ref.layer(i, "IPv4")
        opts = r4 is not None and r4[0][1] - r4[0][0] != 20
        hbh = fam.batch.packet(i)[12:14] == b"\x86\xdd" and fam.batch.packet(i)[20] == 0
        err = (int(ref.status[i]) & 3) == 2
        assert (err or opts or hbh) == bool(fam.outside[i]), (name, i, d, str(ref.err(i)))


def test_checker_equals_the_reference_kats():
    """ip4_test.go's header checksums, decode_test.go's 0x555A / 0x9A8F, tcpip_test.go's 0xBC5F
    and 0x4D21 and its jumbogram value, from the checker alone."""
    for name in ("ip4_checksum_kat_0", "ip4_checksum_kat_1"):
        c = CASES[name]
        assert EC.ip4_checksum(bytes.fromhex(c["hex"])) == c["expect"]["ip4_csum"]
    c = CASES["simple_tcp_dlp4"]
    pkt = bytearray(G.case_bytes(c))
    assert c["expect"]["ip4_csum"] == 0x555A and EC.ip4_checksum(bytes(pkt[14:34])) == 0x555A
    total = int.from_bytes(pkt[16:18], "big")
    assert EC.l4_checksum(bytes(pkt), 34, 14 + total, "IPv4", 14, 6) == c["expect"]["l4_csum"] == 0
    pkt[34 + 16:34 + 18] = b"\0\0"
    assert EC.l4_checksum(bytes(pkt), 34, 14 + total, "IPv4", 14, 6) == c["expect"]["l4_csum_zeroed"] == 0x9A8F
    for name, kind, l4, want in (("udp4_checksum_kat", "IPv4", 20, 0xBC5F), ("udp6_dstopts_checksum_kat", "IPv6", 48, 0x4D21)):
        c = CASES[name]
        pkt = bytearray(G.case_bytes(c))
        assert c["expect"]["l4_csum_zeroed"] == want
        assert EC.l4_checksum(bytes(pkt), l4, len(pkt), kind, 0, 17) == 0
        pkt[l4 + 6:l4 + 8] = b"\0\0"
        assert EC.l4_checksum(bytes(pkt), l4, len(pkt), kind, 0, 17) == want
    k = META["udp6_jumbogram_checksum_kat"]
    seg = bytes.fromhex(k["udp_header"]) + bytes([k["payload_byte"]]) * k["payload_len"]
    pkt = bytes(8) + bytes.fromhex(k["src"]) + bytes.fromhex(k["dst"]) + seg
    assert len(seg) >> 16, "the length >> 16 term is not zero"
    assert EC.l4_checksum(pkt, 40, len(pkt), "IPv6", 0, 17) == k["want"]


def test_go_wrap_is_the_only_difference_between_the_sums():
    """The jumbograms past 2^32: the checker's value needs the wrap (folding the unreduced sum
    gives another checksum), and the oracle agrees with the wrapped one."""
    fam = CC.family("jumbograms")
    ref, cs, _ = CC.reference("jumbograms")
    past = 0
    for i in range(fam.batch.n):
        pkt = fam.batch.packet(i)
        if pkt[54] != 6:  # (UDP: the reference stops at its decoder, csum_cases.jumbo_frame)
            assert not (int(ref.status[i]) >> 19) & 1 and (int(ref.status[i]) & 3) == 2
            continue
        s = EC.l4_sum(pkt, 54, len(pkt), "IPv6", 14, 6)
        if s >> 32:
            past += 1
            t = s
            while t > 0xFFFF:
                t = (t >> 16) + (t & 0xFFFF)
            assert (~t & 0xFFFF) != int(cs[i]) >> 16, "an end-around fold of the whole sum differs"
        assert CC.fold(s) ^ 0xFFFF == int(cs[i]) >> 16 == int(ref.csum[i]) >> 16
    assert past >= 2


def test_designed_counts_of_the_named_pairs():
    """The counts DESIGN.md §6 states outright, from the model alone (so a drift of the model
    shows here and not as a changed expectation above)."""
    for name in CC.SHORT:
        fam = CC.family(name)
        for t in (dict(window_bytes=4096, split=0), dict(window_bytes=4096, split=0, shift=1)):
            assert CC.kernel_of(fam.batch, t, False) == ("rs", 4096)
            assert CC.designed_fallback(fam, t, False) == int(fam.outside.sum())
            assert (CC.designed_fallback(fam, t, False) == 0) == (name != "ip4_headers")
    for name in CC.LONG:
        fam = CC.family(name)
        for w in (2, 3):
            t = dict(header_once=2, waves_per_simd=w)
            assert CC.kernel_of(fam.batch, t, True) == ("ro", 8192)
            assert CC.designed_fallback(fam, t, True) == 0
    for _, t in CC.TUNINGS:
        for rec in (False, True):
            assert CC.designed_fallback(CC.family("jumbograms"), t, rec) == CC.family("jumbograms").batch.n
    vx = CC.family("vxlan_inner")
    assert CC.designed_fallback(vx, dict(header_once=2), False) == vx.batch.n
    # (the windows that end a tile hold few frames: their VXLAN lanes are listed)
    assert 0 < CC.designed_fallback(vx, dict(window_bytes=8192, header_once=1), False) < vx.batch.n // 16
    assert CC.designed_fallback(vx, dict(window_bytes=8192, header_once=0), False) == 0


def test_split_kernel_window_model():
    """designed_fallback's model of the split kernel's one window per tile, on a layout small
    enough to state by hand: 64 frames of 100 bytes at 16-aligned slots of 112 — the window
    holds the frames that end by byte 4096, the first 36."""
    import error_sites as ES
    f = ES.eth(0x0800, ES.ip4(ES.udp(bytes(58)), proto=17))
    assert len(f) == 100
    fam = CC.Family("model", PacketBatch.from_packets([f] * 64))
    assert CC.kernel_of(fam.batch, dict(window_bytes=4096, split=1), True) == ("sp", 4096)
    assert CC.designed_fallback(fam, dict(window_bytes=4096, split=1), True) == 64 - 36
    assert CC.designed_fallback(fam, dict(window_bytes=4096, split=1), False) == 0
    assert CC.kernel_of(fam.batch, None, False) == ("rs", 8192)
    assert CC.kernel_of(CC.family("fills_long").batch, None, True) == ("ro", 8192)
    assert O is not None
