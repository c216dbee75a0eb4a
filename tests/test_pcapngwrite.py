"""The pcapng writer (include/gpd_pcapngwrite.h) on the CPU: the ABI, the struct layout, the
host-built blocks against the checker (tests/pcapngwrite_ref.py) byte for byte, the round trip of
pcapgo's own two writer tests (tests/golden/pcapng_write_vectors.json, from
pcapgo/ngwrite_test.go) through the Python NgWriter and this project's NgReader, and the host
error paths, those of the C entry points in a sanitized stand-alone program."""
import ctypes as C
import io
import itertools
import json
import os
import subprocess

import pytest

import pcapngwrite_ref as R
from conftest import ROOT
from gopacket_amd import pcapng as NG
from gopacket_amd.pcap import PcapError

VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "pcapng_write_vectors.json")))


def _pw():
    from gopacket_amd import pcapwrite as PW
    return PW


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    PW = _pw()
    header = open(os.path.join(ROOT, "include", "gpd_pcapngwrite.h")).read()
    assert list(PW.NGW_EXPORTS) == ["gpd_pcapng_section_block", "gpd_pcapng_interface_block",
                                    "gpd_pcapng_stats_block", "gpd_pcapng_write"]
    for name in PW.NGW_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name + "(" in header, name
        assert name not in _lib.EXPORTS
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()
    assert f"#define GPD_PCAPNGW_MAX_PREFIX {PW.GPD_PCAPNGW_MAX_PREFIX}u" in header
    assert PW.NgNoValue64 == 2 ** 64 - 1 == R.NO_VALUE64


def test_reexport_and_defaults():
    import gopacket_amd
    PW = gopacket_amd.pcapwrite
    assert gopacket_amd.NgWriter is PW.NgWriter and gopacket_amd.NewNgWriter is PW.NewNgWriter
    assert gopacket_amd.NewNgWriterInterface is PW.NewNgWriterInterface
    assert PW.DefaultNgWriterOptions.SectionInfo == NG.NgSectionInfo(b"amd64", b"linux", b"gopacket")
    assert PW.DefaultNgInterface == NG.NgInterface(Name=b"intf0", OS=b"linux", SnapLength=0, TimestampResolution=9)
    assert PW.CaptureInfo().InterfaceIndex == 0 and PW.CaptureInfo(1, 2, 3) == PW.CaptureInfo(1, 2, 3, 0)
    s = PW.NgInterfaceStatistics()
    assert (s.LastUpdate, s.StartTime, s.EndTime, s.PacketsReceived, s.PacketsDropped) == \
        (None, None, None, PW.NgNoValue64, PW.NgNoValue64)


def test_struct_layout_matches_c(tmp_path):
    PW = _pw()
    f = [n for n, _ in PW.GpdPcapngStats._fields_]
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_pcapngwrite.h"\nint main(void){'
                    'printf("%zu' + ' %zu' * len(f) + ' %u %u %u %u %llu\\n", sizeof(gpd_pcapng_stats)' +
                    "".join(f", offsetof(gpd_pcapng_stats, {x})" for x in f) +
                    ", GPD_PCAPNGW_MAX_PREFIX, GPD_PCAPNGW_BAD_NONE, GPD_PCAPNGW_BAD_IFACE, GPD_PCAPNGW_BAD_LENGTH,"
                    " (unsigned long long)GPD_PCAPNG_NO_VALUE64); return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == ([C.sizeof(PW.GpdPcapngStats)] + [getattr(PW.GpdPcapngStats, x).offset for x in f] +
                   [PW.GPD_PCAPNGW_MAX_PREFIX, PW.BAD_NONE, PW.BAD_IFACE, PW.BAD_LENGTH, PW.NgNoValue64])
    assert C.sizeof(PW.GpdPcapngStats) == 56
    assert (PW.BAD_NONE, PW.BAD_IFACE, PW.BAD_LENGTH) == (R.BAD_NONE, R.BAD_IFACE, R.BAD_LENGTH)


# ---------------------------------------------------------------- the builders against the checker
STR = [b"", b"a", b"ab", b"abc", b"abcd", b"abcde"]  # lengths 0..5: every padding residue


def test_section_block_matches_checker():
    PW = _pw()
    assert PW.ng_section_block(NG.NgSectionInfo()) == R.section_block()
    assert len(R.section_block()) == 24 + 4  # no option, no end-of-options entry
    for hw, os_, app, com in itertools.product(STR[::2] + [b"\0\xff"], STR[:4], STR[1::2] + [b""], STR[3:] + [b""]):
        got = PW.ng_section_block(NG.NgSectionInfo(hw, os_, app, com))
        assert got == R.section_block(hw, os_, app, com), (hw, os_, app, com)
    for s in STR:  # one option alone, each length
        assert PW.ng_section_block(NG.NgSectionInfo(Comment=s)) == R.section_block(comment=s)
        assert PW.ng_section_block(NG.NgSectionInfo(Hardware=s)) == R.section_block(hardware=s)
    every = R.section_block(b"hw", b"os", b"app", b"note")
    assert every.index(b"app") < every.index(b"note") < every.index(b"hw") < every.index(b"os")
    with pytest.raises(Exception) as e:
        PW.ng_section_block(NG.NgSectionInfo(big_endian=True))
    assert "little-endian" in str(e.value)
    with pytest.raises(Exception):
        PW.ng_section_block(NG.NgSectionInfo(Comment=bytes(65536)))
    assert PW.ng_section_block(NG.NgSectionInfo(Comment=bytes(65535))) == R.section_block(comment=bytes(65535))


def test_interface_block_matches_checker():
    PW = _pw()
    bare = PW.ng_interface_block(NG.NgInterface())
    assert bare == R.interface_block(0, 0) and len(bare) == 32
    assert bare[16:24] == bytes([9, 0, 1, 0, 9, 0, 0, 0])  # if_tsresol: one byte kept in four
    for name, com, desc, filt, os_ in itertools.product(STR[:3], STR[2:5], STR[::5], STR, STR[::3]):
        for off in (0, 100, 2 ** 63 + 5):
            i = NG.NgInterface(name, com, desc, filt, os_, LinkType=228, TimestampResolution=3,
                               TimestampOffset=off, SnapLength=262144)
            want = R.interface_block(228, 262144, name, com, desc, filt, os_, off)
            assert PW.ng_interface_block(i) == want, i
    for res in (0, 3, 6, 9, 0x86):  # whatever the struct says
        assert PW.ng_interface_block(NG.NgInterface(TimestampResolution=res)) == bare
    f = PW.ng_interface_block(NG.NgInterface(Filter=b"none"))
    assert f[16:28] == bytes([11, 0, 5, 0]) + b"\0none" + bytes(3)  # the filter's leading zero byte
    assert b"\x0e\x00\x08\x00" not in bare  # no if_tsoffset when it is zero
    t = PW.ng_interface_block(NG.NgInterface(TimestampOffset=100))
    assert t[16:28] == bytes([14, 0, 8, 0, 100, 0, 0, 0, 0, 0, 0, 0]) and len(t) == 44
    every = R.interface_block(1, 0, b"nm", b"cm", b"ds", b"fl", b"os", 7)
    order = [every.index(x) for x in (b"nm", b"cm", b"ds", b"fl", b"os", b"\x0e\x00\x08\x00", b"\x09\x00\x01\x00")]
    assert order == sorted(order)


def test_stats_block_matches_checker():
    PW = _pw()
    T0, NV = 1519128000195312500, PW.NgNoValue64
    for lu, st, en, rx, dr in itertools.product((None, 0, T0, -5), (None, T0 - 10 ** 11), (None, 0, T0),
                                                (NV, 0, 100, NV - 1), (NV, 0, 1)):
        got = PW.ng_stats_block(1, 2, PW.NgInterfaceStatistics(lu, st, en, rx, dr))
        assert got == R.stats_block(1, 2, lu, st, en, rx, dr), (lu, st, en, rx, dr)
    none = PW.ng_stats_block(0, 1, PW.NgInterfaceStatistics())
    assert none == R.stats_block(0, 1) and len(none) == 24 and none[12:20] == bytes(8)
    full = R.stats_block(0, 1, T0, T0 - 1, T0 + 1, 100, 1)
    assert [full[20 + 12 * k] for k in range(4)] == [2, 3, 5, 4]  # start, end, dropped, received
    assert full[24:32] == (T0 - 1 >> 32).to_bytes(4, "little") + (T0 - 1 & 0xFFFFFFFF).to_bytes(4, "little")
    for intf, n in ((1, 1), (2, 1), (-1, 3), (0, 0)):
        with pytest.raises(PcapError) as e:
            PW.ng_stats_block(intf, n, PW.NgInterfaceStatistics())
        assert str(e.value) == R.IFACE_TEXT % (intf, n)
        with pytest.raises(ValueError) as e2:
            R.stats_block(intf, n)
        assert str(e2.value) == str(e.value)


def test_pcapng_module_helpers_agree_where_options_overlap():
    assert NG.section_block(False, b"hw", b"os", b"app", b"c") == R.section_block(b"hw", b"os", b"app", b"c")
    assert NG.section_block() == R.section_block()
    assert NG.interface_block(1, 96, b"intf0", tsresol=9) == R.interface_block(1, 96, b"intf0")
    assert NG.interface_block(0, 0, b"", tsresol=9) == R.interface_block(0, 0)
    for data, wl in ((b"", None), (b"a", 9), (b"abcd", None), (b"abcde", 5), (bytes(range(67)), 100)):
        ts = 1519128000195312500 + len(data)
        want = R.record(ts, 2, len(data), len(data) if wl is None else wl, data)
        assert NG.enhanced_block(data, 2, ts, wl) == want


# ---------------------------------------------------------------- the reference's two tests, by round trip
def _b(v):
    return v.encode()


def _iface(d):
    return NG.NgInterface(_b(d["Name"]), _b(d["Comment"]), _b(d["Description"]), _b(d["Filter"]), _b(d["OS"]),
                          d["LinkType"], d["TimestampResolution"], d["TimestampOffset"], d["SnapLength"])


def _stats(PW, d):
    return PW.NgInterfaceStatistics(d["LastUpdate"], d["StartTime"], d["EndTime"], d["PacketsReceived"],
                                    d["PacketsDropped"])


def _ci(PW, p):
    return PW.CaptureInfo(p["ts_ns"], p["CaptureLength"], p["Length"], p["InterfaceIndex"])


def _read_back_and_compare(raw, section, expect):
    r = NG.NewNgReader(raw)
    got = r.ReadAll()  # the statistics blocks are skipped on the way
    assert got.err is None and got.stop == NG.STOP_EOF
    s = r.SectionInfo()
    assert (s.Hardware, s.OS, s.Application, s.Comment) == tuple(_b(section[k]) for k in
                                                                 ("Hardware", "OS", "Application", "Comment"))
    assert r.NInterfaces() == len(expect["interfaces"])
    for i, d in enumerate(expect["interfaces"]):
        assert r.Interface(i) == _iface(d), i
    assert got.batch.n == len(expect["packets"])
    for j, p in enumerate(expect["packets"]):
        assert got.batch.packet(j) == bytes.fromhex(p["data"]), j
        assert (int(got.batch.caplen[j]), int(got.length[j]), int(got.ifindex[j])) == \
            (p["CaptureLength"], p["Length"], p["InterfaceIndex"]), j
        assert int(got.ts_sec[j]) * 1000000000 + int(got.ts_nsec[j]) == p["ts_ns"], j


def test_ng_write_simple_round_trip():
    PW = _pw()
    v = VEC["simple"]
    assert VEC["parity"] == "by round trip, bytes unpinned"
    buf = io.BytesIO()
    w = PW.NewNgWriter(buf, v["linktype"])
    p = v["packets"][0]
    w.WritePacket(_ci(PW, p), bytes.fromhex(p["data"]))
    w.Flush()
    _read_back_and_compare(buf.getvalue(), v["section"], v["expect"])
    assert buf.getvalue() == (R.section_block(b"amd64", b"linux", b"gopacket") +
                              R.interface_block(1, 0, b"intf0", os_=b"linux") +
                              R.record(0, 0, p["CaptureLength"], p["Length"], bytes.fromhex(p["data"])))


def test_ng_write_complex_round_trip():
    PW = _pw()
    v = VEC["complex"]
    assert v["order"] == [["packet", 0], ["interface", 1], ["packet", 1], ["stats", 1], ["packet", 2],
                          ["packet", 3], ["packet", 4], ["stats", 0]]
    buf = io.BytesIO()
    s = v["section"]
    options = PW.NgWriterOptions(NG.NgSectionInfo(_b(s["Hardware"]), _b(s["OS"]), _b(s["Application"]), _b(s["Comment"])))
    w = PW.NewNgWriterInterface(buf, _iface(v["interfaces"][0]), options)
    want = [R.section_block(comment=b"A test"),
            R.interface_block(1, 0, b"in0", b"test0", b"some test interface")]
    for what, k in v["order"]:
        if what == "packet":
            p = v["packets"][k]
            w.WritePacket(_ci(PW, p), bytes.fromhex(p["data"]))
            want.append(R.record(p["ts_ns"], p["InterfaceIndex"], p["CaptureLength"], p["Length"],
                                 bytes.fromhex(p["data"])))
        elif what == "interface":
            assert w.AddInterface(_iface(v["interfaces"][k])) == k
            want.append(R.interface_block(1, 0, b"null0", b"", b"some test interface", b"none", b"not needed", 100))
        else:
            st = v["interfaces"][k]["Statistics"]
            w.WriteInterfaceStats(k, _stats(PW, st))
            want.append(R.stats_block(k, 2, st["LastUpdate"], st["StartTime"], st["EndTime"],
                                      st["PacketsReceived"], st["PacketsDropped"]))
    w.Flush()
    assert v["expect"]["packets"][1]["ts_ns"] == v["packets"][1]["ts_ns"] + 100 * 10 ** 9  # the offset is not subtracted
    assert all(i["TimestampResolution"] == 9 for i in v["expect"]["interfaces"])
    _read_back_and_compare(buf.getvalue(), s, v["expect"])
    assert buf.getvalue() == b"".join(want)


# ---------------------------------------------------------------- host errors
def test_write_packet_host_errors():
    PW = _pw()
    buf = io.BytesIO()
    w = PW.NewNgWriter(buf, 1)
    n0 = len(buf.getvalue())
    for ifx in (1, 5, -1):
        with pytest.raises(PcapError) as e:
            w.WritePacket(PW.CaptureInfo(0, 4, 4, ifx), b"abcd")
        assert str(e.value) == f"Can't send statistics for non existent interface {ifx}; have only 1 interfaces"
    with pytest.raises(PcapError) as e:
        w.WritePacket(PW.CaptureInfo(0, 5, 5, 0), b"abcd")
    assert str(e.value) == "capture length 5 does not match data length 4"
    with pytest.raises(PcapError) as e:
        w.WritePacket(PW.CaptureInfo(0, 4, 3, 0), b"abcd")
    assert str(e.value).startswith("invalid capture info ") and str(e.value).endswith(":  capture length > length")
    with pytest.raises(PcapError) as e:  # the interface check comes first
        w.WritePacket(PW.CaptureInfo(0, 5, 3, 1), b"abcd")
    assert "non existent interface 1" in str(e.value)
    with pytest.raises(PcapError) as e:
        w.WriteInterfaceStats(1, PW.NgInterfaceStatistics())
    assert str(e.value) == R.IFACE_TEXT % (1, 1)
    assert len(buf.getvalue()) == n0  # a refused call writes nothing
    assert w.AddInterface(NG.NgInterface(Name=b"two")) == 1
    w.WritePacket(PW.CaptureInfo(7, 4, 4, 1), b"abcd")
    w.WriteInterfaceStats(1, PW.NgInterfaceStatistics())
    assert buf.getvalue()[n0:] == (R.interface_block(0, 0, b"two") + R.record(7, 1, 4, 4, b"abcd") +
                                   R.stats_block(1, 2))


def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/pcapngwrite_errpath.cpp: a stand-alone program (its own main, the runtime stubbed)
    linked with gpd_pcapngwrite.hip, host code built with AddressSanitizer and UBSan, run on the
    CPU: the builders with exact-size and one-short buffers and as sizing calls, and every path of
    gpd_pcapng_write that returns before a device is needed."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "pcapngwrite_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "pcapngwrite_errpath.cpp"),
                    os.path.join(CSRC, "gpd_pcapngwrite.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
