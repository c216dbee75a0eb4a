"""The pcap writer without a GPU: the host-only entry point, the Python Writer's single-packet
path and the checker (tests/pcapwrite_ref.py) against pcapgo/write_test.go's byte literals
(tests/golden/pcapgo_write_vectors.json) and the golden captures."""
import ctypes as C
import io
import json
import os
import re
import subprocess

import pytest

import pcapwrite_ref as WR
from gopacket_amd import pcap

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VEC = json.load(open(os.path.join(HERE, "golden", "pcapgo_write_vectors.json")))
CAPTURES = ["test_dns.pcap", "test_ethernet.pcap", "test_loopback.pcap"]


def test_file_header_equals_reference_vectors():
    from gopacket_amd import pcapwrite as PW
    for h in VEC["headers"]:
        want = bytes.fromhex(h["hex"])
        assert PW.file_header(h["snaplen"], h["linktype"], h["nanos"]) == want, h["name"]
        assert WR.file_header(h["snaplen"], h["linktype"], h["nanos"]) == want, h["name"]
        buf = io.BytesIO()
        w = PW.NewWriterNanos(buf) if h["nanos"] else PW.NewWriter(buf)
        w.WriteFileHeader(h["snaplen"], h["linktype"])
        assert buf.getvalue() == want, h["name"]


def test_file_header_refuses_unknown_flags_and_null():
    from gopacket_amd import pcapwrite as PW
    lib = PW.pw_lib()
    buf = (C.c_uint8 * 24)()
    assert lib.gpd_pcap_file_header(4, 0, 1, buf) == -1
    assert lib.gpd_pcap_file_header(0, 0, 1, None) == -1
    # GPD_PCAPW_FILE_HEADER is accepted (the flags word of gpd_pcap_write) and changes nothing
    assert lib.gpd_pcap_file_header(2, 7, 1, buf) == 0
    assert bytes(buf) == WR.file_header(7, 1, False)


def test_checker_and_writer_reproduce_record_vector():
    from gopacket_amd import pcapwrite as PW
    p = VEC["packet"]
    data, want = bytes.fromhex(p["data"]), bytes.fromhex(p["hex"])
    assert WR.record(p["ts_ns"], p["caplen"], p["length"], data) == want
    buf = io.BytesIO()
    PW.NewWriter(buf).WritePacket(PW.CaptureInfo(p["ts_ns"], p["caplen"], p["length"]), data)
    assert buf.getvalue() == want
    nano = want[:4] + (0xAA * 1000).to_bytes(4, "little") + want[8:]
    assert WR.record(p["ts_ns"], p["caplen"], p["length"], data, nanos=True) == nano
    buf = io.BytesIO()
    PW.NewWriterNanos(buf).WritePacket(PW.CaptureInfo(p["ts_ns"], p["caplen"], p["length"]), data)
    assert buf.getvalue() == nano


def test_write_packet_rejects_capture_info_errors():
    from gopacket_amd import pcapwrite as PW
    r = VEC["rejected"]
    data = bytes.fromhex(r["data"])
    for info in r["infos"]:
        buf = io.BytesIO()
        with pytest.raises(pcap.PcapError) as e:
            PW.NewWriter(buf).WritePacket(PW.CaptureInfo(r["ts_ns"], info["caplen"], info["length"]), data)
        assert buf.getvalue() == b""
        if info["error"] is not None:
            assert str(e.value) == info["error"]
        else:
            assert str(e.value).endswith(":  capture length > length")


def test_write_packet_zero_timestamp_is_now():
    import time
    from gopacket_amd import pcapwrite as PW
    buf = io.BytesIO()
    t0 = int(time.time())
    PW.NewWriter(buf).WritePacket(PW.CaptureInfo(None, 2, 2), b"ab")
    sec = int.from_bytes(buf.getvalue()[:4], "little")
    assert t0 <= sec <= t0 + 5 and buf.getvalue()[16:] == b"ab"


@pytest.mark.parametrize("name", CAPTURES)
def test_checker_roundtrips_golden_capture(name):
    raw = open(os.path.join(HERE, "golden", name), "rb").read()
    p = pcap.index(pcap.capture_array(raw))
    assert p.err is None and not p.nano
    out, n, bad = WR.write(p.batch, p.ts_ns, p.length, None, False, (p.snaplen, p.linktype))
    assert (n, bad) == (p.batch.n, WR.NO_BAD)
    assert out == raw


def test_checker_stops_at_first_bad_kept_packet():
    import numpy as np
    from gopacket_amd.batch import PacketBatch
    b = PacketBatch.from_packets([b"abcd", b"efghij", b"kl", b"mnop"])
    ts = np.arange(4, dtype=np.uint64) * 1000
    length = np.array([4, 5, 2, 3], np.uint32)  # packets 1 and 3 have caplen > length
    out, n, bad = WR.write(b, ts, length)
    assert (n, bad) == (1, 1) and out == WR.record(0, 4, 4, b"abcd")
    out, n, bad = WR.write(b, ts, length, keep=np.array([1, 0, 0x80, 0], np.uint8))
    assert (n, bad) == (2, WR.NO_BAD) and out == WR.record(0, 4, 4, b"abcd") + WR.record(2000, 2, 2, b"kl")
    data, off, cap, idx = WR.select(b, np.array([0, 1, 1, 0], np.uint8))
    assert data == b"efghij" + bytes(10) + b"kl" + bytes(14)
    assert off.tolist() == [0, 16] and cap.tolist() == [6, 2] and idx.tolist() == [1, 2]


def test_new_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    from gopacket_amd import pcapwrite as PW
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpd_pcapwrite.h")).read()
    for name in PW.PW_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name + "(" in header, name
        assert name not in _lib.EXPORTS
    assert _lib.lib.gpd_abi_version() == 10


def test_lazy_reexport():
    import gopacket_amd
    assert gopacket_amd.pcapwrite.NewWriter is not None


def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/pcapwrite_errpath.cpp: a stand-alone program (its own main, the runtime stubbed)
    linked with gpd_pcapwrite.hip alone, host code built with AddressSanitizer and UBSan, run on
    the CPU: gpd_pcap_file_header, and every path of gpd_pcap_write and gpd_batch_select that
    returns before a device is needed, error texts compared whole."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "pcapwrite_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "pcapwrite_errpath.cpp"),
                    os.path.join(CSRC, "gpd_pcapwrite.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


# ---------------------------------------------------------------- one scan, one chunk loop
WRITERS = ("gpd_pcapwrite.hip", "gpd_pcapngwrite.hip")


def _csrc_texts():
    csrc = os.path.join(ROOT, "gopacket_amd", "csrc")
    return {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))
            if f.endswith((".h", ".hip", ".cpp"))}


def test_wave_and_byte_helpers_have_one_copy():
    """The byte shuffles, the 64-bit wave helpers and check_in are each defined once in
    gopacket_amd/csrc: the helpers in gpd_stream_util.h, check_in in gpd_write_scan.h."""
    texts = _csrc_texts()
    where = {"bytes_from": "gpd_stream_util.h", "byte_mask": "gpd_stream_util.h", "low_bytes": "gpd_stream_util.h",
             "wave_scan64": "gpd_stream_util.h", "shfl64": "gpd_stream_util.h", "shfl_up64": "gpd_stream_util.h",
             "wave_min32": "gpd_stream_util.h", "src16_of": "gpd_stream_util.h"}
    for name, home in where.items():
        pat = r"^[ \t]*(?:static\s+)?__device__[^;{()]*\b%s\s*\([^;{]*\)\s*\{" % name
        assert {f: len(re.findall(pat, t, re.M)) for f, t in texts.items() if re.search(pat, t, re.M)} == {home: 1}, name
    pat = r"\bint check_in\s*\("
    assert {f: len(re.findall(pat, t)) for f, t in texts.items() if re.search(pat, t)} == {"gpd_write_scan.h": 1}
    for f in WRITERS:
        assert not re.search(r"\bsrc16\s*\(|\bshfl64\s*\([^)]*\)\s*\{", texts[f]), f


def test_scan_and_chunk_loop_have_one_copy():
    """The full form: bad, sum, scan and copy kernels live in gpd_write_scan.h alone, one
    __global__ copy kernel for the three record forms; the writers include the header, define
    their forms and neither kept() nor a kernel of those kinds of their own."""
    texts = _csrc_texts()
    kernels = lambda t: re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", t)
    assert sorted(kernels(texts["gpd_write_scan.h"])) == ["bad_kernel", "copy_kernel", "scan_kernel", "sum_kernel"]
    assert kernels(texts["gpd_pcapwrite.hip"]) == ["pw_head_kernel"] and kernels(texts["gpd_pcapngwrite.hip"]) == []
    copies = {f: [k for k in kernels(t) if "copy" in k] for f, t in texts.items()}
    assert {f: c for f, c in copies.items() if c} == {"gpd_write_scan.h": ["copy_kernel"]}
    for f in WRITERS:
        t = texts[f]
        assert '#include "gpd_write_scan.h"' in t, f
        assert not re.search(r"\bbool\s+kept\s*\(|struct\s+(WrArgs|NgwArgs|Rec)\b|__builtin_nontemporal_store", t), f
        assert not re.search(r"GPD_PW_(COPY_WAVES|NT_LOADS|PLAIN_STORES)", t), f
        assert not re.search(r"\bk(ScanBlock|ScanWaves|CopyWaves|None)\s*=", t), f
    assert re.findall(r"struct\s+(\w+Form)\b", texts["gpd_pcapwrite.hip"]) == ["PcapForm", "BatchForm"]
    assert re.findall(r"struct\s+(\w+Form)\b", texts["gpd_pcapngwrite.hip"]) == ["NgForm"]
    for form in ("PcapForm", "BatchForm"):
        assert f"copy_kernel<{form}>" in texts["gpd_pcapwrite.hip"] and f"sum_kernel<{form}>" in texts["gpd_pcapwrite.hip"]
    assert "copy_kernel<NgForm>" in texts["gpd_pcapngwrite.hip"] and "sum_kernel<NgForm>" in texts["gpd_pcapngwrite.hip"]
    assert "kCopyWaves = 4;" in texts["gpd_write_scan.h"]
    assert "GPD_PW_" not in texts["gpd_write_scan.h"]
    from gopacket_amd.build import HEADERS
    assert "gpd_write_scan.h" in {os.path.basename(h) for h in HEADERS}
    from gopacket_amd import _lib
    assert _lib.lib.gpd_abi_version() == 10
