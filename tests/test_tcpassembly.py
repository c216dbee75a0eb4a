"""The tcpassembly hand-off (include/gpd_tcpassembly.h) on the CPU: the ABI, the record
layouts, the restated assembler (tests/tcpassembly_ref.py) against tcpassembly's own test
vectors (tests/golden/tcpassembly_vectors.json, from tcpassembly/assembly_test.go), and the
segment oracle (tests/tcpseg_ref.py) on hand-built packets with the expected fields written out."""
import os
import subprocess

import numpy as np

import oracle_ref as O
import tcpassembly_ref as TA
import tcpseg_ref as TS
from conftest import ROOT
from gopacket_amd import layers as L
from gopacket_amd.batch import PacketBatch

from tcpseg_cases import A4, A6, ACK, ALL, B4, B6, PSH, VEC, hand_built, vec_bytes, vec_want  # noqa: F401


# ---------------------------------------------------------------- the ABI
def test_symbol_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    from gopacket_amd import tcpassembly as T
    header = open(os.path.join(ROOT, "include", "gpd_tcpassembly.h")).read()
    assert list(T.TCPSEG_EXPORTS) == ["gpd_tcp_segments"]
    for name in T.TCPSEG_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name + "(" in header, name
        assert name not in _lib.EXPORTS
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()


def test_lazy_reexport():
    import gopacket_amd
    assert gopacket_amd.tcpassembly.TCPSegments is not None
    assert gopacket_amd.tcpassembly.SORT_TILE > 64


def test_struct_layouts_match_c(tmp_path):
    from gopacket_amd.tcpassembly import GROUP_DTYPE, SEG_DTYPE, TCP_UNGROUPED
    assert SEG_DTYPE == TS.SEG_DTYPE and GROUP_DTYPE == TS.GROUP_DTYPE and TCP_UNGROUPED == TS.UNGROUPED
    sf = ["packet", "flow_id", "seq", "ack", "payload_off", "payload_len", "tcp_off", "flags", "lookup_only",
          "reserved"]
    gf = ["flow_id", "start", "count", "first_packet"]
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_tcpassembly.h"\nint main(void){'
                    'printf("%zu' + ' %zu' * (len(sf) + 1 + len(gf)) + ' %u\\n", sizeof(gpd_tcp_seg)' +
                    "".join(f", offsetof(gpd_tcp_seg, {f})" for f in sf) + ", sizeof(gpd_tcp_group)" +
                    "".join(f", offsetof(gpd_tcp_group, {f})" for f in gf) + ', GPD_TCP_UNGROUPED); return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == ([SEG_DTYPE.itemsize] + [SEG_DTYPE.fields[f][1] for f in sf] + [GROUP_DTYPE.itemsize] +
                   [GROUP_DTYPE.fields[f][1] for f in gf] + [TCP_UNGROUPED])
    assert SEG_DTYPE.itemsize == 32 and GROUP_DTYPE.itemsize == 16


def test_segments_to_host_raises_on_a_short_buffer():
    import pytest
    import torch
    from gopacket_amd import tcpassembly as T
    buf = torch.zeros(3 * 32, dtype=torch.uint8)
    assert len(T.segments_to_host(buf, 3)) == 3
    with pytest.raises(ValueError):
        T.segments_to_host(buf, 4)


# ---------------------------------------------------------------- the restated assembler
def test_sequence_overflow():
    so = VEC["sequence_overflow"]
    assert TA.difference(so["s"], so["t"]) == so["difference"]  # TestSequenceOverflow
    assert TA.add(0xFFFFFFFF, 11) == 10


def test_assembler_reproduces_every_reference_vector():
    """assembly_test.go's `test` helper: one pool, one assembler with
    MaxBufferedPagesPerConnection = 4 (:57), every Assemble call's Reassembled list compared."""
    assert VEC["max_buffered_pages_per_connection"] == 4 and VEC["page_bytes"] == TA.PAGE_BYTES
    assert set(VEC["tests"]) == {"TestReorder", "TestMaxPerSkip", "TestReorderFast", "TestOverlap",
                                 "TestBufferedOverlap", "TestOverrun1", "TestOverrun2", "TestCacheLargePacket"}
    for name, steps in VEC["tests"].items():
        fac = TA.RecordingFactory()
        a = TA.NewAssembler(fac, VEC["max_buffered_pages_per_connection"])
        for k, s in enumerate(steps):
            before = len(fac.calls.get("k", []))
            rec = np.zeros((), TS.SEG_DTYPE)
            pay = vec_bytes(s["payload"])
            rec["seq"], rec["flags"], rec["payload_len"] = s["seq"], TA.SYN if s["syn"] else 0, len(pay)
            a.AssembleSegment("k", rec, pay)
            calls = fac.calls.get("k", [])[before:]
            got = calls[0] if calls else []
            assert len(calls) <= 1 and got == vec_want(s), (name, k, got)


def test_assembler_ignores_and_closes():
    """:535 (nothing to act on), :550-556 (an empty non-SYN packet creates no connection) and
    :630-632 (FIN / RST ends the stream)."""
    fac = TA.RecordingFactory()
    a = TA.NewAssembler(fac)
    a.AssembleWithTimestamp("k", 5, ACK, b"")
    a.AssembleWithTimestamp("k", 5, TA.FIN | ACK, b"")
    assert fac.calls == {} and a.connPool.conns == {}
    a.AssembleWithTimestamp("k", 5, TA.SYN, b"")
    a.AssembleWithTimestamp("k", 6, ACK, b"ab")
    a.AssembleWithTimestamp("k", 8, TA.FIN | ACK, b"")
    assert fac.calls["k"] == [[(b"", 0, True, False)], [(b"ab", 0, False, False)], [(b"", 0, False, True)]]
    assert fac.completed == {"k": 1} and a.connPool.conns == {} and a.used == 0


# ---------------------------------------------------------------- the segment oracle, by hand
def test_segment_oracle_on_hand_built_packets():
    cases = hand_built()
    batch = PacketBatch.from_packets([f if cap is None else f[:cap] for f, cap, _ in cases])
    res = O.decode(batch, L.LayerTypeEthernet, ALL, 0, ext=True)
    segs = TS.segments(batch, res)
    want = [(i, e) for i, (_, _, e) in enumerate(cases) if e is not None]
    assert list(segs["packet"]) == [i for i, _ in want]
    for r, (i, e) in zip(segs, want):
        got = {k: int(r[k]) for k in e}
        assert got == e, (i, got, e)
        assert int(r["flow_id"]) == TS.FLOW_NONE and not r["reserved"].any()
    # the payload bytes are the ones the frames were built with
    p = batch.packet(11)
    assert bytes(p[104:110]) == b"inner!"


def test_grouping_restatement():
    """Stable by id, ids at or above the bound in one trailing run in packet order."""
    s = np.zeros(8, TS.SEG_DTYPE)
    s["packet"] = np.arange(8) * 3
    s["flow_id"] = [5, 0xFFFFFFFE, 2, 5, 100, 2 | 0x80000000, 5, 99]
    g_s, g, un = TS.group(s, 100)
    assert list(g_s["packet"]) == [6, 0, 9, 18, 21, 3, 12, 15]
    assert [tuple(int(x) for x in r) for r in g] == [(2, 0, 1, 6), (5, 1, 3, 0), (99, 4, 1, 21),
                                                      (TS.UNGROUPED, 5, 3, 3)]
    assert un == 3
    assert TS.group(s[:0], 100)[2] == 0 and len(TS.group(s[:0], 100)[1]) == 0


# ---------------------------------------------------------------- the host part, sanitized
def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/tcpseg_errpath.cpp: a stand-alone program (its own main, the runtime stubbed)
    linked with gpd_tcpseg.hip, host code built with AddressSanitizer and UBSan, run on the CPU
    against every path of gpd_tcp_segments that returns before a device is needed."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "tcpseg_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "tcpseg_errpath.cpp"), os.path.join(CSRC, "gpd_tcpseg.hip"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
