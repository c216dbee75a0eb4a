"""The TCP stream assembly (include/gpd_tcpstream.h) on the CPU: the ABI and the layouts, the
oracle (tests/tcpstream_ref.py) against tcpassembly's own vectors and two hand-checked drain
cases, the sequential step of the kernels (gopacket_amd/csrc/gpd_tcpstream_walk.h) compiled for the
host under the sanitizers against the oracle, the entry point's no-device paths, and `deliver`."""
import os
import subprocess

import numpy as np
import pytest

import tcpassembly_ref as TA
import tcpstream_ref as SR
from conftest import ROOT
from tcpseg_cases import VEC, vec_bytes, vec_want
from tcpstream_cases import crafted, gen_groups

FIN, SYN, RST = 1, 2, 4


# ---------------------------------------------------------------- the ABI
def test_symbol_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    from gopacket_amd import tcpassembly as T
    from gopacket_amd import tcpstream as S
    header = open(os.path.join(ROOT, "include", "gpd_tcpstream.h")).read()
    assert list(S.TCPSTREAM_EXPORTS) == ["gpd_tcp_assemble"]
    for name in S.TCPSTREAM_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name + "(" in header, name
        assert name not in _lib.EXPORTS and name not in T.TCPSEG_EXPORTS
    assert "MaxBufferedPagesTotal" in header and "reordering horizon" in header
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()


def test_lazy_reexport():
    import gopacket_amd
    assert gopacket_amd.tcpstream.TCPStreams is not None
    assert "tcpstream" in gopacket_amd.__all__


def test_struct_layouts_and_constants_match_c(tmp_path):
    from gopacket_amd import tcpstream as S
    assert S.REASM_DTYPE == SR.REASM_DTYPE and S.STREAM_DTYPE == SR.STREAM_DTYPE and S.CONN_DTYPE == SR.CONN_DTYPE
    structs = (("gpd_tcp_reasm", S.REASM_DTYPE, 32), ("gpd_tcp_stream", S.STREAM_DTYPE, 48),
               ("gpd_tcp_conn", S.CONN_DTYPE, 8),
               ("gpd_tcp_asm_opts", np.dtype([("max_pages_per_connection", "<u4"), ("close_all", "<u4")]), 8))
    consts = (("GPD_TCP_R_START", S.R_START), ("GPD_TCP_R_END", S.R_END), ("GPD_TCP_R_FLUSHED", S.R_FLUSHED),
              ("GPD_TCP_CONN_OPEN", S.CONN_OPEN), ("GPD_TCP_PAGE_BYTES", S.PAGE_BYTES),
              ("GPD_TCP_UNGROUPED", S.TCP_UNGROUPED))
    exprs, want = [], []
    for name, dt, size in structs:
        assert dt.itemsize == size
        exprs.append(f"sizeof({name})")
        want.append(size)
        for f in dt.names:
            exprs.append(f"offsetof({name}, {f})")
            want.append(dt.fields[f][1])
    for name, v in consts:
        exprs.append(f"(size_t){name}")
        want.append(v)
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_tcpstream.h"\nint main(void){' +
                    "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == want
    assert S.PAGE_BYTES == TA.PAGE_BYTES == VEC["page_bytes"]
    assert S.GpdTcpAsmOpts.max_pages_per_connection.offset == 0 and S.GpdTcpAsmOpts.close_all.offset == 4


# ---------------------------------------------------------------- the oracle
def _one_group(segments):
    """(batch, segs, groups) for one key, segments as (seq, flags, payload bytes)."""
    batch, segs, groups = crafted([[(s, f, len(p)) for s, f, p in segments]])
    data = batch.data.copy()
    for r, (_, _, p) in zip(segs, segments):  # the payloads asked for, not random fill
        at = int(batch.offset[int(r["packet"])]) + int(r["payload_off"])
        data[at:at + len(p)] = np.frombuffer(bytes(p), np.uint8)
    batch.data[:] = data
    return batch, segs, groups


def test_oracle_reproduces_every_reference_vector():
    """All eight assembly_test.go streams at MaxBufferedPagesPerConnection 4 through the oracle's
    record arrays: call by call the vectors' Reassembly lists, and nothing in between (the drain
    runs after the last step; what it adds is cut off here and checked by hand below)."""
    assert len(VEC["tests"]) == 8
    for name, steps in VEC["tests"].items():
        segments = [(s["seq"], SYN if s["syn"] else 0, vec_bytes(s["payload"])) for s in steps]
        batch, segs, groups = _one_group(segments)
        e = SR.assemble(segs, groups, batch.packet, max_pages=VEC["max_buffered_pages_per_connection"])
        want = [vec_want(s) for s in steps if s["want"]]
        calls = []
        for c in range(int(e.streams[0]["ncalls"])):
            rs = e.recs[e.recs["call"] == c]
            if (rs["flags"] & SR.R_FLUSHED).any():
                assert (rs["flags"] & SR.R_FLUSHED).all()
                continue
            calls.append([(e.bytes[int(r["stream_off"]):int(r["stream_off"]) + int(r["len"])].tobytes(), int(r["skip"]),
                           bool(r["flags"] & SR.R_START), bool(r["flags"] & SR.R_END)) for r in rs])
        assert calls == want, name
        # the records point at the bytes they carry
        for r in e.recs:
            p = batch.packet(int(r["packet"]))
            assert bytes(p[int(r["src_off"]):int(r["src_off"]) + int(r["len"])]) == \
                e.bytes[int(r["stream_off"]):int(r["stream_off"]) + int(r["len"])].tobytes()


HAND = [(1001, 0, bytes([1, 2, 3])), (1004, 0, bytes([2, 2, 3])), (1010, 0, bytes([4, 2, 3]))]


def _calls(e):
    ev = e.events[0]
    return SR.call_lists(ev), [fl for fl, _ in ev.calls]


def test_hand_checked_drain_case_1():
    """No SYN, page limit 4, no close_all: all three wait for a start, the drain skips to the
    first (-1), takes the contiguous second with it, then skips the gap of 3."""
    batch, segs, groups = _one_group(HAND)
    e = SR.assemble(segs, groups, batch.packet, max_pages=4, close_all=False)
    calls, flushed = _calls(e)
    assert calls == [[(bytes([1, 2, 3]), -1, False, False), (bytes([2, 2, 3]), 0, False, False)],
                     [(bytes([4, 2, 3]), 3, False, False)]]
    assert flushed == [True, True]
    s = e.streams[0]
    assert (int(s["open"]), int(s["next_seq"]), int(s["completed"]), int(s["ncalls"]), int(s["nrec"])) == \
        (1, 1013, 0, 2, 3)
    assert e.bytes.tobytes() == bytes([1, 2, 3, 2, 2, 3, 4, 2, 3])
    assert list(e.recs["call"]) == [0, 0, 1] and list(e.recs["flags"]) == [SR.R_FLUSHED] * 3
    assert (e.nrecs, e.nstreams, e.nbytes, e.ncalls) == (3, 1, 9, 2)


def test_hand_checked_drain_case_2():
    """The same with FIN on the third segment and close_all: the last record has End, one
    ReassemblyComplete, nothing left open for FlushAll to close."""
    segments = HAND[:2] + [(1010, FIN, bytes([4, 2, 3]))]
    batch, segs, groups = _one_group(segments)
    e = SR.assemble(segs, groups, batch.packet, max_pages=4, close_all=True)
    calls, _ = _calls(e)
    assert calls == [[(bytes([1, 2, 3]), -1, False, False), (bytes([2, 2, 3]), 0, False, False)],
                     [(bytes([4, 2, 3]), 3, False, True)]]
    s = e.streams[0]
    assert (int(s["open"]), int(s["completed"]), int(s["next_seq"])) == (0, 1, 0)
    assert e.events[0].order == ["new", ("call", 0), ("call", 1), "complete"]
    assert list(e.recs["flags"]) == [SR.R_FLUSHED, SR.R_FLUSHED, SR.R_FLUSHED | SR.R_END]


def test_oracle_state_carry_and_close_all():
    """An open connection is its nextSeq: carried by state, closed by close_all with no call."""
    batch, segs, groups = _one_group([(100, SYN, b""), (101, 0, b"ab")])
    st = np.zeros(4, SR.CONN_DTYPE)
    e = SR.assemble(segs, groups, batch.packet, state=st)
    assert tuple(e.state[0]) == (103, 1) and not st.view(np.uint32).any()
    b2, s2, g2 = _one_group([(105, 0, b"ef"), (103, 0, b"cd")])
    e2 = SR.assemble(s2, g2, b2.packet, state=e.state, close_all=True)
    assert SR.call_lists(e2.events[0]) == [[(b"cd", 0, False, False), (b"ef", 0, False, False)]]
    assert e2.events[0].order == [("call", 0), "complete"] and tuple(e2.state[0]) == (0, 0)
    assert int(e2.streams[0]["completed"]) == 1 and list(e2.recs["flags"]) == [0, 0]


# ---------------------------------------------------------------- the kernels' sequential step, on the host
def _walk_text(e):
    out = []
    for s in e.streams:
        for r in e.recs[int(s["first_rec"]):int(s["first_rec"]) + int(s["nrec"])]:
            out.append("R %d %d %d %d %d %d %d" % (r["packet"], r["src_off"], r["len"], r["skip"],
                                                   int(r["stream_off"]) - int(s["byte_off"]), r["call"], r["flags"]))
        out.append("S %d %d %d %d %d %d" % (s["nrec"], s["ncalls"], s["nbytes"], s["completed"], s["open"],
                                            s["next_seq"]))
    return out


@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("walk") / "tcpstream_walk_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "c", "tcpstream_walk_host.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("max_pages,close_all,seed", [(0, False, 11), (4, False, 12), (0, True, 13), (4, True, 14)])
def test_walk_on_the_host_equals_the_oracle(walk_host, tmp_path, max_pages, close_all, seed):
    """A stand-alone program (its own main) includes gpd_tcpstream_walk.h, built with
    AddressSanitizer and UBSan: the sequential step and the drain over 800 generated groups per
    option set (3,200 in all), every group's arrays sized to exactly its pages; the records and
    the totals equal the oracle's.  A third of the groups start from an open connection."""
    groups = gen_groups(seed, 800, max_segments=60)
    batch, segs, grp = crafted(groups)
    rng = np.random.default_rng(seed)
    state = np.zeros(len(groups), SR.CONN_DTYPE)
    for k in range(0, len(groups), 3):
        state[k] = (int(rng.integers(1 << 32)) if k % 2 else (groups[k][0][0] + 1) & 0xFFFFFFFF, 1)
    e = SR.assemble(segs, grp, lambda i: bytes(int(batch.caplen[i])), max_pages=max_pages, close_all=close_all,
                    state=state)
    lines = ["%d %d %d" % (max_pages, int(close_all), len(grp))]
    for g in grp:
        k = int(g["flow_id"])
        lines.append("%d %d %d" % (g["count"], state[k]["flags"], state[k]["next_seq"]))
        for r in segs[int(g["start"]):int(g["start"]) + int(g["count"])]:
            lines.append("%d %d %d %d %d" % (r["packet"], r["seq"], r["flags"], r["payload_off"], r["payload_len"]))
    inp = tmp_path / "groups.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([walk_host, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = r.stdout.split("\n")[:-1], _walk_text(e)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
    assert e.nrecs > 20000 and (e.recs["skip"] > 0).any() and (e.recs["skip"] == -1).any()
    assert (e.recs["flags"] & SR.R_END).any() and (e.recs["len"] == 0).any()


# ---------------------------------------------------------------- the host part, sanitized
def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/tcpstream_errpath.cpp: a stand-alone program (its own main, the runtime stubbed)
    linked with gpd_tcpstream.hip, host code built with AddressSanitizer and UBSan, run on the CPU
    against every path of gpd_tcp_assemble that returns before a device is needed."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "tcpstream_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "tcpstream_errpath.cpp"),
                    os.path.join(CSRC, "gpd_tcpstream.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


# ---------------------------------------------------------------- deliver
@pytest.mark.parametrize("gather", [True, False])
def test_deliver_gives_the_oracles_call_lists(gather):
    """`deliver` over host copies: a recording StreamFactory sees, key by key, the calls the
    oracle's streams saw, New / Reassembled / ReassemblyComplete in the reference's order."""
    from gopacket_amd import tcpstream as S
    groups = gen_groups(21, 60, max_segments=40)
    batch, segs, grp = crafted(groups, keys=[3 * j + 1 for j in range(len(groups))])
    e = SR.assemble(segs, grp, batch.packet, max_pages=4, close_all=True)
    host = S.HostStreams(e.recs, e.streams, e.bytes if gather else None)

    class Factory:
        def __init__(self):
            self.order, self.calls = {}, {}

        def New(self, key):
            fac = self
            fac.order.setdefault(key, []).append("new")

            class _Stream:
                def Reassembled(self, rs):
                    fac.order[key].append(("call", len(fac.calls.setdefault(key, []))))
                    fac.calls[key].append([r.as_tuple() for r in rs])

                def ReassemblyComplete(self):
                    fac.order[key].append("complete")
            return _Stream()

    def payload(r):
        p = batch.packet(int(r["packet"]))
        return bytes(p[int(r["src_off"]):int(r["src_off"]) + int(r["len"])])

    fac = Factory()
    S.deliver(host, fac, payload=None if gather else payload)
    assert set(fac.order) == {k for k, ev in e.events.items() if ev.order}
    for key, ev in e.events.items():
        if ev.order:
            assert fac.calls.get(key, []) == SR.call_lists(ev), key
            assert fac.order[key] == ev.order, key
    assert sum(o.count("complete") for o in fac.order.values()) == int(e.streams["completed"].sum()) > 10
