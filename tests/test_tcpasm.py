"""The stateful TCP assembler (include/gpd_tcpasm.h) on the CPU: the ABI and the layouts, the
oracle (tests/tcpasm_ref.py) against hand-checked flush cases and tcpassembly's own vectors, the
state machine of the kernels (gopacket_amd/csrc/gpd_tcpasm_walk.h) compiled for the host under the
sanitizers against the oracle over connections cut into several runs, the entry points'
no-device paths, and `deliver`."""
import os
import subprocess

import numpy as np
import pytest

import tcpasm_ref as AR
import tcpassembly_ref as TA
import tcpseg_ref as TS
from conftest import ROOT
from tcpasm_cases import cut_all, set_payloads
from tcpseg_cases import VEC, vec_bytes, vec_want
from tcpstream_cases import crafted, gen_groups

FIN, SYN, RST = 1, 2, 4


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    from gopacket_amd import tcpasm as M
    from gopacket_amd import tcpstream as S
    header = open(os.path.join(ROOT, "include", "gpd_tcpasm.h")).read()
    assert list(M.TCPASM_EXPORTS) == ["gpd_tcp_assembler_create", "gpd_tcp_assembler_destroy",
                                      "gpd_tcp_assembler_run", "gpd_tcp_assembler_reset",
                                      "gpd_tcp_assembler_stats", "gpd_tcp_assembler_conns"]
    for name in M.TCPASM_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name + "(" in header, name
        assert name not in _lib.EXPORTS and name not in S.TCPSTREAM_EXPORTS
    assert "MaxBufferedPagesTotal" in header and "FlushWithOptions" in header
    assert "gpd_tcpasm.h" in open(os.path.join(ROOT, "include", "gpd_tcpstream.h")).read()
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()


def test_lazy_reexport():
    import gopacket_amd
    assert gopacket_amd.tcpasm.NewAssembler is not None
    assert "tcpasm" in gopacket_amd.__all__


def test_struct_layouts_and_constants_match_c(tmp_path):
    from gopacket_amd import tcpasm as M
    assert M.CONN_INFO_DTYPE == AR.CONN_INFO_DTYPE
    structs = (("gpd_tcp_conn_info", M.CONN_INFO_DTYPE, 24),
               ("gpd_tcp_flush", np.dtype([("before_ns", "<u8"), ("close_all", "<u4"), ("flush_all", "<u4")]), 16))
    consts = (("GPD_TCP_CONN_OPEN", M.CONN_OPEN), ("GPD_TCP_CONN_NOSEQ", M.CONN_NOSEQ),
              ("GPD_TCP_R_FLUSHED", M.R_FLUSHED), ("GPD_TCP_R_CARRIED", M.R_CARRIED),
              ("GPD_TCP_NO_PACKET", M.NO_PACKET), ("GPD_TCP_R_START", AR.R_START), ("GPD_TCP_R_END", AR.R_END))
    assert (M.CONN_NOSEQ, M.R_CARRIED, M.NO_PACKET) == (2, 8, 0xFFFFFFFF)
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
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_tcpasm.h"\nint main(void){' +
                    "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == want
    assert M.GpdTcpFlush.before_ns.offset == 0 and M.GpdTcpFlush.close_all.offset == 8
    assert M.GpdTcpFlush.flush_all.offset == 12


# ---------------------------------------------------------------- the oracle
def _one_key(segments, ts):
    """(batch, segs, groups, ts) for one key 0: segments as (seq, flags, payload bytes)."""
    batch, segs, groups = crafted([[(s, f, len(p)) for s, f, p in segments]])
    set_payloads(batch, segs, [p for _, _, p in segments])
    return batch, segs, groups, list(ts)


def _calls(ev, since=0):
    return AR.call_lists(ev)[since:]


EXAMPLE = [(9, SYN, b""), (15, 0, b"AAAAA"), (20, 0, b"BBBBB"), (30, 0, b"C" * 20)]
EXAMPLE_TS = [100, 200, 300, 400]


def test_flush_example_of_the_reference_comment():
    """assembly.go:213-223: processed through 10, bytes [15,20) [20,25) [30,50) in the list.  A
    flush with T between the Seen of [15,20) and of [30,50) pushes [15,20) and the contiguous
    [20,25) in one call, the first with Skip 5; [30,50) stays.  A later T sends it, Skip 5.
    CloseAll with T past lastSeen closes.  Seen == T and lastSeen == T do nothing."""
    m = AR.Model(4)
    batch, segs, groups, ts = _one_key(EXAMPLE, EXAMPLE_TS)
    e = m.run(segs, groups, batch.packet, ts=ts)
    ev = m.keys[0]
    assert _calls(ev) == [[(b"", 0, True, False, 100)]] and tuple(e.conns[0]) == (10, 1, 3, 30, 400)
    assert e.out == (1, 1, 0, 1, 1, 3, 30, 0) and int(e.streams[0]["reserved"]) == 3
    # Seen == T: nothing is before it
    e = m.run(T=200, close_all=True)
    assert e.out == (0, 0, 0, 0, 1, 3, 30, 0) and len(e.streams) == 0 and tuple(e.conns[0]) == (10, 1, 3, 30, 400)
    # T between 200 and 400
    e = m.run(T=250)
    assert _calls(ev, 1) == [[(b"AAAAA", 5, False, False, 200), (b"BBBBB", 0, False, False, 300)]]
    assert list(e.recs["flags"]) == [AR.R_FLUSHED | AR.R_CARRIED] * 2 and list(e.recs["call"]) == [0, 0]
    assert list(e.recs["packet"]) == [AR.NO_PACKET] * 2 and list(e.recs["src_off"]) == [0, 0]
    assert list(e.seen_ns) == [200, 300] and e.bytes.tobytes() == b"AAAAABBBBB"
    assert tuple(e.conns[0]) == (25, 1, 1, 20, 400) and e.out == (2, 1, 10, 1, 1, 1, 20, 0)
    assert tuple(e.streams[0]) == (0, 0, 2, 1, 0, 10, 0, 1, 25, 1)
    # a second flush with a later T sends [30,50) with Skip 5
    e = m.run(T=401)
    assert _calls(ev, 2) == [[(b"C" * 20, 5, False, False, 400)]]
    assert tuple(e.conns[0]) == (50, 1, 0, 0, 400) and AR.order_of(ev) == ["new", "call", "call", "call"]
    # lastSeen == T: no close
    e = m.run(T=400, close_all=True)
    assert e.out == (0, 0, 0, 0, 1, 0, 0, 0) and m.open_keys() == [0]
    # CloseAll without T past lastSeen: no close either; with it: closed, one completion, no call
    e = m.run(T=401, close_all=False)
    assert m.open_keys() == [0]
    e = m.run(T=401, close_all=True)
    assert m.open_keys() == [] and AR.order_of(ev)[-1] == "complete" and e.out == (0, 1, 0, 0, 0, 0, 0, 0)
    assert tuple(e.streams[0]) == (0, 0, 0, 0, 0, 0, 1, 0, 0, 0) and not e.conns.view(np.uint8).any()


def test_flush_of_a_connection_without_syn():
    """No SYN: the data waits with nextSeq invalid (NOSEQ), T = 0 flushes nothing, FlushOlderThan
    sends it with Skip -1 and, the list drained and lastSeen before T, closes."""
    m = AR.Model(2)
    batch, segs, groups, ts = _one_key([(1001, 0, b"abc"), (1010, 0, b"xyz")], [50, 60])
    e = m.run(segs, groups, batch.packet, ts=ts)
    assert e.out == (0, 1, 0, 0, 1, 2, 6, 0) and tuple(e.conns[0]) == (0, 3, 2, 6, 60)
    assert tuple(e.streams[0]) == (0, 0, 0, 0, 0, 0, 0, 3, 0, 2)
    e = m.run(T=55)
    ev = m.keys[0]
    assert _calls(ev) == [[(b"abc", -1, False, False, 50)]] and tuple(e.conns[0]) == (1004, 1, 1, 3, 60)
    e = m.run(T=61, close_all=True)  # FlushOlderThan(61)
    assert _calls(ev, 1) == [[(b"xyz", 6, False, False, 60)]]
    assert AR.order_of(ev) == ["new", "call", "call", "complete"] and m.open_keys() == []
    assert int(e.streams[0]["completed"]) == 1 and int(e.streams[0]["open"]) == 0


def test_flush_all_and_a_segment_that_fills_a_carried_gap():
    m = AR.Model(1)
    batch, segs, groups, ts = _one_key([(9, SYN, b""), (12, 0, b"cd")], [1, 2])
    m.run(segs, groups, batch.packet, ts=ts)
    b2, s2, g2, t2 = _one_key([(10, 0, b"ab")], [3])
    e = m.run(s2, g2, b2.packet, ts=t2)
    assert _calls(m.keys[0], 1) == [[(b"ab", 0, False, False, 3), (b"cd", 0, False, False, 2)]]
    assert list(e.recs["flags"]) == [0, AR.R_CARRIED] and list(e.recs["packet"]) == [0, AR.NO_PACKET]
    e = m.run(flush_all=True)
    assert e.out == (0, 1, 0, 0, 0, 0, 0, 0) and AR.order_of(m.keys[0])[-1] == "complete"


def test_oracle_reproduces_every_reference_vector():
    """All eight assembly_test.go streams at MaxBufferedPagesPerConnection 4 through the stateful
    subclass with no flush, whole and cut into one run per packet: the vectors' lists, call by
    call."""
    assert len(VEC["tests"]) == 8
    for name, steps in VEC["tests"].items():
        segments = [(s["seq"], SYN if s["syn"] else 0, vec_bytes(s["payload"])) for s in steps]
        want = [vec_want(s) for s in steps if s["want"]]
        batch, segs, groups, ts = _one_key(segments, range(len(segments)))
        for cuts in ([0, len(segments)], list(range(len(segments) + 1))):
            m = AR.Model(1, max_pages=VEC["max_buffered_pages_per_connection"])
            for b, s, g in cut_all(batch, segs, cuts):
                m.run(s, g, b.packet)
            assert [[c[:4] for c in call] for call in _calls(m.keys[0])] == want, (name, len(cuts))


# ---------------------------------------------------------------- the kernels' state machine, on the host
@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("walk") / "tcpasm_walk_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "c", "tcpasm_walk_host.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("max_pages,seed", [(0, 31), (4, 32), (1, 33), (0, 34)])
def test_walk_on_the_host_equals_the_oracle(walk_host, tmp_path, max_pages, seed):
    """A stand-alone program (its own main) includes gpd_tcpasm_walk.h, built with
    AddressSanitizer and UBSan: 750 generated connections per option set (3,000 in all), each cut
    into two or three runs (a quarter with a pure flush run behind), the page list carried
    between the runs through arrays of exactly conn.pages records, node and record arrays of
    exactly the bound, T / close_all / flush_all drawn per run (T from 0, a packet's timestamp,
    one past it, and later than all); records, Seen and connection state equal the oracle's."""
    groups = gen_groups(seed, 750, max_segments=60)
    batch, segs, grp = crafted(groups)
    rng = np.random.default_rng(seed)
    lines, want = ["%d %d" % (max_pages, len(grp))], []
    stamp = lambda p: 1000 + 7 * p
    carried_recs = skips = noseq = 0
    for g in grp:
        mine = segs[int(g["start"]):int(g["start"]) + int(g["count"])]
        n = len(mine)
        nruns = min(int(rng.integers(2, 4)), n)
        cuts = [0] + sorted(rng.choice(np.arange(1, n), nruns - 1, replace=False).tolist()) + [n] if nruns > 1 else [0, n]
        runs = [mine[cuts[k]:cuts[k + 1]] for k in range(len(cuts) - 1)]
        if rng.random() < 0.25:
            runs.append(mine[:0])
        lines.append("%d" % len(runs))
        m = AR.Model(1, max_pages=max_pages)
        for rs in runs:
            hi = int(rs["packet"].max()) if len(rs) else int(mine["packet"].max())
            pick = stamp(int(mine["packet"][rng.integers(n)]))
            T = int((0, 0, pick, pick + 1, stamp(hi) + 1, 1 << 62)[rng.integers(6)])
            close_all, flush_all = bool(rng.random() < 0.4), bool(rng.random() < 0.15)
            lines.append("%d %d %d %d" % (len(rs), T, close_all, flush_all))
            ts = {}
            for r in rs:
                ts[int(r["packet"])] = stamp(int(r["packet"]))
                lines.append("%d %d %d %d %d %d" % (r["packet"], r["seq"], r["flags"], r["payload_off"],
                                                    r["payload_len"], stamp(int(r["packet"]))))
            sub = rs.copy()
            sub["flow_id"] = 0
            gr = np.array([(0, 0, len(sub), int(sub["packet"][0]))], TS.GROUP_DTYPE) if len(sub) else None
            e = m.run(sub if len(sub) else None, gr, lambda i: bytes(int(batch.caplen[i])), ts=ts, T=T,
                      close_all=close_all, flush_all=flush_all)
            for r, sn in zip(e.recs, e.seen_ns):
                want.append("R %d %d %d %d %d %d %d %d" % (r["packet"], r["src_off"], r["len"], r["skip"],
                                                           r["stream_off"], r["call"], r["flags"], sn))
            s = e.streams[0] if len(e.streams) else np.zeros(1, AR.STREAM_DTYPE)[0]
            c = e.conns[0]
            want.append("S %d %d %d %d %d %d %d %d %d" % (s["nrec"], s["ncalls"], s["nbytes"], s["completed"], c["flags"],
                                                          c["next_seq"], c["pages"], c["page_bytes"], c["last_seen_ns"]))
            carried_recs += int((e.recs["flags"] & AR.R_CARRIED != 0).sum())
            skips += int((e.recs["skip"] > 0).sum())
            noseq += int(c["flags"]) >> 1
    inp = tmp_path / "conns.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([walk_host, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
    # (with a page limit of 1 every insert pops at once: no page outlives its run)
    assert (carried_recs == 0 if max_pages == 1 else carried_recs > 300) and skips > 100
    assert max_pages == 1 or noseq > 50


# ---------------------------------------------------------------- the host part, sanitized
def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/tcpasm_errpath.cpp: a stand-alone program (its own main, the context stubbed)
    linked with gpd_tcpasm.hip, host code built with AddressSanitizer and UBSan, run on the CPU
    against every path of the entry points that returns before a device is needed."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "tcpasm_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "tcpasm_errpath.cpp"),
                    os.path.join(CSRC, "gpd_tcpasm.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


# ---------------------------------------------------------------- deliver
class Factory:
    def __init__(self):
        self.order, self.calls = {}, {}

    def New(self, key):
        fac = self
        fac.order.setdefault(key, []).append("new")

        class _Stream:
            def Reassembled(self, rs):
                fac.order[key].append("call")
                fac.calls.setdefault(key, []).append([r.as_tuple() + (r.Seen,) for r in rs])

            def ReassemblyComplete(self):
                fac.order[key].append("complete")
        return _Stream()


def test_deliver_makes_the_references_calls_across_runs():
    """`deliver` over the oracle's arrays, run after run, into one recording factory: key by key
    New / Reassembled / ReassemblyComplete in the reference's order with Seen as a timestamp.  New
    is called once for a connection that spans runs, and again after it closed and a SYN
    reopened it."""
    from gopacket_amd import tcpasm as M
    groups = gen_groups(41, 40, max_segments=40)
    groups.append([(100, SYN, 0), (101, 0, 4), (110, 0, 4), (105, 0, 5), (114, FIN, 0), (500, SYN, 2), (503, 0, 3)])
    span, reopen = len(groups) - 1, len(groups)
    groups.append([(7, SYN, 1), (9, FIN, 1)] + [(20, 0, 2)] * 30 + [(50, SYN, 0), (51, 0, 3)])
    steady = len(groups)
    groups.append([(1000, SYN, 0)] + [(1001 + 3 * k, 0, 3) for k in range(60)])
    batch, segs, grp = crafted(groups, keys=[3 * j + 1 for j in range(len(groups))], interleave_seed=9)
    n = batch.n
    ts = [10 * (i + 1) for i in range(n)]
    m = AR.Model(3 * len(groups) + 2, max_pages=4)
    fac, pool = Factory(), {}
    cuts = [0, n // 3, (2 * n) // 3, n]
    for k, (b, s, g) in enumerate(cut_all(batch, segs, cuts)):
        before = np.array(m.open_keys(), np.uint32)
        e = m.run(s, g, b.packet, ts=ts[cuts[k]:cuts[k + 1]], T=ts[cuts[k]] if k else 0, close_all=(k == 1))
        M.deliver(M.HostAsm(e.recs, e.seen_ns, e.streams, e.bytes, before), fac, pool)
    before = np.array(m.open_keys(), np.uint32)
    e = m.run(flush_all=True)
    M.deliver(M.HostAsm(e.recs, e.seen_ns, e.streams, e.bytes, before), fac, pool)
    assert m.open_keys() == [] and pool == {}
    for key, ev in m.keys.items():
        assert fac.order.get(key, []) == AR.order_of(ev), key
        assert fac.calls.get(key, []) == AR.call_lists(ev), key
    # one New for the connection that spans all runs (it has calls in each), one per life otherwise
    assert fac.order[3 * steady + 1] == ["new"] + ["call"] * 61 + ["complete"]
    assert fac.order[3 * span + 1].count("new") == 2 and fac.order[3 * reopen + 1].count("new") >= 2
    assert sum(o.count("complete") for o in fac.order.values()) > 20
