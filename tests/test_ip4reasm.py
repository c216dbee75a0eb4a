"""The IPv4 defragmentation (include/gpd_ip4reasm.h) on the CPU: the ABI and the layouts, the
oracle (tests/ip4reasm_ref.py) against every outcome ip4defrag's own tests assert
(tests/golden/defrag_vectors.json), the state machine of the kernels
(gopacket_amd/csrc/gpd_ip4reasm_walk.h) compiled for the host under the sanitizers against the
oracle, and the entry points' no-device paths."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ip4reasm_ref as RR
import oracle_ref as O
from conftest import ROOT
from gopacket_amd import layers as L
from gopacket_amd.batch import PacketBatch
from ip4reasm_cases import random_frames
from test_defrag import ALL, D, VEC, _frames, struct_frames


def handoff(batch):
    """The hand-off records of a batch, from the CPU oracles."""
    return D.ip4_fragments(batch, O.decode(batch, L.LayerTypeEthernet, ALL, 0, ext=True))


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    from gopacket_amd import ip4reasm as I
    header = open(os.path.join(ROOT, "include", "gpd_ip4reasm.h")).read()
    assert list(I.IP4REASM_EXPORTS) == ["gpd_ip4_defrag_create", "gpd_ip4_defrag_destroy", "gpd_ip4_defrag_run",
                                        "gpd_ip4_defrag_discard", "gpd_ip4_defrag_stats"]
    for name in I.IP4REASM_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name + "(" in header, name
        assert name not in _lib.EXPORTS
    for cite in ("defrag.go:86-135", ":216-273", ":278-328", ":140-151", ":120-125", "ip4.go:214-218"):
        assert cite in header, cite
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()


def test_lazy_reexport():
    import gopacket_amd
    assert gopacket_amd.ip4reasm.NewIPv4Defragmenter is not None
    assert "ip4reasm" in gopacket_amd.__all__


def test_struct_layouts_and_constants_match_c(tmp_path):
    from gopacket_amd import ip4reasm as I
    assert I.OUTCOME_DTYPE == RR.OUTCOME_DTYPE and I.DGRAM_DTYPE == RR.DGRAM_DTYPE
    structs = (("gpd_ip4_outcome", I.OUTCOME_DTYPE, 8), ("gpd_ip4_dgram", I.DGRAM_DTYPE, 32))
    consts = (("GPD_IP4_FILED", I.FILED), ("GPD_IP4_COMPLETE", I.COMPLETE), ("GPD_IP4_REJECTED", I.REJECTED),
              ("GPD_IP4_UNCHANGED", I.UNCHANGED), ("GPD_IP4_HOLE", I.HOLE), ("GPD_IP4_INVALID", I.INVALID),
              ("GPD_IP4_LIST_FULL", I.LIST_FULL), ("GPD_IP4_D_SHORT_SLICE", I.D_SHORT_SLICE),
              ("GPD_IP4_MAX_LIST_LEN", I.MAX_LIST_LEN))
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
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_ip4reasm.h"\nint main(void){' +
                    "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == want
    import ip4defrag_ref as R
    assert I.MAX_LIST_LEN == R.IPv4MaximumFragmentListLen
    assert (RR.FILED, RR.COMPLETE, RR.REJECTED, RR.UNCHANGED, RR.HOLE, RR.INVALID, RR.LIST_FULL) == tuple(range(7))
    assert I.OUTCOME_ERRORS[I.HOLE] in RR.ERR_WHAT and I.OUTCOME_ERRORS[I.INVALID] in RR.ERR_WHAT
    # the length limit's text is the oracle's own
    d = R.NewIPv4Defragmenter()
    d.ip_flows[(b"\1\1\1\1", b"\2\2\2\2", 7)] = fl = R.FragmentList()
    fl.frags = [None] * 8191
    fl.highest = 100
    rec = np.zeros((), RR.FRAG_DTYPE)
    rec["src"], rec["dst"], rec["id"], rec["ihl"], rec["length"], rec["flags"] = [1] * 4, [2] * 4, 7, 5, 120, 1
    rec["frag_offset"], rec["payload_len"] = 8183, 100
    assert d.DefragIPv4WithTimestamp(rec, bytes(120), 1)[1] == I.OUTCOME_ERRORS[I.LIST_FULL]


# ---------------------------------------------------------------- the oracle, pinned
def _run_names(ref, names, fr, **kw):
    batch = PacketBatch.from_packets([fr[k] for k in names])
    return ref.run(batch, handoff(batch), **kw)


def test_ref_reproduces_defrag_test_go():
    """Every outcome ip4defrag/defrag_test.go asserts, through the batch oracle: the ping
    payloads byte for byte (TestDefragPing1, twice on one defragmenter), duplicates
    (TestDefragPingMultipleFrags), TestDefragPing1and2's completion order, the Id field, Discard,
    and the struct cases (TooSmall, FragmentOffset, MaxSize)."""
    fr = _frames()
    a = VEC["asserted"]
    want = {p: b"".join(fr[f"testPing{p}Frag{k}"][a["payload_from"]:] for k in (1, 2, 3, 4)) for p in (1, 2)}
    assert len(want[1]) == a["datagram_payload_len"]
    order = ["testPing1Frag1", "testPing1Frag3", "testPing1Frag2", "testPing1Frag4"]
    ref = RR.RefDefragmenter()
    for rnd in range(2):  # two batches on one defragmenter
        r = _run_names(ref, order, fr)
        assert list(r.outcomes["what"]) == [RR.FILED] * 3 + [RR.COMPLETE] and len(r.dgrams) == 1
        g = r.dgrams[0]
        assert r.payloads[0] == want[1] and g["payload_len"] == len(want[1]) == g["length"]
        assert g["id"] == struct.unpack(">H", fr["testPing1Frag1"][18:20])[0]  # TestDefragIDField
        assert g["nfrags"] == 4 and g["packet"] == 3 and g["frag"] == 3 and g["ihl"] == 5 and g["protocol"] == 1
        # the bytes: the completing fragment's header, patched, then the payload
        b = r.bytes.tobytes()
        assert len(b) == 20 + len(want[1]) == int(r.caplen[0]) and b[20:] == want[1]
        h4 = fr["testPing1Frag4"][14:34]
        assert b[:2] == h4[:2] and b[4:6] == h4[4:6] and b[8:10] == h4[8:10] and b[12:20] == h4[12:20]
        assert b[2:4] == struct.pack(">H", 20 + len(want[1])) and b[6:8] == b"\0\0" and RR.ip_checksum(b[:20]) == 0
        assert ref.stats() == {"lists": 0, "fragments": 0, "bytes": 0}
    r = _run_names(RR.RefDefragmenter(), ["testPing1Frag1"] * 3 + order[1:], fr)
    assert list(r.outcomes["what"]) == [RR.FILED] * 5 + [RR.COMPLETE] and r.payloads[0] == want[1]
    ref = RR.RefDefragmenter()
    r = _run_names(ref, a["ping1_and2_order"], fr)
    done = [a["ping1_and2_order"][int(g["frag"])] for g in r.dgrams]
    assert done == [a["completing"]["ping1"], a["completing"]["ping2_after_ping1_and2_order"]]
    assert r.payloads == [want[1], want[2]] and list(r.outcomes["datagram"][r.outcomes["what"] == RR.COMPLETE]) == [0, 1]
    assert int(r.offset[1]) == 20 + len(want[1])
    ref = RR.RefDefragmenter()  # TestDefragDiscard
    _run_names(ref, ["testPing1Frag1", "testPing2Frag1"], fr, now=1)
    assert ref.stats()["lists"] == 2 and ref.discard(2) == 2 and ref.stats()["lists"] == 0
    # the struct cases, each test's layers through one defragmenter
    cases = struct_frames()
    by_test = {}
    for k, (s, _) in enumerate(cases):
        by_test.setdefault(s["test"].split()[0], []).append(k)
    for name, ks in by_test.items():
        batch = PacketBatch.from_packets([cases[k][1] for k in ks])
        recs = handoff(batch)
        r = RR.RefDefragmenter().run(batch, recs)
        by_pkt = {int(x["packet"]): int(o["what"]) for x, o in zip(recs, r.outcomes)}
        for j, k in enumerate(ks):
            s = cases[k][0]
            if s.get("unchanged"):
                assert j not in by_pkt, s["test"]
            else:
                assert (by_pkt[j] == RR.REJECTED) == s["error"] and by_pkt[j] in (RR.REJECTED, RR.FILED), s["test"]


def test_ref_on_the_crafted_shapes():
    """The shapes of tests/ip4reasm_cases.py do what their docstrings say."""
    from ip4reasm_cases import frames_of, hole_then_piece, invalid, key_of, quirk_complete, short_slice
    rng = np.random.default_rng(3)

    def run(g, key=key_of(0)):
        batch = PacketBatch.from_packets(frames_of(rng, g, key))
        ref = RR.RefDefragmenter()
        return ref, ref.run(batch, handoff(batch))

    _, r = run(quirk_complete(2))
    assert list(r.outcomes["what"]) == [RR.FILED, RR.FILED, RR.COMPLETE]
    assert (r.dgrams[0]["payload_len"], r.dgrams[0]["length"], r.dgrams[0]["flags"]) == (80, 96, 0)
    _, r = run(short_slice(6))
    assert list(r.outcomes["what"]) == [RR.FILED, RR.FILED, RR.COMPLETE] and r.dgrams[0]["flags"] == RR.D_SHORT_SLICE
    _, r = run(quirk_complete(2, cap=14 + 20 + 5))
    assert r.dgrams[0]["flags"] == RR.D_SHORT_SLICE
    ref, r = run(invalid())
    assert list(r.outcomes["what"]) == [RR.FILED, RR.FILED, RR.INVALID] and ref.stats()["fragments"] == 3
    ref, r = run(hole_then_piece())
    assert list(r.outcomes["what"]) == [RR.FILED, RR.FILED, RR.HOLE, RR.FILED, RR.FILED]
    assert ref.stats()["fragments"] == 3  # the list stays after the hole


# ---------------------------------------------------------------- the state machine, sanitized
@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("walk") / "ip4reasm_walk_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "c", "ip4reasm_walk_host.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _group_text(batch, recs, rows, split, ts):
    lines = ["%d %d" % (len(rows), split)]
    for i in rows:
        r = recs[i]
        src = int(batch.offset[int(r["packet"])]) + int(r["net_off"]) + 4 * int(r["ihl"])
        lines.append("%d %d %d %d %d %d" % (src, r["payload_len"], r["frag_offset"], r["length"], int(r["flags"]) & 1,
                                            ts[int(r["packet"])]))
    return lines


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_walk_on_the_host_equals_the_oracle(walk_host, tmp_path, seed):
    """A stand-alone program (its own main) includes gpd_ip4reasm_walk.h, built with
    AddressSanitizer and UBSan: insert, build and the flushes over 1,000 generated groups per
    seed (3,000 in all), each cut into two batches at a random record with the list carried
    between them, every batch's node and piece arrays sized to exactly the carried nodes plus
    its records.  Outcomes, datagram fields, the pieces' bytes and the list left behind equal
    the oracle's."""
    batch = PacketBatch.from_packets(random_frames(seed, 1000))
    recs = handoff(batch)
    rng = np.random.default_rng(seed)
    ts = rng.integers(1, 1 << 40, batch.n)
    groups = {}
    for i, r in enumerate(recs):
        if int(r["verdict"]) == RR.FRAG_INSERT:
            groups.setdefault((bytes(r["src"]), bytes(r["dst"]), int(r["id"])), []).append(i)
    assert len(groups) == 1000
    lines = [str(len(groups))]
    for rows in groups.values():
        lines += _group_text(batch, recs, rows, int(rng.integers(0, len(rows) + 1)), ts)
    inp = tmp_path / "groups.txt"
    inp.write_text("\n".join(lines) + "\n")
    p = subprocess.run([walk_host, str(inp)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = iter(p.stdout.split("\n"))
    ref = RR.RefDefragmenter()
    e = ref.run(batch, recs, ts=ts)
    data = batch.data.tobytes()
    seen = set()
    for key, rows in groups.items():
        for i in rows:
            o = list(map(int, next(got).split()[1:]))
            assert o[0] == int(e.outcomes[i]["what"]), (key, i, o)
            seen.add(o[0])
            if o[0] == RR.COMPLETE:
                g = e.dgrams[int(e.outcomes[i]["datagram"])]
                assert o[1:5] == [g["payload_len"], g["nfrags"], g["length"], g["flags"]], (key, i, o)
                pay, pos = b"", 0
                for _ in range(o[5]):
                    src, ln, at = map(int, next(got).split()[1:])
                    assert at == pos
                    pay += data[src:src + ln]
                    pos += ln
                assert pay == e.payloads[int(e.outcomes[i]["datagram"])]
        nn, hi, cur, fin, seen_t = map(int, next(got).split()[1:])
        fl = ref.d.ip_flows.get(key)
        assert nn == (len(fl.frags) if fl else 0)
        if fl:
            assert (hi, cur, bool(fin), seen_t) == (fl.highest, fl.current, fl.final_received, fl.last_seen)
    assert next(got) == "" and seen == {RR.FILED, RR.COMPLETE, RR.HOLE, RR.INVALID}
    assert (e.dgrams["flags"] & RR.D_SHORT_SLICE).any() and (e.dgrams["payload_len"] != e.dgrams["length"]).any()


def test_walk_on_the_host_at_the_length_limit(walk_host, tmp_path):
    """One key, 8,193 fragments at offset 8183 whose end wraps past 65535, so every one is a
    PushBack: the 8,192nd insert flushes the list (LIST_FULL) and the key starts afresh."""
    lines = ["1", "8193 4000"] + ["0 100 8183 120 1 %d" % (k + 1) for k in range(8193)]
    inp = tmp_path / "full.txt"
    inp.write_text("\n".join(lines) + "\n")
    p = subprocess.run([walk_host, str(inp)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.split("\n")
    what = [int(x.split()[1]) for x in out[:8193]]
    assert what == [RR.FILED] * 8191 + [RR.LIST_FULL, RR.FILED]
    assert out[8193] == "L 1 28 100 0 8193"


# ---------------------------------------------------------------- the host part, sanitized
def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/ip4reasm_errpath.cpp: a stand-alone program (its own main, the runtime stubbed)
    linked with gpd_ip4reasm.hip, host code built with AddressSanitizer and UBSan, run on the CPU
    against every path of the entry points that returns before a device is needed."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "ip4reasm_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "ip4reasm_errpath.cpp"),
                    os.path.join(CSRC, "gpd_ip4reasm.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_outcome_error_texts():
    from gopacket_amd import ip4reasm as I
    assert I.outcome_error(I.FILED) is None and I.outcome_error(I.COMPLETE) is None
    assert I.outcome_error(I.HOLE) == "defrag: building - hole found"
    rec = np.zeros((), RR.FRAG_DTYPE)
    rec["verdict"], rec["length"], rec["ihl"] = 1, 27, 5
    assert I.outcome_error(I.REJECTED, rec) == "defrag: fragment too small (handcrafted? 7 < 8)"
