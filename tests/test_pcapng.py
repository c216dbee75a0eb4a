"""pcapng ingest on the host (include/gpd_pcapng.h, gopacket_amd/pcapng.py): the native reader
against pcapgo's own test vectors (tests/golden/pcapng_vectors.json, read from
pcapgo/ngread_test.go by tests/golden/make_pcapng_vectors.py) and against the plain-Python
restatement of pcapgo/ngread.go (tests/ngread_ref.py) on a seeded fuzz."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ng_synth as S
import ngread_ref as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
VECTORS = json.load(open(os.path.join(GOLDEN, "pcapng_vectors.json")))
CASES = [(t, e) for t in VECTORS["tests"] for e in ("le", "be")]
FUZZ_SEEDS = 2400


def _id(c):
    return "%s%s-%s" % (c[0]["name"], c[0]["type"].replace("/", "."), c[1])


def fixture_bytes(t, e):
    with open(os.path.join(GOLDEN, "pcapng", e, t["name"] + ".pcapng"), "rb") as f:
        return f.read()


def flags_of(t):
    return t["want_mixed_linktype"], t["error_on_mismatching_linktype"], t["skip_unknown_version"]


def native(data, flags, max_n=None):
    """The native reader's whole output: (packets as dicts, stop, text, pos, sections seen at
    the end: (section strings, interfaces))."""
    from gopacket_amd import pcapng
    o = pcapng.NgReaderOptions(*flags)
    try:
        r = pcapng.NgReader(data, o)
    except pcapng.PcapNgError as err:
        return [], err.stop, str(err), None, None
    pk, stop, text = [], pcapng.STOP_LIMIT, None
    while stop == pcapng.STOP_LIMIT:
        p = r.index(max_n)
        b = p.batch
        pk += [dict(off=int(b.offset[i]), caplen=int(b.caplen[i]), wirelen=int(p.length[i]), sec=int(p.ts_sec[i]),
                    nsec=int(p.ts_nsec[i]), ifindex=int(p.ifindex[i]), linktype=int(p.linktype[i]))
               for i in range(b.n)]
        stop, text = p.stop, p.err
    state = (r.SectionInfo(), [r.Interface(i) for i in range(r.NInterfaces())], r.LinkType())
    return pk, stop, text, r.pos(), state


def restated(data, flags, section_end=None):
    r = R.NgReaderRef(data, *flags, section_end=section_end)
    pk, stop, text = r.read()
    return r, pk, stop, text


def same_state(r, state):
    sec, ifaces, lt = state
    assert (sec.Hardware, sec.OS, sec.Application, sec.Comment) == tuple(
        r.section[k] for k in ("Hardware", "OS", "Application", "Comment"))
    assert lt == r.linkType
    assert len(ifaces) == len(r.ifaces)
    for a, b in zip(ifaces, r.ifaces):
        assert (a.Name, a.Comment, a.Description, a.Filter, a.OS, a.LinkType, a.TimestampResolution,
                a.TimestampOffset, a.SnapLength) == (b.Name, b.Comment, b.Description, b.Filter, b.OS, b.LinkType,
                                                     b.TimestampResolution, b.TimestampOffset, b.SnapLength)


def opened(data, flags):
    """Whether NewNgReader itself succeeds (the restatement keeps an open failure as a stop)."""
    r = R.NgReaderRef(data, *flags)
    return r.stopped is None, r


def compare(data, flags, max_n=None):
    ok, r0 = opened(data, flags)
    pk, stop, text, pos, state = native(data, flags, max_n)
    if not ok:  # NewNgReader fails: no reader, its stop and text
        assert (pk, stop, text, state) == ([], r0.stopped[0], r0.stopped[1], None)
        return pk, stop, text
    r, rpk, rstop, rtext = restated(data, flags)
    assert len(pk) == len(rpk)
    assert pk == rpk
    assert (stop, text, pos) == (rstop, rtext, r.position())
    same_state(r, state)
    return pk, stop, text


# ---- the reference's own vectors -------------------------------------------------------------

def check_vectors(t, data, pk, stop, text):
    want = [p for p in t["packets"] if "err" not in p]
    errs = [p["err"] for p in t["packets"] if "err" in p]
    assert len(pk) == len(want)
    for got, w in zip(pk, want):
        assert data[got["off"]:got["off"] + got["caplen"]].hex() == w["data"]
        assert (got["sec"], got["nsec"]) == (w["ts_sec"], w["ts_nsec"])
        assert (got["wirelen"], got["caplen"], got["ifindex"]) == (w["Length"], w["CaptureLength"], w["InterfaceIndex"])
        if "linktype" in w:
            assert got["linktype"] == w["linktype"]
    if errs:
        assert text == errs[0]
    else:
        assert (stop, text) == (R.STOP_EOF, None)


def section_matches(want, section, ifaces):
    assert {k: section[k].decode() for k in want["sectionInfo"]} == want["sectionInfo"]
    assert len(ifaces) == len(want["ifaces"])
    for f, w in zip(ifaces, want["ifaces"]):
        got = dict(Name=f.Name.decode(), Comment=f.Comment.decode(), Description=f.Description.decode(),
                   Filter=f.Filter.decode(), OS=f.OS.decode(), LinkType=f.LinkType, SnapLength=f.SnapLength,
                   TimestampResolution=f.TimestampResolution, TimestampOffset=f.TimestampOffset)
        assert got == {k: w[k] for k in got}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_restatement_reads_the_reference_vectors(case):
    """tests/ngread_ref.py against ngread_test.go's table, sections included (its
    SectionEndCallback is how the Go test sees every section of a multi-section file)."""
    t, e = case
    data = fixture_bytes(t, e)
    seen = []
    r, pk, stop, text = restated(data, flags_of(t), section_end=lambda i, s: seen.append((s, i)))
    check_vectors(t, data, pk, stop, text)
    assert r.linkType == (0 if t["want_mixed_linktype"] else t["linkType"])
    if text != "Unknown pcapng Version in Section Header":  # (ngread_test.go:168-170)
        seen.append((r.section, r.ifaces))
        assert len(seen) == len(t["sections"])
        for (s, i), w in zip(seen, t["sections"]):
            section_matches(w, s, i)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_native_reader_reads_the_reference_vectors(case):
    t, e = case
    data = fixture_bytes(t, e)
    pk, stop, text, pos, state = native(data, flags_of(t))
    check_vectors(t, data, pk, stop, text)
    sec, ifaces, lt = state
    assert lt == (0 if t["want_mixed_linktype"] else t["linkType"])
    if text != "Unknown pcapng Version in Section Header":
        section_matches(t["sections"][-1], dict(Hardware=sec.Hardware, OS=sec.OS, Application=sec.Application,
                                                Comment=sec.Comment), ifaces)
    compare(data, flags_of(t))          # ... and every output equals the restatement's
    for m in (1, 2, 7):                 # bounded calls continued == one call
        assert compare(data, flags_of(t), m)[0] == pk


def test_every_fixture_has_vectors():
    names = {t["name"] for t in VECTORS["tests"]}
    for e in ("le", "be"):
        files = sorted(f[:-7] for f in os.listdir(os.path.join(GOLDEN, "pcapng", e)))
        assert files == sorted(names) == [f[:-7] for f in VECTORS["files"][e]]
    assert sum(len(v) for v in VECTORS["files"].values()) == 52
    assert not VECTORS["omitted"]


# ---- fuzz: native reader == restatement in every output ---------------------------------------

def test_fuzz_native_equals_restatement():
    stops, texts, packets = set(), set(), 0
    for seed in range(FUZZ_SEEDS):
        data, flags = S.fuzz_capture(seed)
        pk, stop, text = compare(data, flags)
        stops.add(stop)
        texts.add(re.sub(r"\d+", "N", text or ""))
        packets += len(pk)
    # the fuzz reaches every stop of the reader (MAGIC through a flipped first byte) ...
    assert stops >= set(range(1, 12)), stops
    # ... and both kinds of panic
    assert any("divide by zero" in t for t in texts) and any("option of" in t for t in texts), texts
    assert packets > FUZZ_SEEDS  # (the generator's own health: captures that mostly get somewhere)


def test_fuzz_bounded_calls():
    for seed in range(0, FUZZ_SEEDS, 8):
        data, flags = S.fuzz_capture(seed)
        whole = compare(data, flags)
        for m in (1, 2, 7):
            assert compare(data, flags, m) == whole


def small_capture(e="<"):
    o = S.opt(2, b"eth0", e) + S.opt(9, b"\x09", e) + S.opt(14, struct.pack(e + "Q", 5), e) + S.END[e]
    return b"".join([S.shb(e, S.opt(1, b"cut me", e) + S.END[e]), S.idb(e, 1, 40, o),
                     S.epb(b"A" * 17, e, ts=1234567890123), S.block(0xBAD, b"xxxx", e), S.spb(b"B" * 50, e),
                     S.idb(e, 0, 0), S.pb(b"C" * 9, e, ifindex=1), S.pb(b"D" * 8, e, ifindex=0, ts=7),
                     S.isb(e, 0, 99, S.opt(4, struct.pack(e + "Q", 3), e) + S.END[e]),
                     S.shb(">", S.END[">"]), S.idb(">", 1, 0), S.epb(b"E" * 33, ">")])


def test_cut_at_every_byte():
    for e in "<>":
        data = small_capture(e)
        full = compare(data, (False, False, False))
        assert len(full[0]) == 4 and full[1] == R.STOP_EOF  # the link type 0 packet is dropped
        assert full[0][1]["caplen"] == 40                   # the simple block clipped to snaplen
        for flags in ((False, False, False), (True, False, False)):
            for k in range(len(data)):
                pk, stop, text = compare(data[:k], flags)
                assert stop in (R.STOP_EOF, R.STOP_EOF_BLOCK) and (text or "EOF") == "EOF"


def test_documented_corner_cases():
    e = "<"
    head = S.shb(e) + S.idb(e)
    two = S.epb(b"x" * 20, e) + S.epb(b"y" * 20, e)
    # the trailing length is never checked
    assert len(compare(head + S.epb(b"x" * 20, e, trailer=7) + two, (0, 0, 0))[0]) == 3
    # total_len - 8 wraps: a tiny length skips to EOF
    for bad in (0, 4):
        pk, stop, text = compare(head + S.block(0xBAD, b"", e, total=bad) + two, (0, 0, 0))
        assert (len(pk), stop, text) == (0, R.STOP_EOF_BLOCK, "EOF")
    # a capture length may reach into the (unchecked) trailing length ...
    assert len(compare(head + two + S.epb(b"z" * 20, e, caplen=24) + two, (0, 0, 0))[0]) == 5
    # ... beyond the block the bytes are read, then "bufio: negative count"
    pk, stop, text = compare(head + two + S.epb(b"z" * 20, e, caplen=25) + two, (0, 0, 0))
    assert (len(pk), stop, text) == (2, R.STOP_NEGATIVE, "bufio: negative count")
    # out-of-range interface id, with the reference's text
    pk, stop, text = compare(head + two + S.epb(b"z", e, ifindex=3), (0, 0, 0))
    assert (len(pk), text) == (2, "Interface id 3 not present in section (have only 1 interfaces)")
    pk, stop, text = compare(S.shb(e) + S.spb(b"z", e), (1, 0, 0))
    assert text == "At least one Interface is needed for a packet"
    pk, stop, text = compare(S.shb(e) + S.spb(b"z", e), (0, 0, 0))
    assert (stop, text) == (R.STOP_NO_FIRST, "A section must have an interface before a packet block")
    pk, stop, text = compare(head + two + S.shb(e, bom=0x01020304), (0, 0, 0))
    assert (len(pk), text) == (2, "Wrong byte order value in Section Header")
    pk, stop, text = compare(S.shb(e, struct.pack("<HH", 0, 4) + b"abcd"), (0, 0, 0))
    assert text == "End of Options must be zero length"
    # binary resolution 2^-64 and decimal 10^-64: secondMask 0, the reference divides by it
    for res in (0x80 | 64, 64):
        pk, stop, text = compare(head + two + S.idb(e, opts=S.opt(9, bytes([res]), e) + S.END[e]) + two, (0, 0, 0))
        assert (len(pk), stop) == (2, R.STOP_PANIC) and "the reference panics here" in text
    # convertTime wraps as uint64: offset 2^64 - 1 takes one second off
    f = S.idb(e, opts=S.opt(14, struct.pack("<Q", (1 << 64) - 1), e) + S.END[e])
    pk, _, _ = compare(S.shb(e) + f + S.epb(b"q", e, ts=10 * 10**6 + 5), (0, 0, 0))
    assert (pk[0]["sec"], pk[0]["nsec"]) == (9, 5000)
    # a zero-length option keeps the reference's previous option value
    o = S.opt(3, b"descr", e) + S.opt(2, b"", e) + S.END[e]
    from gopacket_amd import pcapng
    r = pcapng.NewNgReader(S.shb(e) + S.idb(e, opts=o))
    assert r.Interface(0).Name == b"descr"
    r = pcapng.NewNgReader(S.shb(e, S.opt(1, b"", e) + S.END[e]) + S.idb(e))
    assert r.SectionInfo().Comment == bytes(1024)
    with pytest.raises(pcapng.PcapNgError, match="Interface 1 invalid. There are only 1 interfaces"):
        r.Interface(1)
    with pytest.raises(pcapng.PcapNgError, match="Unknown magic a1b2c3d4"):
        pcapng.NewNgReader(struct.pack("<I", 0xA1B2C3D4) + bytes(40))


def test_skip_section_and_mixed_linktype():
    from gopacket_amd import pcapng
    e = "<"
    data = (S.shb(e, S.opt(1, b"one", e) + S.END[e]) + S.idb(e) + S.epb(b"a" * 10, e) +
            S.shb(">", S.opt(1, b"two", ">") + S.END[">"]) + S.idb(">", 0) + S.idb(">", 1) +
            S.epb(b"b" * 11, ">", ifindex=0) + S.epb(b"c" * 12, ">", ifindex=1))
    r = pcapng.NewNgReader(data, pcapng.NgReaderOptions(WantMixedLinkType=True))
    assert (r.LinkType(), r.Resolution(), r.SectionInfo().Comment) == (0, (0, 0), b"one")
    r.SkipSection()
    ref = R.NgReaderRef(data, True)
    assert ref.SkipSection() == (0, None)
    assert (r.SectionInfo().Comment, r.SectionInfo().big_endian, r.pos()) == (b"two", True, ref.position())
    p = r.ReadAll()
    assert list(p.linktype) == [0, 1] and list(p.batch.caplen) == [11, 12] and p.stop == pcapng.STOP_EOF
    with pytest.raises(pcapng.PcapNgError, match="EOF"):
        r.SkipSection()


def test_write_pcapng_round_trip(tmp_path):
    from gopacket_amd import pcap, pcapng, synth
    b = synth.make_mixed(300)
    sec = np.arange(300, dtype=np.int64) * 3 + 1_600_000_000
    nsec = (np.arange(300, dtype=np.uint32) * 999_983) % 1_000_000_000
    for be in (False, True):
        raw = pcapng.write_pcapng(b, snaplen=65535, ts_sec=sec, ts_nsec=nsec, big_endian=be)
        p = pcapng.parse_pcapng(raw)
        assert (p.batch.n, p.stop, p.err) == (300, pcapng.STOP_EOF, None)
        assert all(p.batch.packet(i) == b.packet(i) for i in range(300))
        assert np.array_equal(p.ts_sec, sec) and np.array_equal(p.ts_nsec, nsec)
        assert np.array_equal(p.length, b.caplen) and not p.ifindex.any() and (p.linktype == 1).all()
        compare(raw, (False, False, False))
    cap = pcapng.synth_capture_ng(b)
    q = pcapng.NgReader(cap).ReadAll()
    assert q.batch.n == 300 and all(q.batch.packet(i) == b.packet(i) for i in range(300))
    assert q.next_pos == cap.shape[0] - 64 and list(q.ts_nsec[:3]) == [0, 1000, 2000]
    # read_capture picks the reader by the file's magic
    f1, f2 = tmp_path / "a.pcapng", tmp_path / "a.pcap"
    f1.write_bytes(raw)
    f2.write_bytes(pcap.write_pcap(b))
    assert isinstance(pcapng.read_capture(str(f1)), pcapng.PcapNg) and pcapng.read_pcapng(str(f1)).batch.n == 300
    assert isinstance(pcapng.read_capture(str(f2)), pcap.Pcap)


# ---- ABI -------------------------------------------------------------------------------------

def ng_declared_functions():
    src = open(os.path.join(ROOT, "include", "gpd_pcapng.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpd_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_the_pcapng_header():
    from gopacket_amd import _lib, pcapng
    lib = C.CDLL(_lib.LIB_PATH)
    fns = ng_declared_functions()
    assert "gpd_pcapng_open" in fns and "gpd_decode_pcapng" in fns
    assert not [f for f in fns if not hasattr(lib, f)]
    assert set(fns) == set(pcapng.NG_EXPORTS)
    assert not set(fns) & set(_lib.EXPORTS)     # a table of their own
    assert lib.gpd_abi_version() == 10 == _lib.GPD_ABI_VERSION


def test_pcapng_struct_layouts_match_c(tmp_path):
    from gopacket_amd import pcapng
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_pcapng.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gpd_pcapng_opts),'
                    ' offsetof(gpd_pcapng_opts, chunk_bytes), sizeof(gpd_pcapng_str),'
                    ' sizeof(gpd_pcapng_section_info), offsetof(gpd_pcapng_section_info, big_endian),'
                    ' sizeof(gpd_pcapng_iface), offsetof(gpd_pcapng_iface, ts_offset),'
                    ' offsetof(gpd_pcapng_iface, linktype)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert out == [C.sizeof(pcapng.GpdPcapngOpts), pcapng.GpdPcapngOpts.chunk_bytes.offset,
                   C.sizeof(pcapng.GpdPcapngStr), C.sizeof(pcapng.GpdPcapngSectionInfo),
                   pcapng.GpdPcapngSectionInfo.big_endian.offset, C.sizeof(pcapng.GpdPcapngIface),
                   pcapng.GpdPcapngIface.ts_offset.offset, pcapng.GpdPcapngIface.linktype.offset]


def test_decode_refuses_mixed_linktype_and_null():
    from gopacket_amd import pcapng
    lib = pcapng.ng_lib()
    r = pcapng.NewNgReader(S.shb() + S.idb(), pcapng.NgReaderOptions(WantMixedLinkType=True))
    n, stop = C.c_uint64(), C.c_int()
    assert lib.gpd_decode_pcapng(None, r.h, 1, None, C.byref(n), C.byref(stop), 0) == -1
    with pytest.raises(Exception, match="chunk_bytes"):
        pcapng.NewNgReader(S.shb() + S.idb(), pcapng.NgReaderOptions(chunk_bytes=1000))


# ---- the stand-alone host check under the sanitizers -----------------------------------------

def _sanitizer_runtime():
    if not shutil.which("g++") or not shutil.which("gcc"):
        return False
    r = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True)
    return r.returncode == 0 and os.path.isabs(r.stdout.strip())


@pytest.mark.skipif(not _sanitizer_runtime(), reason="the sanitizer runtime (libasan) is not installed")
def test_standalone_host_walk_under_sanitizers(tmp_path):
    """tests/c/ng_walk_host.c + gpd_pcapng.cpp alone (no HIP, no runtime, never loaded into
    Python) under -fsanitize=address,undefined, on the CPU: the fixtures, every truncation of
    three of them, and the fuzz captures that stop the restatement anywhere but at a clean EOF."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
    inc = ["-I", os.path.join(ROOT, "include")]
    exe = tmp_path / "ng_walk_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *san, *inc, "-DGPD_PCAPNG_STANDALONE", "-c",
                    os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_pcapng.cpp"), "-o", str(tmp_path / "ng.o")],
                   check=True)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", *san, *inc, "-c",
                    os.path.join(ROOT, "tests", "c", "ng_walk_host.c"), "-o", str(tmp_path / "main.o")], check=True)
    subprocess.run(["g++", *san, str(tmp_path / "main.o"), str(tmp_path / "ng.o"), "-o", str(exe)], check=True)

    def run(args, files, flags=(False, False, False)):
        letters = "".join(c for c, f in zip("WES", flags) if f) or "-"
        r = subprocess.run([str(exe), *args, "--opts", letters, *map(str, files)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return [l.split() for l in r.stdout.splitlines()]

    def expect(data, flags):
        ok, r0 = opened(data, flags)
        if not ok:
            return 0, r0.stopped[0], 0
        r, pk, stop, _ = restated(data, flags)
        return len(pk), stop, r.position()

    for flags in {flags_of(t) for t in VECTORS["tests"]}:
        files = [os.path.join(GOLDEN, "pcapng", e, n) for e in ("le", "be") for n in VECTORS["files"][e]]
        for path, line in zip(files, run([], files, flags)):
            assert tuple(map(int, line[1:4])) == expect(open(path, "rb").read(), flags), path
    cut = [os.path.join(GOLDEN, "pcapng", e, n + ".pcapng") for e, n in (("le", "test006"), ("be", "test202"),
                                                                          ("le", "test102"))]
    lines = run(["--cut"], cut)
    assert [l[0].endswith("/cut") for l in lines] == [False, True] * 3
    worst = []
    for seed in range(FUZZ_SEEDS):
        data, flags = S.fuzz_capture(seed)
        n, stop, pos = expect(data, flags)
        if stop != R.STOP_EOF:
            worst.append((seed, data, flags, (n, stop, pos)))
    assert len(worst) > 300
    by_flags = {}
    for seed, data, flags, want in worst:
        f = tmp_path / ("fuzz%05d.pcapng" % seed)
        f.write_bytes(data)
        by_flags.setdefault(flags, []).append((f, want))
    for flags, items in by_flags.items():
        for (f, want), line in zip(items, run([], [f for f, _ in items], flags)):
            assert tuple(map(int, line[1:4])) == want, f
    small = tmp_path / "small.pcapng"
    small.write_bytes(small_capture())
    run(["--cut"], [small])
