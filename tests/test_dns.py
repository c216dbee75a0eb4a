"""The DNS decode (include/gpd_dns.h) on the CPU: the model (tests/dns_ref.py) against the
reference's own DNS tests (tests/golden/dns_vectors.json) and test_dns.pcap, the host walker
gpd_dns_decode_host byte for byte against the model, the ABI and the layouts, the objects
`messages()` builds, and the walker (gopacket_amd/csrc/gpd_dns_walk.h) and the entry points'
no-device paths as stand-alone programs under the host sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import dns_cases as DC
import dns_ref as R
from conftest import ROOT

VEC = DC.VEC


def _msg(v):
    f = bytes.fromhex(v["frame_hex"])
    return f[v["dns_off"]:v["dns_off"] + v["dns_len"]]


# ---------------------------------------------------------------- the model against the reference's tests
def test_golden_holds_the_references_dns_tests():
    assert [v["test"] for v in VEC["vectors"]] == [
        "TestPacketDNSNilRdata", "TestPacketDNSRegression", "TestParseDNSTypeTXT", "TestParseDNSBadVers",
        "TestParseDNSBadCookie", "TestParseDNSTypeURI", "TestParseDNSTypeOPT", "TestDNSMalformedPacket",
        "TestDNSMalformedPacket2", "TestBlankNameRootQuery", "TestAnotherMalformedDNS", "TestMalformedDNSAgain",
        "TestMalformedDNSOhGodMakeItStop", "TestMalformedDNSOPT", "TestPacketDNSPanic7"]
    assert len(VEC["fuzz"]) == 4
    assert sum(v["asserts"]["err"] is not None for v in VEC["vectors"]) == 7


@pytest.mark.parametrize("k", range(15))
def test_model_reproduces_every_asserted_value(k):
    v = VEC["vectors"][k]
    a = v["asserts"]
    d = R.decode(_msg(v))
    if a["err"] is None:
        assert d.err is None
    else:
        assert d.err is not None and a["err"] in str(d.err)
    for key, lst in (("questions", d.Questions), ("answers", d.Answers), ("additionals", d.Additionals)):
        if key in a:
            assert len(lst) == a[key], key
    if "response_code" in a:
        assert d.ResponseCode == a["response_code"]
    if "answer0_txts" in a:
        assert [t.decode() for t in d.Answers[0].TXTs] == a["answer0_txts"]
    if "answer0_uri" in a:
        u = d.Answers[0].URI
        assert (u["Target"].decode(), u["Priority"], u["Weight"]) == \
            (a["answer0_uri"]["target"], a["answer0_uri"]["priority"], a["answer0_uri"]["weight"])
    if "additional0_opts" in a:
        assert len(d.Additionals[0].OPT or []) == a["additional0_opts"]
    if "additional0_opt0" in a:
        code, data = d.Additionals[0].OPT[0]
        assert (code, data.hex()) == (a["additional0_opt0"]["code"], a["additional0_opt0"]["data_hex"])
    assert d.work < 500  # no golden vector comes near the default budget


def test_model_decodes_the_fuzz_corpus_and_the_capture():
    for f in VEC["fuzz"]:
        d = R.decode(bytes.fromhex(f["hex"]))
        assert d.err is not None and d.work < 500  # (each is a cut message)
    from gopacket_amd.pcap import read_pcap
    pc = read_pcap(os.path.join(ROOT, "tests", "golden", "test_dns.pcap"))
    assert pc.batch.n == 10
    names = set()
    for i in range(pc.batch.n):
        p = pc.batch.packet(i)
        assert p[12:14] == b"\x08\x00" and p[23] == 17 and 53 in struct.unpack(">HH", p[34:38])
        d = R.decode(p[42:42 + struct.unpack(">H", p[38:40])[0] - 8])
        assert d.err is None and d.QDCount == 1 and not d.QR
        # by the definition: the question, its decodeName call, an iteration a label, the name's
        # bytes with every dot; an OPT additional adds its record and its call on the root name
        nm = d.Questions[0].Name
        assert d.work == 2 + nm.count(b".") + 1 + len(nm) + 1 + 2 * len(d.Additionals)
        assert d.work <= 26
        names.add(nm)
    assert len(names) == 10 and b"picslife.ru" in names


def test_every_reachable_error_has_a_case():
    seen = {(R.decode(m).err.code if R.decode(m).err else 0) for m in DC.named_cases().values()}
    assert seen == R.REACHABLE
    assert R.decode(DC.named_cases()["empty_by_pointer"]).Questions[0].Name == b""
    assert len(R.decode(DC.named_cases()["two_levels_500"]).Questions[0].Name) == 499
    assert R.decode(DC.named_cases()["opt_rcode"]).ResponseCode == 0x63  # 3 | 0x20 | 0x40
    assert R.decode(DC.named_cases()["opt_in_answers"]).ResponseCode == 0
    assert 100 <= len(DC.compressed_response()) <= 130


# ---------------------------------------------------------------- the host walker against the model
def _same_as_model(data, max_work=0):
    from gopacket_amd import dns as D
    d = R.decode(data)
    msg, ents, names, counts = D.decode_host(data, max_work)
    wm, we, wn = R.records(d, len(data), max_work)
    assert msg.tobytes() == wm.tobytes(), (data.hex(), msg, wm)
    assert ents.tobytes() == we.tobytes(), (data.hex(), ents, we)
    assert names == wn, data.hex()
    deferred = bool(max_work) and d.work > max_work
    assert counts["deferred"] == deferred and counts["msgs"] == 1
    if not deferred:
        assert counts["work"] == d.work, data.hex()
    return d


def _bases():
    return [m for _, m in DC.vector_messages()] + list(DC.named_cases().values())


def test_host_walker_equals_the_model_on_vectors_and_cases():
    for m in _bases():
        _same_as_model(m)
    d = _same_as_model(DC.bomb())
    assert d.err is None and len(d.Answers) == 400 and d.work > 200000


def test_host_walker_equals_the_model_on_every_truncation():
    n = 0
    for m in _bases():
        for k in range(len(m)):
            _same_as_model(m[:k])
            n += 1
    assert n > 4000


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_host_walker_equals_the_model_on_seeded_mutations(seed):
    """20,000 mutations in all (byte flips, pointer rewrites, count rewrites, cuts)."""
    seen = set()
    for m in DC.mutations(seed, 5000, _bases()):
        d = _same_as_model(m)
        seen.add(d.err.code if d.err else 0)
    assert len(seen) >= 12  # the mutations reach most error returns


def test_budget_is_exact_on_the_host():
    """work == max_work decodes, max_work + 1 is deferred; an error inside the budget stays an
    error, a budget passed before the error is deferred."""
    from gopacket_amd import dns as D
    for m in _bases() + [DC.pointer_chain(40)]:
        d = R.decode(m)
        if d.work == 0:
            continue
        msg, _, _, c = D.decode_host(m, d.work)
        assert int(msg["verdict"][0]) == (d.err.code if d.err else 0) and c["deferred"] == 0
        _same_as_model(m, d.work)
        if d.work > 1:
            msg, ents, names, c = D.decode_host(m, d.work - 1)
            assert int(msg["verdict"][0]) == R.DEFERRED and c["deferred"] == 1 and len(ents) == 0 and names == b""
            _same_as_model(m, d.work - 1)
    assert all(R.decode(m).work <= 4096 for _, m in DC.vector_messages())  # none deferred at the default
    assert R.decode(DC.named_cases()["self_pointer"]).work == 512
    assert R.decode(DC.pointer_chain(40)).work == 2 * 40 + 7  # 2 a level, and the tail's call, label and question


def test_host_capacities_exact_and_one_short():
    from gopacket_amd import _lib
    from gopacket_amd import dns as D
    m = DC.compressed_response()
    msg, ents, names, c = D.decode_host(m)
    assert (c["entries"], c["name_bytes"]) == (6, len(names)) and len(names) > 60
    for caps in ((5, len(names)), (6, len(names) - 1)):
        with pytest.raises(_lib.GpdError) as e:
            D.decode_host(m, 0, caps)
        assert (e.value.counts["entries"], e.value.counts["name_bytes"]) == (6, len(names))
    again = D.decode_host(m, 0, (6, len(names)))
    assert again[1].tobytes() == ents.tobytes() and again[2] == names


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib, tcptrack
    from gopacket_amd import dns as D
    header = open(os.path.join(ROOT, "include", "gpd_dns.h")).read()
    assert list(D.DNS_EXPORTS) == ["gpd_dns_decode", "gpd_dns_decode_host"]
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(gpd_dns_[a-z_]+)\s*\(", code))) == sorted(D.DNS_EXPORTS)
    for name in D.DNS_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name not in _lib.EXPORTS and name not in tcptrack.TCPTRACK_EXPORTS
    for cite in ("layers/dns.go:304-392", ":538-627", ":710-738", ":906-993", "layers/ports.go:63,106", "udp.go:30-56",
                 "max_work", "unreachable", "not modelled", "GPD_HDR_TP"):
        assert cite in header, cite
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()


def test_lazy_reexport_and_build_lists():
    import gopacket_amd
    from gopacket_amd.build import HEADERS, SOURCES
    assert gopacket_amd.dns.DecodeDNS is not None and "dns" in gopacket_amd.__all__
    names = lambda xs: {os.path.basename(x) for x in xs}
    assert "gpd_dns.hip" in names(SOURCES) and {"gpd_dns.h", "gpd_dns_walk.h"} <= names(HEADERS)
    # the scans are the shared ones: no scan of its own, no wait on another workgroup
    src = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_dns.hip")).read()
    for used in ("compact_count(", "compact_scan(", "compact_index(", "scan_sum(", "scan_apply("):
        assert used in src, used
    assert "__shfl" not in src and "atomicCAS" not in src and "while (atomic" not in src
    walk = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_dns_walk.h")).read()
    assert "hip_runtime" not in walk and "template <class Sink>" in walk


def test_struct_layouts_and_constants_match_c(tmp_path):
    from gopacket_amd import dns as D
    fields_m = [n for n in R.MSG_DTYPE.names]
    fields_e = [n for n in R.ENTRY_DTYPE.names]
    assert D.MSG_DTYPE == R.MSG_DTYPE and D.ENTRY_DTYPE == R.ENTRY_DTYPE
    consts = [("GPD_DNS_OK", 0), ("GPD_DNS_DEFERRED", D.DNS_DEFERRED), ("GPD_DNS_E_COUNT", D.DNS_E_COUNT),
              ("GPD_DNS_MAX_WORK_DEFAULT", D.MAX_WORK_DEFAULT), ("GPD_DNS_MAX_WORK_LIMIT", D.MAX_WORK_LIMIT),
              ("GPD_DNS_SEC_QUESTION", 0), ("GPD_DNS_SEC_ANSWER", 1), ("GPD_DNS_SEC_AUTHORITY", 2),
              ("GPD_DNS_SEC_ADDITIONAL", 3), ("GPD_LT_DNS", 107)]
    header = open(os.path.join(ROOT, "include", "gpd_dns.h")).read()
    errs = re.findall(r"#define (GPD_DNS_E_[A-Z0-9_]+) (\d+)u", header)
    assert [int(v) for n, v in errs if n != "GPD_DNS_E_COUNT"] == list(range(1, 27))
    assert (D.MAX_WORK_DEFAULT, D.MAX_WORK_LIMIT, D.DNS_DEFERRED) == (4096, 65535, 255)
    exprs = (["sizeof(gpd_dns_msg)", "sizeof(gpd_dns_entry)", "sizeof(gpd_dns_config)", "sizeof(gpd_dns_out)",
              "sizeof(gpd_dns_counts)"] + [f"offsetof(gpd_dns_msg, {f})" for f in fields_m] +
             [f"offsetof(gpd_dns_entry, {f})" for f in fields_e] + [f"(size_t){n}" for n, _ in consts])
    want = ([48, 32, 8, 48, 40] + [R.MSG_DTYPE.fields[f][1] for f in fields_m] +
            [R.ENTRY_DTYPE.fields[f][1] for f in fields_e] + [v for _, v in consts])
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_dns.h"\nint main(void){' +
                    "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == want
    assert (C.sizeof(D.GpdDnsConfig), C.sizeof(D.GpdDnsOut), C.sizeof(D.GpdDnsCounts)) == (8, 48, 40)
    assert D.GpdDnsOut.cap_names.offset == 40 and D.GpdDnsCounts.work.offset == 32
    # the error texts are the model's (the reference's), code by code
    assert D.ERROR_FORMATS == R.FORMATS
    comp = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_compact.h")).read()
    assert D.COMPACT_BLOCK == int(re.search(r"kCompactBlock = (\d+);", comp).group(1))
    assert f"c0 += {D.SCAN_ROUND}u" in comp
    from gopacket_amd import _names
    assert (_names.DNS_TYPE_NAMES[28], _names.DNS_CLASS_NAMES[255], _names.DNS_RCODE_NAMES[23],
            _names.DNS_OPCODE_NAMES[5]) == ("AAAA", "Any", "Bad Cookie", "Update")
    assert (D.dns_type_name(41), D.dns_type_name(99), D.dns_class_name(1), D.dns_response_code_name(16),
            D.dns_opcode_name(0), D.dns_opcode_name(3)) == ("OPT", "Unknown", "IN", "Bad OPT Version", "Query", "Unknown")


# ---------------------------------------------------------------- the objects
def test_materialised_objects_equal_the_models():
    from gopacket_amd import dns as D
    for m in _bases() + DC.mutations(9, 1500, _bases()):
        DC.same_object(D.decode_bytes(m), R.decode(m))
    d = D.decode_bytes(DC.named_cases()["label_80"])
    assert d.err.Error() == "qname '0x80' unsupported yet (data=85 index=16)" and d.err.code == 11
    v = next(v for v in VEC["vectors"] if v["test"] == "TestParseDNSTypeOPT")
    d = D.decode_bytes(_msg(v))
    assert d.Additionals[0].OPT[0].Code == 26946 and d.Additionals[0].OPT[0].Data[:7] == b"OpenDNS"


# ---------------------------------------------------------------- the walker and the entry points, sanitized
@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dns") / "dns_walk_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "dns_walk_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("max_work", [0, 40])
def test_walker_under_host_sanitizers_equals_the_model(walk_host, tmp_path, max_work):
    """tests/c/dns_walk_host.cpp: both sinks over the vectors, every truncation of them and seeded
    mutations, each message in a heap block of exactly its length, with exactly-sized and
    one-short output arrays, under AddressSanitizer and UBSan; its lines against the model."""
    bases = _bases()
    msgs = bases + [m[:k] for m in bases for k in range(len(m))] + DC.mutations(11, 3000, bases) + \
        [DC.bomb(), DC.pointer_chain(300), b""]
    f = tmp_path / "msgs.bin"
    with open(f, "wb") as fh:
        fh.write(struct.pack("<I", len(msgs)))
        for m in msgs:
            fh.write(struct.pack("<I", len(m)) + m)
    r = subprocess.run([walk_host, str(f), str(max_work)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(msgs)
    hx = lambda b: b.hex() if len(b) else "-"
    deferred = 0
    for m, line in zip(msgs, lines):
        d = R.decode(m)
        wm, we, wn = R.records(d, len(m), max_work)
        got = line.split()
        assert got[:3] == [hx(wm.tobytes()), hx(we.tobytes()), hx(wn)], m.hex()
        if max_work and d.work > max_work:
            deferred += 1
        else:
            assert int(got[3]) == d.work
    assert (deferred > 1000) == bool(max_work)


def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/dns_errpath.cpp: a stand-alone program (its own main, the context stubbed) linked
    with gpd_dns.hip, host code built with AddressSanitizer and UBSan, run on the CPU against
    every path of gpd_dns_decode that returns before a device is needed and gpd_dns_decode_host."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "dns_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "dns_errpath.cpp"),
                    os.path.join(CSRC, "gpd_dns.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_no_dns_kernel_uses_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage over gpd_dns.hip: every kernel's ScratchSize is 0."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    r = subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-c", os.path.join(CSRC, "gpd_dns.hip"), "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(names) == len(scratch) == 10 and set(scratch) == {"0"}, (names, scratch)
    for k in ("dns_count_kernel", "dns_locate_kernel", "dns_size_kernel", "dns_emit_kernel", "dns_apply_kernel"):
        assert any(k in n for n in names), k
