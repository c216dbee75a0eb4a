"""The TLS record decode (include/gpd_tls.h) on the CPU: the model (tests/tls_ref.py) against the
reference's own TLS tests (tests/golden/tls_vectors.json), the host walker gpd_tls_decode_host
byte for byte against the model, the budget, the ABI and the layouts, the objects `messages()`
builds, and the walker (gopacket_amd/csrc/gpd_tls_walk.h) and the entry points' no-device paths as
stand-alone programs under the host sanitizers."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import pytest

import tls_cases as TC
import tls_ref as R
from conftest import ROOT

VEC = TC.VEC


# ---------------------------------------------------------------- the model against the reference's tests
def test_golden_holds_the_references_tls_tests():
    assert [v["name"] for v in VEC["vectors"]] == [
        "testClientHello", "testServerHello", "testClientKeyExchange", "testNewSessionTicket", "testDoubleAppData",
        "testAlertEncrypted", "testMalformed"]
    assert [v["tls_off"] for v in VEC["vectors"]] == [54, 0, 0, 0, 0, 0, 0]
    assert [len(v["hex"]) // 2 for v in VEC["vectors"]] == [268, 477, 134, 234, 74, 37, 45]
    assert [d["struct"] for d in VEC["decoded"]] == [
        "testClientHelloDecoded", "testClientKeyExchangeDecoded", "testDoubleAppDataDecoded",
        "testAlertEncryptedDecoded"]
    assert sorted(t for d in VEC["decoded"] for t in d["tests"]) == [
        "TestParseTLSAlertEncrypted", "TestParseTLSAppData", "TestParseTLSChangeCipherSpec",
        "TestParseTLSClientHello", "TestTLSClientHelloDecodeFromBytes"]
    assert [e["test"] for e in VEC["errors"]] == ["TestParseTLSMalformed", "TestParseTLSTooShort",
                                                  "TestParseTLSLengthMismatch"]
    mal, dbl = bytes.fromhex(VEC["vectors"][6]["hex"]), bytearray.fromhex(VEC["vectors"][4]["hex"])
    dbl[3:5] = b"\xff\xff"
    assert [bytes.fromhex(e["hex"]) for e in VEC["errors"]] == [mal, mal[0:2], bytes(dbl)]
    # the frame of testClientHello carries its TLS data to port 443
    f = bytes.fromhex(VEC["vectors"][0]["hex"])
    assert f[12:14] == b"\x08\x00" and f[23] == 6 and struct.unpack(">H", f[36:38])[0] == 443 and f[46] >> 4 == 5


@pytest.mark.parametrize("k", range(4))
def test_model_reproduces_every_asserted_value(k):
    d = VEC["decoded"][k]
    data = TC.vector(d["vector"])
    t = R.decode(data)
    assert t.err is None and not t.truncated
    assert t.Contents == data[d["contents_start"]:]
    head = lambda x: {"ContentType": x.ContentType, "Version": x.Version, "Length": x.Length}
    assert [dict(head(x), Message=x.Message) for x in t.ChangeCipherSpec] == d["ChangeCipherSpec"]
    assert [head(x) for x in t.Handshake] == d["Handshake"]
    assert [dict(head(x), Payload=x.Payload) for x in t.AppData] == \
        [dict(r, Payload=data[r["Payload"][0]:r["Payload"][1]]) for r in d["AppData"]]
    assert [dict(head(x), Level=x.Level, Description=x.Description, EncryptedMsg=x.EncryptedMsg) for x in t.Alert] == \
        [dict(r, EncryptedMsg=data[r["EncryptedMsg"][0]:r["EncryptedMsg"][1]]) for r in d["Alert"]]
    # TestTLSClientHelloDecodeFromBytes decodes twice into one object: a second call equals the first
    assert R.records(R.decode(data), len(data))[0].tobytes() == R.records(t, len(data))[0].tobytes()


def test_model_fails_the_three_error_tests_and_decodes_the_other_vectors():
    errs = [R.decode(bytes.fromhex(e["hex"])).err.code for e in VEC["errors"]]
    assert errs == [R.E_UNKNOWN_TYPE, R.E_TOO_SHORT, R.E_LENGTH_MISMATCH]
    for name in ("testServerHello", "testNewSessionTicket"):
        t = R.decode(TC.vector(name))
        assert t.err is None and t.work == 3
    t = R.decode(TC.vector("testNewSessionTicket"))
    assert (len(t.Handshake), len(t.ChangeCipherSpec)) == (2, 1) and t.contents_off == 181


def test_every_reachable_verdict_has_a_case_and_the_others_are_unreachable():
    cases = TC.named_cases()
    seen = {(R.decode(m).err.code if R.decode(m).err else 0) for m in cases.values()}
    assert seen == R.REACHABLE
    want = {"len_0": R.E_TOO_SHORT, "len_4": R.E_TOO_SHORT, "len_5": R.E_LENGTH_MISMATCH, "exact_end": 0,
            "tail_4": R.E_TOO_SHORT, "length0_ccs": R.E_CCS_LENGTH, "length0_alert": R.E_ALERT_SHORT,
            "length0_handshake": 0, "length0_appdata": 0, "alert_len1": R.E_ALERT_SHORT, "alert_len2": 0,
            "alert_len3": 0, "ccs_len2": R.E_CCS_LENGTH, "length_ffff_short": R.E_LENGTH_MISMATCH,
            "length_ffff_full": 0, "type_0": R.E_UNKNOWN_TYPE, "type_19": R.E_UNKNOWN_TYPE,
            "type_24": R.E_UNKNOWN_TYPE, "type_255": R.E_UNKNOWN_TYPE, "type_19_short_body": R.E_UNKNOWN_TYPE,
            "error_after_two": R.E_LENGTH_MISMATCH, "handshake_300": 0}
    for k, v in want.items():
        t = R.decode(cases[k])
        assert (t.err.code if t.err else 0) == v, k
    assert [R.decode(cases[f"ccs_msg{k}"]).ChangeCipherSpec[0].Message for k in (1, 0, 2)] == [1, 255, 255]
    a2, a3 = R.decode(cases["alert_len2"]).Alert[0], R.decode(cases["alert_len3"]).Alert[0]
    assert (a2.Level, a2.Description, a2.EncryptedMsg) == (2, 40, None)
    assert (a3.Level, a3.Description, a3.EncryptedMsg) == (255, 255, b"\x02\x28\x00")
    t = R.decode(cases["error_after_two"])  # the two records before the error stay
    assert (len(t.Handshake), len(t.ChangeCipherSpec), len(t.AppData)) == (1, 1, 0) and t.err_off == 16 and t.work == 3
    t = R.decode(cases["handshake_300"])
    assert len(t.Handshake) == 300 and t.work == 300 and t.contents_off == 1495
    assert len(R.decode(cases["length_ffff_full"]).AppData[0].Payload) == 0xFFFF
    # GPD_TLS_E_APPDATA_LENGTH and the second unknown-type return never come: every 6-byte input
    # whose header passes the first three tests (all types, both length bytes that fit, a body byte)
    from gopacket_amd import tls as T
    n = 0
    for ct, l0, l1, body in itertools.product(range(256), (0, 1, 255), (0, 1, 2, 255), (0, 1, 2, 255)):
        m = bytes([ct, 3, 3, l0, l1, body])
        t = R.decode(m)
        code = t.err.code if t.err else 0
        assert code in R.REACHABLE and code != R.E_APPDATA_LENGTH
        assert int(T.decode_host(m)[0]["verdict"][0]) == code
        n += 1
    assert n == 256 * 48
    assert set(T.ERROR_TEXTS) == set(range(1, 7)) and R.E_APPDATA_LENGTH not in R.REACHABLE


# ---------------------------------------------------------------- the host walker against the model
def _same_as_model(data, max_records=0):
    from gopacket_amd import tls as T
    t = R.decode(data)
    msg, recs, counts = T.decode_host(data, max_records)
    wm, wr = R.records(t, len(data), max_records)
    assert msg.tobytes() == wm.tobytes(), (data[:64].hex(), msg, wm)
    assert recs.tobytes() == wr.tobytes(), (data[:64].hex(), recs, wr)
    deferred = bool(max_records) and t.work > max_records
    assert counts["deferred"] == deferred and counts["msgs"] == 1 and counts["records"] == len(wr)
    if not deferred:
        assert counts["work"] == t.work, data[:64].hex()
    return t


def _bases():
    return [m for _, m in TC.vector_messages()] + list(TC.named_cases().values())


def test_host_walker_equals_the_model_on_vectors_and_cases():
    for m in _bases():
        _same_as_model(m)
    t = _same_as_model(TC.zero_records(2000))
    assert t.err is None and len(t.Handshake) == 2000


def test_host_walker_equals_the_model_on_every_truncation():
    n = 0
    for _, m in TC.vector_messages():
        for k in range(len(m) + 1):
            _same_as_model(m[:k])
            n += 1
    assert n > 1300
    for name, m in TC.named_cases().items():  # (the long ones: around every record boundary)
        ks = range(len(m) + 1) if len(m) <= 64 else sorted({k for b in range(0, len(m), 5) for k in (b, b + 1)} |
                                                              set(range(len(m) - 12, len(m) + 1)))
        for k in ks:
            if k <= len(m):
                _same_as_model(m[:k])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_walker_equals_the_model_on_seeded_mutations(seed):
    """900 mutations in all (byte flips, header rewrites, cuts, spliced records)."""
    seen = set()
    for m in TC.mutations(seed, 300, _bases()):
        t = _same_as_model(m)
        seen.add(t.err.code if t.err else 0)
    assert seen == R.REACHABLE  # the mutations reach every verdict


def test_budget_is_exact_on_the_host():
    """work == max_records decodes, one more record defers; an error inside the budget stays an
    error, a budget passed before the error is deferred."""
    from gopacket_amd import tls as T
    for m in _bases():
        t = R.decode(m)
        msg, _, c = T.decode_host(m, t.work)
        assert int(msg["verdict"][0]) == (t.err.code if t.err else 0) and c["deferred"] == 0
        _same_as_model(m, t.work)
        if t.work > 1:
            msg, recs, c = T.decode_host(m, t.work - 1)
            assert int(msg["verdict"][0]) == R.DEFERRED and c["deferred"] == 1 and len(recs) == 0
            assert not msg["contents_off"][0] and not msg["err_off"][0] and int(msg["data_len"][0]) == len(m)
            _same_as_model(m, t.work - 1)
    for k in (3, 1024):
        assert int(T.decode_host(TC.zero_records(k), k)[0]["verdict"][0]) == 0
        assert int(T.decode_host(TC.zero_records(k + 1), k)[0]["verdict"][0]) == R.DEFERRED
        assert int(T.decode_host(TC.zero_records(k - 1) + TC.rec(99), k)[0]["verdict"][0]) == R.E_UNKNOWN_TYPE
        assert int(T.decode_host(TC.zero_records(k) + TC.rec(99), k)[0]["verdict"][0]) == R.DEFERRED
    assert all(R.decode(m).work <= 1024 for m in _bases())  # none deferred at the default
    # a wire-size payload holds at most 292 records: (1500 - 20 - 20) // 5
    assert (1500 - 40) // 5 == 292 and R.decode(TC.zero_records(292)).work == 292


def test_host_capacity_exact_and_one_short():
    from gopacket_amd import _lib
    from gopacket_amd import tls as T
    m = TC.named_cases()["all_four"]
    msg, recs, c = T.decode_host(m)
    assert c["records"] == 5 == len(recs)
    with pytest.raises(_lib.GpdError) as e:
        T.decode_host(m, 0, 4)
    assert e.value.counts["records"] == 5
    again = T.decode_host(m, 0, 5)
    assert again[1].tobytes() == recs.tobytes() and again[0].tobytes() == msg.tobytes()
    assert list(recs["index_in_kind"]) == [0, 0, 0, 0, 1] and list(recs["content_type"]) == [22, 20, 23, 21, 22]


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib, dns
    from gopacket_amd import tls as T
    header = open(os.path.join(ROOT, "include", "gpd_tls.h")).read()
    assert list(T.TLS_EXPORTS) == ["gpd_tls_decode", "gpd_tls_decode_ranges", "gpd_tls_decode_host"]
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(gpd_tls_[a-z_]+)\s*\(", code))) == sorted(T.TLS_EXPORTS)
    for name in T.TLS_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name not in _lib.EXPORTS and name not in dns.DNS_EXPORTS
    for cite in ("layers/tls.go:118-194", ":131-134", ":146-148", ":158-159", ":152-155", "tls_cipherspec.go:43-46",
                 "tls_alert.go:80-83", "tls_appdata.go:28-30", "layers/ports.go:64-73", "max_records", "unreachable",
                 "GPD_HDR_TP", "TLS record too short", "Unknown TLS record type", "TLS packet length mismatch",
                 "TLS Alert packet too short", "TLS Application Data length mismatch"):
        assert cite in header, cite
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()


def test_lazy_reexport_and_build_lists():
    import gopacket_amd
    from gopacket_amd.build import HEADERS, SOURCES
    assert gopacket_amd.tls.DecodeTLS is not None and "tls" in gopacket_amd.__all__
    assert gopacket_amd.tls.DecodeTLSRanges and gopacket_amd.tls.DecodeTLSStreams
    names = lambda xs: {os.path.basename(x) for x in xs}
    assert "gpd_tls.hip" in names(SOURCES) and {"gpd_tls.h", "gpd_tls_walk.h", "gpd_locate.h"} <= names(HEADERS)
    csrc = os.path.join(ROOT, "gopacket_amd", "csrc")
    src = open(os.path.join(csrc, "gpd_tls.hip")).read()
    # the scans are the shared ones: no scan of its own, no wait on another workgroup
    for used in ("compact_count(", "compact_scan(", "compact_index(", "scan_sum(", "scan_apply(", "locate_payloads<"):
        assert used in src, used
    assert "__shfl" not in src and "atomicCAS" not in src and "while (atomic" not in src
    # one locate step for DNS and TLS, and one set of kernels for the packets and the ranges
    dns_src = open(os.path.join(csrc, "gpd_dns.hip")).read()
    assert "locate_payloads<" in dns_src and "decode_packet<" not in dns_src and "decode_packet<" not in src
    assert "decode_packet<true>" in open(os.path.join(csrc, "gpd_locate.h")).read()
    assert src.count("tls_walk(") == 3  # the device walk (both sinks through it) and the host entry's two
    walk = open(os.path.join(csrc, "gpd_tls_walk.h")).read()
    assert "hip_runtime" not in walk and "template <class Sink>" in walk


def test_struct_layouts_and_constants_match_c(tmp_path):
    from gopacket_amd import tls as T
    fields_m, fields_r = list(R.MSG_DTYPE.names), list(R.REC_DTYPE.names)
    assert T.MSG_DTYPE == R.MSG_DTYPE and T.REC_DTYPE == R.REC_DTYPE
    consts = [("GPD_TLS_OK", 0), ("GPD_TLS_DEFERRED", T.TLS_DEFERRED), ("GPD_TLS_E_COUNT", T.TLS_E_COUNT),
              ("GPD_TLS_MAX_RECORDS_DEFAULT", T.MAX_RECORDS_DEFAULT), ("GPD_TLS_MAX_RECORDS_LIMIT", T.MAX_RECORDS_LIMIT),
              ("GPD_TLS_CHANGE_CIPHER_SPEC", 20), ("GPD_TLS_ALERT", 21), ("GPD_TLS_HANDSHAKE", 22),
              ("GPD_TLS_APPLICATION_DATA", 23), ("GPD_TLS_REC_ENCRYPTED", T.REC_ENCRYPTED), ("GPD_LT_TLS", 140)]
    header = open(os.path.join(ROOT, "include", "gpd_tls.h")).read()
    errs = re.findall(r"#define (GPD_TLS_E_[A-Z0-9_]+) (\d+)u", header)
    assert [int(v) for n, v in errs if n != "GPD_TLS_E_COUNT"] == list(range(1, 7))
    assert [n for n, _ in errs][:6] == ["GPD_TLS_E_TOO_SHORT", "GPD_TLS_E_UNKNOWN_TYPE", "GPD_TLS_E_LENGTH_MISMATCH",
                                        "GPD_TLS_E_CCS_LENGTH", "GPD_TLS_E_ALERT_SHORT", "GPD_TLS_E_APPDATA_LENGTH"]
    assert (T.MAX_RECORDS_DEFAULT, T.MAX_RECORDS_LIMIT, T.TLS_DEFERRED) == (1024, 1 << 20, 255)
    assert (T.TLS_E_TOO_SHORT, T.TLS_E_UNKNOWN_TYPE, T.TLS_E_LENGTH_MISMATCH, T.TLS_E_CCS_LENGTH, T.TLS_E_ALERT_SHORT,
            T.TLS_E_APPDATA_LENGTH) == (R.E_TOO_SHORT, R.E_UNKNOWN_TYPE, R.E_LENGTH_MISMATCH, R.E_CCS_LENGTH,
                                        R.E_ALERT_SHORT, R.E_APPDATA_LENGTH)
    exprs = (["sizeof(gpd_tls_msg)", "sizeof(gpd_tls_rec)", "sizeof(gpd_tls_config)", "sizeof(gpd_tls_out)",
              "sizeof(gpd_tls_counts)", "sizeof(gpd_tls_ranges)"] + [f"offsetof(gpd_tls_msg, {f})" for f in fields_m] +
             [f"offsetof(gpd_tls_rec, {f})" for f in fields_r] + [f"(size_t){n}" for n, _ in consts])
    want = ([48, 16, 8, 32, 32, 40] + [R.MSG_DTYPE.fields[f][1] for f in fields_m] +
            [R.REC_DTYPE.fields[f][1] for f in fields_r] + [v for _, v in consts])
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_tls.h"\nint main(void){' +
                    "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == want
    assert (C.sizeof(T.GpdTlsConfig), C.sizeof(T.GpdTlsOut), C.sizeof(T.GpdTlsCounts), C.sizeof(T.GpdTlsRanges)) == \
        (8, 32, 32, 40)
    assert T.GpdTlsOut.cap_recs.offset == 24 and T.GpdTlsCounts.work.offset == 24 and T.GpdTlsRanges.n.offset == 32
    # the error texts are the model's (the reference's), code by code
    assert T.ERROR_TEXTS == R.TEXTS and T.error_text(3) == "TLS packet length mismatch"
    comp = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_compact.h")).read()
    assert T.COMPACT_BLOCK == int(re.search(r"kCompactBlock = (\d+);", comp).group(1))
    assert f"c0 += {T.SCAN_ROUND}u" in comp
    # the String() functions
    assert [T.TLSType.String(k) for k in (20, 21, 22, 23, 19, 255)] == \
        ["Change Cipher Spec", "Alert", "Handshake", "Application Data", "Unknown", "Unknown"]
    assert [T.TLSVersion.String(k) for k in (0x0200, 0x0300, 0x0301, 0x0302, 0x0303, 0x0304, 0x0305)] == \
        ["SSL 2.0", "SSL 3.0", "TLS 1.0", "TLS 1.1", "TLS 1.2", "TLS 1.3", "Unknown"]
    assert [T.TLSAlertLevel.String(k) for k in (1, 2, 0, 255)] == ["Warning", "Fatal", "Unknown(0)", "Unknown(255)"]
    assert [T.TLSAlertDescr.String(k) for k in (0, 40, 110, 255)] == \
        ["close_notify", "handshake_failure", "unsupported_extension", "Unknown"]
    assert len(T.TLS_ALERT_DESCR_NAMES) == 25
    # the ports that reach the stop type (layers/ports.go:64-73)
    from gopacket_amd import layers as L
    assert L.LayerTypeTLS == 140


# ---------------------------------------------------------------- the objects
def test_materialised_objects_equal_the_models():
    from gopacket_amd import tls as T
    for m in _bases() + TC.mutations(9, 400, _bases()):
        TC.same_object(T.decode_bytes(m), R.decode(m))
    t = T.decode_bytes(TC.vector("testClientKeyExchange"))
    assert t.err is None and t.Contents == TC.vector("testClientKeyExchange")[81:]
    assert [(x.ContentType, x.Version, x.Length) for x in t.Handshake] == [(22, 0x0301, 70), (22, 0x0301, 48)]
    assert t.ChangeCipherSpec[0].Message == T.TLSChangecipherspecMessage
    t = T.decode_bytes(TC.named_cases()["error_after_two"])
    assert t.err.Error() == "TLS packet length mismatch" and t.err.code == 3 and t.truncated
    assert len(t.Handshake) == 1 and len(t.ChangeCipherSpec) == 1
    t = T.decode_bytes(TC.vector("testAlertEncrypted"))
    assert t.Alert[0].EncryptedMsg == TC.vector("testAlertEncrypted")[5:] and t.Alert[0].Level == 255
    with pytest.raises(ValueError):
        T.materialize(T.decode_host(TC.zero_records(3), 2)[0][0], [], b"")


# ---------------------------------------------------------------- the walker and the entry points, sanitized
@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tls") / "tls_walk_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "tls_walk_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("max_records", [0, 2])
def test_walker_under_host_sanitizers_equals_the_model(walk_host, tmp_path, max_records):
    """tests/c/tls_walk_host.cpp: both sinks over the vectors, every truncation of them, the cases
    and seeded mutations, each message in a heap block of exactly its length, with an exactly-sized
    and a one-short output array, under AddressSanitizer and UBSan; its lines against the model."""
    bases = _bases()
    vecs = [m for _, m in TC.vector_messages()]
    msgs = bases + [m[:k] for m in vecs for k in range(len(m))] + TC.mutations(11, 600, bases) + \
        [TC.zero_records(2000), b""]
    f = tmp_path / "msgs.bin"
    with open(f, "wb") as fh:
        fh.write(struct.pack("<I", len(msgs)))
        for m in msgs:
            fh.write(struct.pack("<I", len(m)) + m)
    r = subprocess.run([walk_host, str(f), str(max_records)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(msgs)
    hx = lambda b: b.hex() if len(b) else "-"
    deferred = 0
    for m, line in zip(msgs, lines):
        t = R.decode(m)
        wm, wr = R.records(t, len(m), max_records)
        got = line.split()
        assert got[:2] == [hx(wm.tobytes()), hx(wr.tobytes())], m[:64].hex()
        if max_records and t.work > max_records:
            deferred += 1
        else:
            assert int(got[2]) == t.work
    assert (deferred > 100) == bool(max_records)  # the budget of 2 defers the three-record flights


def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/tls_errpath.cpp: a stand-alone program (its own main, the context stubbed) linked
    with gpd_tls.hip, host code built with AddressSanitizer and UBSan, run on the CPU against every
    path of gpd_tls_decode and gpd_tls_decode_ranges that returns before a device is needed, and
    gpd_tls_decode_host."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "tls_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "tls_errpath.cpp"),
                    os.path.join(CSRC, "gpd_tls.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_no_tls_kernel_uses_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage over gpd_tls.hip: every kernel's ScratchSize is 0."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    r = subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-c", os.path.join(CSRC, "gpd_tls.hip"), "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    # count, scan, index, scan2, locate x2 (page tables or not), and size, sum, apply, emit x2 (packets, ranges)
    assert len(names) == len(scratch) == 14 and set(scratch) == {"0"}, (names, scratch)
    for k in ("tls_count_kernel", "tls_locate_kernel", "tls_size_kernel", "tls_emit_kernel", "tls_apply_kernel"):
        assert any(k in n for n in names), k
