"""The DHCP message decode (include/gpd_dhcp.h) on the CPU: the model (tests/dhcp_ref.py) against
the values the reference's own DHCP tests assert (tests/golden/dhcp_vectors.json), the host walker
gpd_dhcp_decode_host byte for byte against the model, the budget, the ABI and the layouts, the
objects `messages()` builds, and the walker (gopacket_amd/csrc/gpd_dhcp_walk.h) and the entry
points' no-device paths as stand-alone programs under the host sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import dhcp_cases as TC
import dhcp_ref as R
from conftest import ROOT

VEC = TC.VEC


# ---------------------------------------------------------------- the model against the reference's tests
def test_golden_holds_the_references_dhcp_tests():
    assert [s["test"] for s in VEC["v4"]] == ["TestDHCPv4EncodeRequest", "TestDHCPv4EncodeResponse"]
    assert [s["test"] for s in VEC["v6"]] == ["TestDHCPv6EncodeRequest", "TestDHCPv6EncodeReply"]
    assert [c["msg"] for c in VEC["option_cases"]] == [
        "DHCPOptPad", "Option with zero length", "Option with maximum length", "Too short option",
        "Too short option when option is not 0 or 255", "Malformed option"]
    # (*DHCPv4).Len(): 240, the options, End; (*DHCPv6).Len(): 4 and the options
    assert [len(s["hex"]) // 2 for s in VEC["v4"]] == [240 + 3 + 13 + 1 + 14 + 1, 240 + 3 + 6 + 1 + 4 * 6 + 1]
    assert [len(s["hex"]) // 2 for s in VEC["v6"]] == [4 + 2 * 18] * 2
    for s in VEC["v4"]:
        b = bytes.fromhex(s["hex"])
        assert b[236:240] == bytes.fromhex("63825363") and b[-1] == 255 and b[2] == 6 and b[28:34] == bytes(s["ClientHWAddr"])
    # the generator reproduces the committed file
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dhcp_vectors", os.path.join(ROOT, "tests", "golden", "make_dhcp_vectors.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    assert [g.wire_v4(s).hex() for s in g.V4] == [s["hex"] for s in VEC["v4"]]
    assert [g.wire_v6(s).hex() for s in g.V6] == [s["hex"] for s in VEC["v6"]]
    assert g.OPTION_CASES == VEC["option_cases"]


@pytest.mark.parametrize("k", range(2))
def test_model_reproduces_every_value_testDHCPEqual_compares(k):
    s = VEC["v4"][k]
    d = R.decode(4, bytes.fromhex(s["hex"]))
    assert d.err is None and not d.truncated and d.Contents == bytes.fromhex(s["hex"])
    for f in ("Operation", "HardwareType", "HardwareLen", "HardwareOpts", "Xid", "Secs", "Flags"):
        assert getattr(d, f) == s[f], f
    for f in ("ClientIP", "YourClientIP", "NextServerIP", "RelayAgentIP", "ClientHWAddr", "ServerName", "File"):
        assert getattr(d, f) == bytes(s[f]), f
    assert len(d.Options) == len(s["Options"])
    for o, w in zip(d.Options, s["Options"]):
        assert o.Type == w["Type"] and (o.Data or b"") == bytes(w["Data"] or [])  # bytes.Equal(nil, empty)
    assert [o.Data for o in d.Options if o.Type == 0] == [None]                   # Pad: nil Data, Length 0
    assert d.work == len(s["Options"]) + 1                                        # End is a decode too


@pytest.mark.parametrize("k", range(2))
def test_model_reproduces_every_value_testDHCPv6Equal_compares(k):
    s = VEC["v6"][k]
    d = R.decode(6, bytes.fromhex(s["hex"]))
    assert d.err is None and d.Contents == bytes.fromhex(s["hex"])
    assert (d.MsgType, d.HopCount, d.LinkAddr, d.PeerAddr) == (s["MsgType"], s["HopCount"], None, None)
    assert d.TransactionID == bytes(s["TransactionID"])
    assert [(o.Code, o.Length, o.Data) for o in d.Options] == [(w["Code"], w["Length"], bytes(w["Data"])) for w in s["Options"]]


def test_model_reproduces_the_six_option_cases():
    for c in VEC["option_cases"]:
        e = R.opt4_decode(R.Opt(), bytes(c["buf"]))
        assert (str(e) if e else None) == c["err"], c["msg"]
    # the fourth (no byte at all) is the return the option loop cannot reach; as the tail of a
    # message the others give the message's verdict
    h = TC.bootp()
    got = [R.decode(4, h + bytes(c["buf"])) for c in VEC["option_cases"]]
    assert [(d.err.code if d.err else 0) for d in got] == [0, 0, 0, 0, R.E_V4_OPT_NO_DATA, R.E_V4_OPT_MALFORMED]
    assert [len(d.Options) for d in got] == [1, 1, 1, 0, 0, 0] and got[2].Options[0].Length == 255
    assert got[3].Contents is None and got[3].work == 0  # len == 240


def test_every_reachable_verdict_has_a_case_and_the_others_are_unreachable():
    cases = TC.named_cases()
    code = lambda vm: (lambda d: d.err.code if d.err else 0)(R.decode(*vm))
    assert {code(vm) for vm in cases.values() if vm[0] == 4} == R.REACHABLE_V4
    assert {code(vm) for vm in cases.values() if vm[0] == 6} == R.REACHABLE_V6
    want = {"v4_len_239": R.E_V4_TOO_SHORT, "v4_len_240": 0, "v4_len_241_end": 0, "v4_len_241_pad": 0,
            "v4_len_241_type": R.E_V4_OPT_NO_DATA, "v4_bad_magic_240": R.E_V4_BAD_MAGIC, "v4_no_end": 0,
            "v4_end_then_garbage": 0, "v4_max_length_cut": R.E_V4_OPT_MALFORMED, "v4_exact_fit": 0,
            "v4_tail_type_after_two": R.E_V4_OPT_NO_DATA, "v4_malformed_after_three": R.E_V4_OPT_MALFORMED,
            "v6_len_3": R.E_V6_TOO_SHORT, "v6_len_4": 0, "v6_relay_12_3": R.E_V6_TOO_SHORT,
            "v6_relay_12_4": R.E_V6_RELAY_SHORT, "v6_relay_13_33": R.E_V6_RELAY_SHORT, "v6_relay_13_34": 0,
            "v6_tail_1": R.E_V6_OPT_NO_DATA, "v6_tail_3": R.E_V6_OPT_NO_DATA, "v6_size_short": R.E_V6_OPT_SIZE,
            "v6_type_14_4": 0}
    for k, v in want.items():
        assert code(cases[k]) == v, k
    dec = lambda k: R.decode(*cases[k])
    # the quirks, one by one
    assert dec("v4_len_239").Options == [] and not dec("v4_len_239").assigned and dec("v4_len_239").truncated
    assert str(dec("v4_len_239").err) == "DHCPv4 length 239 too short"
    d = dec("v4_bad_magic_options")       # the cookie is tested after the fields are assigned
    assert d.assigned and d.Xid == 0xDEADBEEF and d.err_off == 236 and d.Contents is None and not d.truncated
    assert dec("v4_len_240").Contents is None and dec("v4_len_241_end").Contents is not None
    d = dec("v4_pads_only")               # Pad is appended, Length 0, nil Data; no End is OK
    assert [(o.Type, o.Length, o.Data) for o in d.Options] == [(0, 0, None)] * 9 and d.err is None
    d = dec("v4_end_then_garbage")        # End is not appended, what follows is ignored
    assert [o.Type for o in d.Options] == [53] and d.work == 2 and d.err_off == len(cases["v4_end_then_garbage"][1])
    d = dec("v4_malformed_after_three")   # an error keeps the options so far, and no Contents
    assert [o.Type for o in d.Options] == [53, 0, 12] and d.Contents is None and d.err_off == 240 + 3 + 1 + 4
    for hl, n, past in ((0, 240, False), (16, 240, False), (212, 240, False), (213, 240, True), (213, 241, False),
                        (227, 240, True), (227, 254, True), (227, 255, False), (227, 256, False)):
        d = dec(f"v4_hlen_{hl}_{n}")
        assert (d.hw_past_data, len(d.ClientHWAddr), d.HardwareLen, d.err) == (past, min(hl, n - 28), hl, None), (hl, n)
    assert dec("v4_hlen_227_254").Contents is not None and len(dec("v4_hlen_227_254").Options) == 14
    # 28+d.HardwareLen wraps in uint8 from 228 up: the reference panics whatever the length, before
    # ClientHWAddr, ServerName, File and the cookie; the fields before :143 are assigned
    for hl, n in ((228, 240), (228, 241), (228, 256), (255, 240), (255, 241), (255, 282), (255, 283)):
        d = dec(f"v4_hlen_{hl}_{n}")
        assert d.err.code == R.E_V4_HW_PANIC and str(d.err) == f"panic: runtime error: slice bounds out of range [28:{hl - 228}]"
        assert (d.err_off, d.hw_past_data, d.truncated, d.Contents, d.Options, d.work) == (28, False, False, None, [], 0)
        assert d.assigned and d.HardwareLen == hl and d.Xid == 0xDEADBEEF and d.RelayAgentIP == bytes([10, 0, 0, 254])
        assert d.ClientHWAddr is None and d.ServerName is None and d.File is None
    assert dec("v4_bad_magic_hlen_228").err.code == R.E_V4_HW_PANIC
    d = dec("v4_bad_magic_hlen_227")
    assert d.err.code == R.E_V4_BAD_MAGIC and d.hw_past_data and len(d.ClientHWAddr) == 212
    d = dec("v6_relay_12_33")
    assert str(d.err) == "DHCPv6 length 33 too short for message type 12" and d.truncated and d.Contents is not None
    d = dec("v6_relay_13_full")
    assert d.relay and d.HopCount == 3 and d.LinkAddr == bytes(range(16)) and d.PeerAddr == bytes(range(16, 32))
    assert d.TransactionID is None and [o.Code for o in d.Options] == [18, 9, 37] and d.Options[1].Data == TC.SOLICIT
    assert dec("v6_type_11_34").TransactionID == TC.RELAY[1:4]
    # the size error's argument wraps in uint16, the test does not
    assert [str(dec(f"v6_size_{k}").err)[-2:].strip() for k in ("short", "wrap_fffc", "wrap_fffe", "wrap_ffff")] == \
        ["14", "0", "2", "3"]
    d = dec("v6_size_after_two")          # the failing option is not appended
    assert [o.Code for o in d.Options] == [1, 2] and d.err_off == 4 + 5 + 4 and d.work == 3 and d.Contents is not None
    from gopacket_amd import dhcp as T
    assert set(T.ERROR_TEXTS) == set(range(1, 11)) and R.E_V4_OPT_EMPTY not in R.REACHABLE
    # every 241- and 242-byte DHCPv4 tail and every 4..8-byte DHCPv6 message over a few byte values
    h = TC.bootp()
    vals = (0, 1, 2, 3, 4, 5, 12, 13, 119, 254, 255)
    for a in vals:
        for b in (None,) + vals:
            m = h + bytes([a] if b is None else [a, b])
            assert int(T.decode_host(4, m)[0]["verdict"][0]) == code((4, m)) in R.REACHABLE_V4
            for t in (1, 12):
                m6 = bytes([t, 9, 9, 9, 0, a] + ([] if b is None else [0, b]) + [7] * (a % 3))
                assert int(T.decode_host(6, m6)[0]["verdict"][0]) == code((6, m6)) in R.REACHABLE_V6


# ---------------------------------------------------------------- the host walker against the model
def _same_as_model(vm, max_options=0, budgets=False):
    """The host walker against the model for one message; budgets: also with work == max_options
    (decodes) and work == max_options + 1 (deferred)."""
    from gopacket_amd import dhcp as T
    v, data = vm
    d = R.decode(v, data)
    if budgets and d.work >= 1:
        _same_as_model(vm, d.work)
        if d.work > 1:
            _same_as_model(vm, d.work - 1)
    msg, opts, counts = T.decode_host(v, data, max_options)
    wm, wo = R.records(d, len(data), max_options)
    assert msg.tobytes() == wm.tobytes(), (v, data[:64].hex(), len(data), msg, wm)
    assert opts.tobytes() == wo.tobytes(), (v, data[:64].hex(), opts, wo)
    deferred = bool(max_options) and d.work > max_options
    assert counts["deferred"] == deferred and counts["msgs"] == 1 and counts["options"] == len(wo)
    if not deferred:
        assert counts["work"] == d.work, data[:64].hex()
    return d


def _bases():
    return [vm for _, vm in TC.vector_messages()] + list(TC.named_cases().values())


def test_host_walker_equals_the_model_on_vectors_and_cases():
    for vm in _bases():
        _same_as_model(vm, budgets=True)
    d = _same_as_model(TC.pads(5000))
    assert d.err is None and len(d.Options) == 5000
    # each message under the other version's decode
    for v, m in _bases():
        _same_as_model((10 - v, m))


def test_host_walker_equals_the_model_on_every_truncation():
    n = 0
    for v, m in _bases():
        for k in range(len(m) + 1):
            _same_as_model((v, m[:k]), budgets=True)
            n += 1
    assert n == sum(len(m) + 1 for _, m in _bases()) > 12000


@pytest.mark.parametrize("version", [4, 6])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_host_walker_equals_the_model_on_seeded_mutations(seed, version):
    """20,000 mutations per version in all (byte flips, option lengths and types, hlen and the
    message type, cuts, spliced options), each also at work == max_options and one more."""
    seen = set()
    for vm in TC.mutations(seed, 5000, _bases(), version):
        d = _same_as_model(vm, budgets=True)
        seen.add(d.err.code if d.err else 0)
    assert seen == (R.REACHABLE_V4 if version == 4 else R.REACHABLE_V6)  # the mutations reach every verdict


def test_budget_is_exact_on_the_host():
    """work == max_options decodes, one more option defers; an error inside the budget stays an
    error, a budget passed before the error is deferred."""
    from gopacket_amd import dhcp as T
    for v, m in _bases():
        d = R.decode(v, m)
        if d.work >= 1:
            msg, _, c = T.decode_host(v, m, d.work)
            assert int(msg["verdict"][0]) == (d.err.code if d.err else 0) and c["deferred"] == 0
            _same_as_model((v, m), d.work)
            _same_as_model((v, m), d.work + 1)
        if d.work > 1:
            msg, opts, c = T.decode_host(v, m, d.work - 1)
            assert int(msg["verdict"][0]) == R.DEFERRED and c["deferred"] == 1 and len(opts) == 0
            assert not msg["err_off"][0] and not msg["mflags"][0] and not msg["xid"][0] and not msg["op"][0]
            assert int(msg["data_len"][0]) == len(m) and int(msg["version"][0]) == v
            _same_as_model((v, m), d.work - 1)
    verdict = lambda vm, k: int(T.decode_host(vm[0], vm[1], k)[0]["verdict"][0])
    for k in (3, 2048):
        assert verdict(TC.pads(k - 1), k) == 0 and verdict(TC.pads(k), k) == R.DEFERRED   # (End is work too)
        assert verdict(TC.pads(k, end=False), k) == 0
        assert verdict(TC.empty_opts6(k), k) == 0 and verdict(TC.empty_opts6(k + 1), k) == R.DEFERRED
        v4, b4 = TC.pads(k - 1, end=False)
        assert verdict((4, b4 + b"\x77"), k) == R.E_V4_OPT_NO_DATA and verdict((4, b4 + b"\x00\x77"), k) == R.DEFERRED
        v6, b6 = TC.empty_opts6(k - 1)
        assert verdict((6, b6 + b"\x00"), k) == R.E_V6_OPT_NO_DATA and verdict((6, b6 + TC.o6(7) + b"\x00"), k) == R.DEFERRED
    assert all(R.decode(v, m).work <= 2048 for v, m in _bases())  # none deferred at the default
    # a 1472-byte UDP payload holds at most 1232 DHCPv4 options (all Pad) or 367 DHCPv6 options
    assert 1472 - 240 == 1232 and R.decode(4, TC.bootp() + bytes(1232)).work == 1232
    assert (1472 - 4) // 4 == 367 and R.decode(*TC.empty_opts6(367)).work == 367 and len(TC.empty_opts6(367)[1]) == 1472


def test_host_capacity_exact_and_one_short():
    from gopacket_amd import _lib
    from gopacket_amd import dhcp as T
    m = TC.DISCOVER
    msg, opts, c = T.decode_host(4, m)
    assert c["options"] == 8 == len(opts) and c["work"] == 9
    with pytest.raises(_lib.GpdError) as e:
        T.decode_host(4, m, 0, 7)
    assert e.value.counts["options"] == 8
    again = T.decode_host(4, m, 0, 8)
    assert again[1].tobytes() == opts.tobytes() and again[0].tobytes() == msg.tobytes()
    assert list(opts["code"]) == [53, 61, 12, 0, 60, 55, 57, 50] and list(opts["length"]) == [1, 7, 6, 0, 8, 8, 2, 4]
    assert list(opts["off"]) == [240, 243, 252, 260, 261, 271, 281, 285]
    with pytest.raises(_lib.GpdError):
        T.decode_host(5, m)


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib, dns, tls
    from gopacket_amd import dhcp as T
    header = open(os.path.join(ROOT, "include", "gpd_dhcp.h")).read()
    assert list(T.DHCP_EXPORTS) == ["gpd_dhcp_decode", "gpd_dhcp_decode_host"]
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(gpd_dhcp_[a-z_]+)\s*\(", code))) == sorted(T.DHCP_EXPORTS)
    for name in T.DHCP_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name not in _lib.EXPORTS and name not in dns.DNS_EXPORTS and name not in tls.TLS_EXPORTS
    for cite in ("layers/dhcpv4.go:126-179", ":558-578", "layers/dhcpv6.go:89-124", "dhcpv6_options.go:610-621",
                 "layers/ports.go:109-112", "dhcpv4.go:127-130", ":146-148", ":568-570", ":572-574", "dhcpv4.go:559-562",
                 "dhcpv6.go:90-93", ":100-103", "dhcpv6_options.go:611-613", ":616-618", "max_options", "unreachable",
                 "GPD_HDR_TP", "GPD_DHCP_HW_PAST_DATA", "parser.go:302-316"):
        assert cite in header, cite
    for text in R.TEXTS.values():  # the error texts, as the reference writes them
        assert f'"{text}"' in header, text
    assert _lib.lib.gpd_abi_version() == 10
    gpd_h = open(os.path.join(ROOT, "include", "gpd.h")).read()
    assert "#define GPD_ABI_VERSION 10 " in gpd_h and "DHCP" not in gpd_h


def test_lazy_reexport_and_build_lists():
    import gopacket_amd
    from gopacket_amd.build import HEADERS, SOURCES
    assert gopacket_amd.dhcp.DecodeDHCP is not None and "dhcp" in gopacket_amd.__all__
    names = lambda xs: {os.path.basename(x) for x in xs}
    assert "gpd_dhcp.hip" in names(SOURCES) and {"gpd_dhcp.h", "gpd_dhcp_walk.h", "gpd_locate.h"} <= names(HEADERS)
    csrc = os.path.join(ROOT, "gopacket_amd", "csrc")
    src = open(os.path.join(csrc, "gpd_dhcp.hip")).read()
    # the scans, the compaction and the locate step are the shared ones
    for used in ("compact_count(", "compact_scan(", "compact_index(", "scan_sum(", "scan_apply(", "locate_payloads<"):
        assert used in src, used
    walk = open(os.path.join(csrc, "gpd_dhcp_walk.h")).read()
    assert "hip_runtime" not in walk and "template <class Sink>" in walk
    assert "DhcpCountSink" in walk and "DhcpStoreSink" in walk
    go = open(os.path.join(ROOT, "go", "gpdecode", "dhcp.go")).read()
    for name in ("gpd_dhcp_decode", "gpd_dhcp_decode_host", "gpd_dhcp.h", "layers.DHCPv4", "layers.DHCPv6"):
        assert name in go, name


def test_struct_layouts_and_constants_match_c(tmp_path):
    from gopacket_amd import dhcp as T
    from gopacket_amd import layers as L
    fields_m, fields_o = list(R.MSG_DTYPE.names), list(R.OPT_DTYPE.names)
    assert T.MSG_DTYPE == R.MSG_DTYPE and T.OPT_DTYPE == R.OPT_DTYPE
    consts = [("GPD_DHCP_OK", 0), ("GPD_DHCP_DEFERRED", T.DHCP_DEFERRED), ("GPD_DHCP_E_COUNT", T.DHCP_E_COUNT),
              ("GPD_DHCP_MAX_OPTIONS_DEFAULT", T.MAX_OPTIONS_DEFAULT), ("GPD_DHCP_MAX_OPTIONS_LIMIT", T.MAX_OPTIONS_LIMIT),
              ("GPD_DHCP_CONTENTS", T.F_CONTENTS), ("GPD_DHCP_RELAY", T.F_RELAY), ("GPD_DHCP_HW_PAST_DATA", T.F_HW_PAST_DATA),
              ("GPD_DHCP_V4_END", T.DHCPOptEnd), ("GPD_DHCP_V4_PAD", T.DHCPOptPad),
              ("GPD_DHCP_V6_RELAY_FORWARD", T.DHCPv6MsgTypeRelayForward), ("GPD_DHCP_V6_RELAY_REPLY", T.DHCPv6MsgTypeRelayReply),
              ("GPD_LT_DHCPV4", L.LayerTypeDHCPv4), ("GPD_LT_DHCPV6", L.LayerTypeDHCPv6)]
    header = open(os.path.join(ROOT, "include", "gpd_dhcp.h")).read()
    errs = re.findall(r"#define (GPD_DHCP_E_[A-Z0-9_]+) (\d+)u", header)
    assert [int(v) for n, v in errs if n != "GPD_DHCP_E_COUNT"] == list(range(1, 11))
    assert [n for n, _ in errs][:10] == [
        "GPD_DHCP_E_V4_TOO_SHORT", "GPD_DHCP_E_V4_BAD_MAGIC", "GPD_DHCP_E_V4_OPT_NO_DATA", "GPD_DHCP_E_V4_OPT_MALFORMED",
        "GPD_DHCP_E_V6_TOO_SHORT", "GPD_DHCP_E_V6_RELAY_SHORT", "GPD_DHCP_E_V6_OPT_NO_DATA", "GPD_DHCP_E_V6_OPT_SIZE",
        "GPD_DHCP_E_V4_OPT_EMPTY", "GPD_DHCP_E_V4_HW_PANIC"]
    assert (T.MAX_OPTIONS_DEFAULT, T.MAX_OPTIONS_LIMIT, T.DHCP_DEFERRED) == (2048, 65536, 255)
    assert (L.LayerTypeDHCPv4, L.LayerTypeDHCPv6, T.LT_DHCPV4, T.LT_DHCPV6) == (118, 134, 118, 134)
    assert (T.DHCP_E_V4_TOO_SHORT, T.DHCP_E_V4_BAD_MAGIC, T.DHCP_E_V4_OPT_NO_DATA, T.DHCP_E_V4_OPT_MALFORMED,
            T.DHCP_E_V6_TOO_SHORT, T.DHCP_E_V6_RELAY_SHORT, T.DHCP_E_V6_OPT_NO_DATA, T.DHCP_E_V6_OPT_SIZE,
            T.DHCP_E_V4_OPT_EMPTY, T.DHCP_E_V4_HW_PANIC) == (R.E_V4_TOO_SHORT, R.E_V4_BAD_MAGIC, R.E_V4_OPT_NO_DATA, R.E_V4_OPT_MALFORMED,
                                       R.E_V6_TOO_SHORT, R.E_V6_RELAY_SHORT, R.E_V6_OPT_NO_DATA, R.E_V6_OPT_SIZE,
                                       R.E_V4_OPT_EMPTY, R.E_V4_HW_PANIC)
    exprs = (["sizeof(gpd_dhcp_msg)", "sizeof(gpd_dhcp_opt)", "sizeof(gpd_dhcp_config)", "sizeof(gpd_dhcp_out)",
              "sizeof(gpd_dhcp_counts)"] + [f"offsetof(gpd_dhcp_msg, {f})" for f in fields_m] +
             [f"offsetof(gpd_dhcp_opt, {f})" for f in fields_o] + [f"(size_t){n}" for n, _ in consts])
    want = ([48, 8, 8, 32, 32] + [R.MSG_DTYPE.fields[f][1] for f in fields_m] +
            [R.OPT_DTYPE.fields[f][1] for f in fields_o] + [v for _, v in consts])
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_dhcp.h"\nint main(void){' +
                    "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == want
    assert [R.MSG_DTYPE.fields[f][1] for f in fields_m] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 34, 36, 37, 38, 39, 40, 41,
                                                            42, 43, 44]
    assert (C.sizeof(T.GpdDhcpConfig), C.sizeof(T.GpdDhcpOut), C.sizeof(T.GpdDhcpCounts)) == (8, 32, 32)
    assert T.GpdDhcpOut.cap_opts.offset == 24 and T.GpdDhcpCounts.work.offset == 24
    # the error texts are the model's (the reference's), code by code, with their arguments
    assert T.ERROR_TEXTS == R.TEXTS
    assert T.error_text(1, 239) == "DHCPv4 length 239 too short" and T.error_text(2) == "Bad DHCP header"
    assert T.error_text(6, 33, 13) == "DHCPv6 length 33 too short for message type 13"
    assert T.error_text(8, 2) == "dhcpv6 option size < length 2"
    assert T.error_text(10, 27) == "panic: runtime error: slice bounds out of range [28:27]"
    comp = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_compact.h")).read()
    assert T.COMPACT_BLOCK == int(re.search(r"kCompactBlock = (\d+);", comp).group(1))
    assert f"c0 += {T.SCAN_ROUND}u" in comp
    # the ports that reach the two stop types (layers/ports.go:109-112)
    assert [int(L.TABLES.udp_port[p]) for p in (67, 68, 546, 547)] == [118, 118, 134, 134]


# ---------------------------------------------------------------- the objects
def test_materialised_objects_equal_the_models():
    from gopacket_amd import dhcp as T
    bases = _bases()
    for v, m in bases + TC.mutations(9, 400, bases, 4) + TC.mutations(9, 400, bases, 6):
        TC.same_object(T.decode_bytes(v, m), R.decode(v, m))
    s = VEC["v4"][1]
    d = T.decode_bytes(4, bytes.fromhex(s["hex"]))
    assert d.err is None and d.Contents == bytes.fromhex(s["hex"]) and d.Payload is None
    assert (d.Operation, d.HardwareType, d.HardwareLen, d.Xid) == (2, 1, 6, 0x12345678)
    assert d.YourClientIP == bytes([192, 168, 0, 123]) and d.ClientHWAddr == bytes(s["ClientHWAddr"])
    assert [(o.Type, o.Data) for o in d.Options] == [(w["Type"], None if w["Data"] is None else bytes(w["Data"]))
                                                     for w in s["Options"]]
    d = T.decode_bytes(4, TC.named_cases()["v4_malformed_after_three"][1])
    assert d.err.Error() == "Option is malformed" and d.err.code == 4 and not d.truncated and d.Contents is None
    assert [o.Type for o in d.Options] == [53, 0, 12]
    d = T.decode_bytes(4, TC.named_cases()["v4_hlen_227_240"][1])   # the address clipped to data
    assert d.hw_past_data and d.HardwareLen == 227 and len(d.ClientHWAddr) == 212 and d.err is None
    d = T.decode_bytes(4, TC.named_cases()["v4_hlen_255_283"][1])   # 28+255 wraps: the reference panics
    assert d.err.Error() == "panic: runtime error: slice bounds out of range [28:27]" and d.err.code == 10
    assert (d.HardwareLen, d.ClientHWAddr, d.ServerName, d.Contents, d.hw_past_data) == (255, None, None, None, False)
    assert d.ClientIP == bytes([10, 0, 0, 5]) and d.Options == []
    d = T.decode_bytes(6, TC.RELAY)
    assert (d.MsgType, d.HopCount, d.LinkAddr, d.TransactionID) == (12, 3, bytes(range(16)), None)
    assert T.decode_bytes(6, d.Options[1].Data).TransactionID == b"\xab\xcd\xef"   # the nested message, by hand
    d = T.decode_bytes(6, TC.named_cases()["v6_size_wrap_fffe"][1])
    assert str(d.err) == "dhcpv6 option size < length 2" and d.Contents is not None and d.Options == []
    with pytest.raises(ValueError):
        T.materialize(T.decode_host(4, TC.pads(3)[1], 2)[0][0], [], b"")


# ---------------------------------------------------------------- the walker and the entry points, sanitized
@pytest.fixture(scope="module")
def walk_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dhcp") / "dhcp_walk_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "dhcp_walk_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("max_options", [0, 2])
def test_walker_under_host_sanitizers_equals_the_model(walk_host, tmp_path, max_options):
    """tests/c/dhcp_walk_host.cpp: both sinks over the vectors and the cases, every truncation of
    them and seeded mutations, each message in a heap block of exactly its length, with an
    exactly-sized and a one-short output array, under AddressSanitizer and UBSan; its lines against
    the model."""
    bases = _bases()
    msgs = bases + [(v, m[:k]) for v, m in bases if len(m) < 600 for k in range(len(m))] + \
        TC.mutations(11, 1500, bases, 4) + TC.mutations(11, 1500, bases, 6) + [TC.pads(5000), (4, b""), (6, b"")]
    f = tmp_path / "msgs.bin"
    with open(f, "wb") as fh:
        fh.write(struct.pack("<I", len(msgs)))
        for v, m in msgs:
            fh.write(struct.pack("<II", v, len(m)) + m)
    r = subprocess.run([walk_host, str(f), str(max_options)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(msgs)
    hx = lambda b: b.hex() if len(b) else "-"
    deferred = 0
    for (v, m), line in zip(msgs, lines):
        d = R.decode(v, m)
        wm, wo = R.records(d, len(m), max_options)
        got = line.split()
        assert got[:2] == [hx(wm.tobytes()), hx(wo.tobytes())], (v, m[:64].hex(), len(m))
        if max_options and d.work > max_options:
            deferred += 1
        else:
            assert int(got[2]) == d.work
    assert (deferred > 100) == bool(max_options)  # the budget of 2 defers every longer option list


def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/dhcp_errpath.cpp: a stand-alone program (its own main, the context stubbed) linked
    with gpd_dhcp.hip, host code built with AddressSanitizer and UBSan, run on the CPU against every
    path of gpd_dhcp_decode that returns before a device is needed, and gpd_dhcp_decode_host."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "dhcp_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "dhcp_errpath.cpp"),
                    os.path.join(CSRC, "gpd_dhcp.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_no_dhcp_kernel_uses_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage over gpd_dhcp.hip: every kernel's ScratchSize is 0."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    r = subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-c", os.path.join(CSRC, "gpd_dhcp.hip"), "-o", str(tmp_path / "k.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    # count, scan, index, locate x2 (page tables or not), size, sum, scan2, apply, emit
    assert len(names) == len(scratch) == 10 and set(scratch) == {"0"}, (names, scratch)
    for k in ("dhcp_count_kernel", "dhcp_locate_kernel", "dhcp_size_kernel", "dhcp_emit_kernel", "dhcp_apply_kernel"):
        assert any(k in n for n in names), k
