"""Write tests/golden/dns_vectors.json from the reference's own DNS tests: the byte literals of
layers/dns_test.go with the values its tests assert (transcribed below, test by test, as data)
and the four corpus inputs of layers/testdata/fuzz/FuzzDecodeFromBytes.

    python tests/golden/make_dns_vectors.py [/path/to/gopacket]

The JSON holds data only: packet bytes, where the DNS message lies in them, and expected values.
"""
import ast
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

# test -> (literal, link type of its NewPacket call, what the test asserts)
#   err: None (ErrorLayer() == nil) or the substring its strings.Contains looks for
TESTS = [
    ("TestPacketDNSNilRdata", "testPacketDNSNilRdata", "dns", {"err": None}),
    ("TestPacketDNSRegression", "testPacketDNSRegression", "ethernet", {"err": None}),
    ("TestParseDNSTypeTXT", "testParseDNSTypeTXT", "null",
     {"err": None, "answers": 1, "answer0_txts": ["v=spf1 include:_spf.google.com ~all"]}),
    ("TestParseDNSBadVers", "testParseDNSBadVers", "null",
     {"err": None, "questions": 1, "answers": 0, "additionals": 1, "additional0_opts": 0, "response_code": 16}),
    ("TestParseDNSBadCookie", "testParseDNSBadCookie", "null",
     {"err": None, "questions": 1, "answers": 0, "additionals": 1, "additional0_opts": 1, "response_code": 23}),
    ("TestParseDNSTypeURI", "testParseDNSTypeURI", "null",
     {"err": None, "answers": 1, "answer0_uri": {"target": "http://www.dns.test:8000", "priority": 10, "weight": 5}}),
    ("TestParseDNSTypeOPT", "testParseDNSTypeOPT", "ethernet",
     {"err": None, "questions": 1, "additionals": 1, "additional0_opts": 1,
      "additional0_opt0": {"code": 26946, "data_hex": b"OpenDNS".hex() + "0123456789abcdef"}}),
    ("TestDNSMalformedPacket", "testDNSMalformedPacket", "ethernet", {"err": "invalid index"}),
    ("TestDNSMalformedPacket2", "testDNSMalformedPacket2", "ethernet", {"err": "offset pointer too high"}),
    ("TestBlankNameRootQuery", "testBlankNameRootQuery", "ethernet", {"err": None}),
    ("TestAnotherMalformedDNS", "testAnotherMalformedDNS", "ethernet", {"err": "offset too high"}),
    ("TestMalformedDNSAgain", "testMalformedDNSAgain", "ethernet", {"err": "walked out of range"}),
    ("TestMalformedDNSOhGodMakeItStop", "testMalformedDNSOhGodMakeItStop", "ethernet",
     {"err": "offset pointer too high"}),
    ("TestMalformedDNSOPT", "testMalformedDNSOPT", "ethernet", {"err": "Malformed DNSOPT record"}),
    ("TestPacketDNSPanic7", "testPacketDNSPanic7", "ethernet", {"err": "resource record length exceeds data"}),
]


def literal(src, name):
    m = re.search(r"var %s = \[\]byte\{(.*?)\n\}" % re.escape(name), src, re.S)
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", body))


def dns_span(frame, link):
    """(offset, length) of the bytes the DNS layer is given: through Loopback / Ethernet, IPv4 and
    UDP as the reference's decoders trim them (ip4.go:214-236, udp.go:42-51)."""
    if link == "dns":
        return 0, len(frame)
    off = 4 if link == "null" else 14
    if link == "ethernet":
        assert frame[12:14] == b"\x08\x00"
    ip = frame[off:]
    ihl, length, proto = (ip[0] & 15) * 4, int.from_bytes(ip[2:4], "big"), ip[9]
    assert proto == 17 and length >= 20
    end = off + min(len(ip), length)
    u = off + ihl
    ulen = int.from_bytes(frame[u + 4:u + 6], "big")
    stop = end if ulen == 0 else min(end, u + ulen)
    assert ulen == 0 or ulen >= 8
    return u + 8, stop - (u + 8)


def go_bytes(text):
    """The []byte("...") of a `go test fuzz v1` corpus file."""
    m = re.search(r'\[\]byte\((".*")\)', text, re.S)
    return ast.literal_eval("b" + m.group(1))


def main():
    src = open(os.path.join(REF, "layers", "dns_test.go")).read()
    vectors = []
    for test, name, link, asserts in TESTS:
        assert ("func %s(" % test) in src and name in src
        frame = literal(src, name)
        off, ln = dns_span(frame, link)
        vectors.append({"test": test, "name": name, "link": link, "frame_hex": frame.hex(), "dns_off": off,
                        "dns_len": ln, "asserts": asserts})
    fuzz = []
    d = os.path.join(REF, "layers", "testdata", "fuzz", "FuzzDecodeFromBytes")
    for f in sorted(os.listdir(d)):
        fuzz.append({"name": f, "hex": go_bytes(open(os.path.join(d, f)).read()).hex()})
    assert len(fuzz) == 4
    out = {"source": "layers/dns_test.go, layers/testdata/fuzz/FuzzDecodeFromBytes", "vectors": vectors, "fuzz": fuzz}
    with open(os.path.join(HERE, "dns_vectors.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(len(vectors), "vectors,", len(fuzz), "fuzz inputs")


if __name__ == "__main__":
    main()
