"""Write tests/golden/tls_vectors.json from the reference's own TLS tests: the byte literals of
layers/tls_test.go with the values of its *Decoded structs (transcribed below, struct by struct,
as data, and checked against the file's text) and the inputs of its three error tests.

    python tests/golden/make_tls_vectors.py [/path/to/gopacket]

The JSON holds data only: bytes, where the TLS data lies in them, and expected values.  Slices of
a literal are written as [start, end] into that literal's TLS data.
"""
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

# literal -> offset of the TLS data in it (testClientHello is an Ethernet/IPv4/TCP frame)
LITERALS = [("testClientHello", 54), ("testServerHello", 0), ("testClientKeyExchange", 0), ("testNewSessionTicket", 0),
            ("testDoubleAppData", 0), ("testAlertEncrypted", 0), ("testMalformed", 0)]

hdr = lambda ct, ver, ln: {"ContentType": ct, "Version": ver, "Length": ln}

# struct -> (its literal, the tests that DeepEqual against it, Contents' start in the literal, lists)
DECODED = [
    ("testClientHelloDecoded", "testClientHello", ["TestParseTLSClientHello"], 54,
     {"ChangeCipherSpec": [], "Handshake": [hdr(22, 0x0301, 209)], "AppData": [], "Alert": []}),
    ("testClientKeyExchangeDecoded", "testClientKeyExchange",
     ["TestTLSClientHelloDecodeFromBytes", "TestParseTLSChangeCipherSpec"], 81,
     {"ChangeCipherSpec": [dict(hdr(20, 0x0301, 1), Message=1)],
      "Handshake": [hdr(22, 0x0301, 70), hdr(22, 0x0301, 48)], "AppData": [], "Alert": []}),
    ("testDoubleAppDataDecoded", "testDoubleAppData", ["TestParseTLSAppData"], 37,
     {"ChangeCipherSpec": [], "Handshake": [],
      "AppData": [dict(hdr(23, 0x0301, 32), Payload=[5, 37]), dict(hdr(23, 0x0301, 32), Payload=[42, 74])],
      "Alert": []}),
    ("testAlertEncryptedDecoded", "testAlertEncrypted", ["TestParseTLSAlertEncrypted"], 0,
     {"ChangeCipherSpec": [], "Handshake": [], "AppData": [],
      "Alert": [dict(hdr(21, 0x0303, 32), Level=0xFF, Description=0xFF, EncryptedMsg=[5, 37])]}),
]

# test -> how its input is made from a literal; each asserts ErrorLayer() != nil
ERROR_TESTS = [
    ("TestParseTLSMalformed", "testMalformed", {"slice": None, "set": []}),
    ("TestParseTLSTooShort", "testMalformed", {"slice": [0, 2], "set": []}),
    ("TestParseTLSLengthMismatch", "testDoubleAppData", {"slice": None, "set": [[3, 0xFF], [4, 0xFF]]}),
]


def literal(src, name):
    m = re.search(r"var %s = \[\]byte\{(.*?)\n\}" % re.escape(name), src, re.S)
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return bytes(int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{2})", body))


def struct_text(src, name):
    return re.search(r"var %s = &TLS\{(.*?)\n\}" % re.escape(name), src, re.S).group(1)


def main():
    src = open(os.path.join(REF, "layers", "tls_test.go")).read()
    lits = {name: literal(src, name) for name, _ in LITERALS}
    vectors = [{"name": name, "hex": lits[name].hex(), "tls_off": off} for name, off in LITERALS]
    decoded = []
    assert len(re.findall(r"var \w+Decoded = &TLS\{", src)) == len(DECODED)
    for name, lit, tests, contents, lists in DECODED:
        text = struct_text(src, name)
        # the transcription against the text: Contents' expression and the headers in order
        c = re.search(r"Contents:\s*(\w+)(?:\[(\d+):\])?,", text)
        assert c.group(1) == lit and int(c.group(2) or 0) == contents, name
        heads = [(int(a), int(b, 16), int(n)) for a, b, n in
                 re.findall(r"ContentType:\s*(\d+),\s*Version:\s*0x([0-9a-fA-F]+),\s*Length:\s*(\d+),", text)]
        want = [(r["ContentType"], r["Version"], r["Length"]) for k in ("ChangeCipherSpec", "Handshake", "AppData", "Alert")
                for r in lists[k]]
        assert heads == want, (name, heads, want)
        for t in tests:
            assert re.search(r"func %s\(" % t, src), t
        off = dict(LITERALS)[lit]
        fix = lambda r: {k: ([v[0] - off, v[1] - off] if isinstance(v, list) else v) for k, v in r.items()}
        decoded.append({"struct": name, "vector": lit, "tests": tests, "contents_start": contents - off,
                        **{k: [fix(r) for r in v] for k, v in lists.items()}})
    errors = []
    for test, lit, how in ERROR_TESTS:
        assert re.search(r"func %s\(" % test, src), test
        b = bytearray(lits[lit])
        for i, v in how["set"]:
            b[i] = v
        if how["slice"]:
            b = b[how["slice"][0]:how["slice"][1]]
        errors.append({"test": test, "vector": lit, "slice": how["slice"], "set": how["set"], "hex": bytes(b).hex()})
    out = {"source": "layers/tls_test.go", "vectors": vectors, "decoded": decoded, "errors": errors}
    with open(os.path.join(HERE, "tls_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(len(vectors), "vectors,", len(decoded), "decoded structs,", len(errors), "error tests")


if __name__ == "__main__":
    main()
