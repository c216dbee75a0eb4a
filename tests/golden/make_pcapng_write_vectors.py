"""Generate tests/golden/pcapng_write_vectors.json: what pcapgo/ngwrite_test.go feeds
pcapgo.NgWriter in TestNgWriteSimple and TestNgWriteComplex and what it expects to read back
(DATA only).  Reads a checkout of google/gopacket as text:
    python tests/golden/make_pcapng_write_vectors.py <path to google/gopacket>

The reference holds no byte literals for the writer: both tests write a stream and read it back
with NgReader (ngRunFileReadTest), so the parity these vectors give is by round trip and the
bytes are unpinned.  The expectations are recorded after the test's own adjustments
(ngwrite_test.go:204-210): every interface reads back with resolution 9, and interface 1, which
has a TimestampOffset of 100 the writer does not subtract, reads back 100 s later.
"""
import json
import os
import re
import sys

REF = sys.argv[1]
OUT = os.path.dirname(os.path.abspath(__file__))
F, FR, FW = "pcapgo/ngwrite_test.go", "pcapgo/ngread_test.go", "pcapgo/ngwrite.go"
SRC = open(os.path.join(REF, F)).read()


def line_of(path, anchor):
    s = open(os.path.join(REF, path)).read()
    return s[:s.index(anchor)].count("\n") + 1


def braces(text, start):
    """The text between the brace at `start` and its partner."""
    depth, k = 1, start + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
    return text[start + 1:k - 1]


def items(body):
    """The top-level {...} items of a composite literal's body."""
    out, k = [], 0
    while True:
        k = body.find("{", k)
        if k < 0:
            return out
        item = braces(body, k)
        out.append(item)
        k += len(item) + 2


def unix_ns(expr):
    """time.Unix(a-b, c) as Unix nanoseconds."""
    sec, nsec = (t.strip() for t in expr.split(","))
    parts = [int(x) for x in sec.split("-")]
    return (parts[0] - sum(parts[1:])) * 1000000000 + int(nsec)


def strings(text):
    return {k: v for k, v in re.findall(r"(\w+):\s+\"([^\"]*)\"", text)}


def ints(text):
    return {k: int(v) for k, v in re.findall(r"(\w+):\s+(\d+),", text)}


def times(text):
    return {k: unix_ns(v) for k, v in re.findall(r"(\w+):\s+time\.Unix\(([^)]*)\)", text)}


def literal_after(text, anchor):
    i = text.index(anchor)
    return braces(text, text.index("{", i + len(anchor) - 1))


# ngPacketSource (ngread_test.go): hex strings
rsrc = open(os.path.join(REF, FR)).read()
packet_source = re.findall(r"ngMustDecode\(\"([0-9a-f]+)\"\)", literal_after(rsrc, "var ngPacketSource = [...][]byte{"))
assert len(packet_source) == 5

# the defaults NewNgWriter uses (ngwrite.go:28-42); runtime.GOARCH / runtime.GOOS are the platform's
wsrc = open(os.path.join(REF, FW)).read()
def_section = strings(literal_after(wsrc, "var DefaultNgWriterOptions = NgWriterOptions{"))
def_iface = literal_after(wsrc, "var DefaultNgInterface = NgInterface{")
assert def_section == {"Application": "gopacket"} and "runtime.GOARCH" in wsrc and "runtime.GOOS" in def_iface


def iface(text, stats_text):
    s, n = strings(text), ints(text)
    # a field the literal leaves out has Go's zero value: the zero time (None), 0 for a counter
    st = {"LastUpdate": None, "StartTime": None, "EndTime": None, "PacketsReceived": 0, "PacketsDropped": 0}
    st.update(times(stats_text))
    st.update(ints(stats_text))
    return {"Name": s.get("Name", ""), "Comment": s.get("Comment", ""), "Description": s.get("Description", ""),
            "Filter": s.get("Filter", ""), "OS": s.get("OS", ""), "LinkType": 1,  # layers.LinkTypeEthernet
            "TimestampResolution": n.get("TimestampResolution", 0), "TimestampOffset": n.get("TimestampOffset", 0),
            "SnapLength": n.get("SnapLength", 0), "Statistics": st}


def packets(body):
    out = []
    for item in items(body):
        m = re.search(r"data:\s+ngPacketSource\[(\d+)\](?:\[:(\d+)\])?", item)
        src, cut = int(m.group(1)), m.group(2)
        full = bytes.fromhex(packet_source[src])
        data = full[:int(cut)] if cut else full
        ci = braces(item, item.index("{", item.index("ci:")))
        cap = re.search(r"CaptureLength:\s+(\d+|len)", ci).group(1)
        out.append({"source": src, "data": data.hex(), "ts_ns": times(ci)["Timestamp"], "Length": len(full),
                    "CaptureLength": len(data) if cap == "len" else int(cap),
                    "InterfaceIndex": ints(ci)["InterfaceIndex"]})
        assert out[-1]["CaptureLength"] == len(data)
    return out


simple_fn = SRC[SRC.index("func TestNgWriteSimple("):SRC.index("func TestNgWriteComplex(")]
complex_fn = SRC[SRC.index("func TestNgWriteComplex("):SRC.index("type ngDevNull")]

# TestNgWriteSimple: NewNgWriter(buffer, LinkTypeEthernet), one packet at time.Unix(0, 0)
assert "time.Unix(0, 0)" in simple_fn and "ngPacketSource[0]" in simple_fn
simple = {
    "source": f"{F}:{line_of(F, 'func TestNgWriteSimple(')}",
    "linktype": 1,
    "section": {"Hardware": "amd64", "OS": "linux", "Application": "gopacket", "Comment": ""},
    "interfaces": [{"Name": "intf0", "Comment": "", "Description": "", "Filter": "", "OS": "linux", "LinkType": 1,
                    "TimestampResolution": 9, "TimestampOffset": 0, "SnapLength": 0}],
    "packets": [{"source": 0, "data": packet_source[0], "ts_ns": 0, "Length": len(packet_source[0]) // 2,
                 "CaptureLength": len(packet_source[0]) // 2, "InterfaceIndex": 0}],
}
simple["expect"] = {"interfaces": simple["interfaces"], "packets": simple["packets"]}

# TestNgWriteComplex
sect = literal_after(complex_fn, "sectionInfo: NgSectionInfo{")
iface_body = literal_after(complex_fn, "ifaces: []NgInterface{")
ifaces = []
for item in items(iface_body):
    k = item.index("Statistics: NgInterfaceStatistics{")
    stats = braces(item, item.index("{", k))
    ifaces.append(iface(item[:k], stats))
pk = packets(literal_after(complex_fn, "packets: []ngFileReadTestPacket{"))
assert len(ifaces) == 2 and len(pk) == 5
# the call order of the test body
calls = [c for c in re.findall(r"w\.(WritePacket\(packets\[\d\]|AddInterface\(test\.sections\[0\]\.ifaces\[\d\]|"
                               r"WriteInterfaceStats\(\d)", complex_fn)]
order = [["packet" if c.startswith("WritePacket") else "interface" if c.startswith("AddInterface") else "stats",
          int(re.search(r"(\d)\]?$", c).group(1))] for c in calls]
assert "TimestampResolution = 9" in complex_fn and "Add(100 * time.Second)" in complex_fn
expect_ifaces = [dict({k: v for k, v in i.items() if k != "Statistics"}, TimestampResolution=9) for i in ifaces]
expect_packets = [dict(p, ts_ns=p["ts_ns"] + (100 * 1000000000 if p["InterfaceIndex"] == 1 else 0)) for p in pk]
s = strings(sect)
complex_ = {
    "source": f"{F}:{line_of(F, 'func TestNgWriteComplex(')}",
    "linktype": 1,
    "section": {"Hardware": s.get("Hardware", ""), "OS": s.get("OS", ""), "Application": s.get("Application", ""),
                "Comment": s.get("Comment", "")},
    "interfaces": ifaces,   # ifaces[0] goes to NewNgWriterInterface
    "packets": pk,
    "order": order,
    "expect": {"interfaces": expect_ifaces, "packets": expect_packets,
               "adjustments": f"{F}:{line_of(F, '// writer fixes resolution to 9')}-"
                              f"{line_of(F, 'test.packets[1].ci.Timestamp = ')}"},
}

vectors = {"parity": "by round trip, bytes unpinned",
           "packet_source": f"{FR}:{line_of(FR, 'var ngPacketSource')}",
           "simple": simple, "complex": complex_}
json.dump(vectors, open(os.path.join(OUT, "pcapng_write_vectors.json"), "w"), indent=1)
print("pcapng_write_vectors.json")
