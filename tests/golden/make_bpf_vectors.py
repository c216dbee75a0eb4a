"""Generate tests/golden/bpf_vectors.json: the packet pcap/bpf_test.go feeds (*BPF).Matches and what
its two benchmarks expect of it (DATA only).  Reads a checkout of google/gopacket as text:
    python tests/golden/make_bpf_vectors.py <path to google/gopacket>

The two filter expressions are compiled by libpcap in the reference's run, and libpcap is not
here: the instruction lists below are the 13-instruction IPv4 form of `ip and tcp and port 80`
(Ethernet link, snap length 262144) and the same with the protocol byte compared with 17, and
the return values were worked out by hand from the rules of include/gpd_bpf.h.
"""
import json
import os
import re
import sys

REF = sys.argv[1]
OUT = os.path.dirname(os.path.abspath(__file__))
F = "pcap/bpf_test.go"

src = open(os.path.join(REF, F)).read()
i = src.index("packet  = [...]byte{")
j = src.index("{", i) + 1
body = re.sub(r"//[^\n]*", "", src[j:src.index("}", j)])
packet = bytes(int(t, 16) for t in re.findall(r"0x([0-9a-fA-F]{1,2})", body))
assert len(packet) == 38
line = src[:i].count("\n") + 1
matching = re.search(r'matchingBPFFilter\s*=\s*"([^"]*)"', src).group(1)
nonmatching = re.search(r'nonmatchingBPFFilter\s*=\s*"([^"]*)"', src).group(1)

PORT80 = [[0x28, 0, 0, 12], [0x15, 0, 10, 0x800], [0x30, 0, 0, 23], [0x15, 0, 8, 6], [0x28, 0, 0, 20],
          [0x45, 6, 0, 0x1fff], [0xb1, 0, 0, 14], [0x48, 0, 0, 14], [0x15, 2, 0, 80], [0x48, 0, 0, 16],
          [0x15, 0, 1, 80], [0x06, 0, 0, 262144], [0x06, 0, 0, 0]]
udp = [list(q) for q in PORT80]
udp[3][3] = 0x11

vectors = {
    "packet": {"source": f"{F}:{line}", "hex": packet.hex()},
    "filters": [
        {"name": "BenchmarkPcapMatchingBPFFilter", "expr": matching, "program": PORT80,
         "cases": [{"caplen": 38, "ret": 262144, "matches": True},
                   {"caplen": 37, "ret": 0, "matches": False}]},  # the dst port's second byte is cut off
        {"name": "BenchmarkPcapNonmatchingBPFFilter", "expr": nonmatching, "program": udp,
         "cases": [{"caplen": 38, "ret": 0, "matches": False}]},
    ],
}
json.dump(vectors, open(os.path.join(OUT, "bpf_vectors.json"), "w"), indent=1)
print("bpf_vectors.json")
