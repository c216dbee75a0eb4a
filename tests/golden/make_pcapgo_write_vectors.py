"""Generate tests/golden/pcapgo_write_vectors.json: the byte literals pcapgo/write_test.go expects
from pcapgo.Writer and the CaptureInfos its tests feed it (DATA only).  Reads a checkout of
google/gopacket as text:
    python tests/golden/make_pcapgo_write_vectors.py <path to google/gopacket>
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

REF = sys.argv[1]
MG.REF = REF
OUT = os.path.dirname(os.path.abspath(__file__))
F = "pcapgo/write_test.go"


def src(fn):
    return f"{F}:{MG.line_of(F, 'func ' + fn + '(')}"


vectors = {
    # w.WriteFileHeader(0x1234, 0x56) through NewWriterNanos / NewWriter
    "headers": [
        {"name": "TestWriteHeaderNanos", "source": src("TestWriteHeaderNanos"), "nanos": True,
         "snaplen": 0x1234, "linktype": 0x56, "hex": MG.go_bytes_at(F, "func TestWriteHeaderNanos(").hex()},
        {"name": "TestWriteHeader", "source": src("TestWriteHeader"), "nanos": False,
         "snaplen": 0x1234, "linktype": 0x56, "hex": MG.go_bytes_at(F, "func TestWriteHeader(").hex()},
    ],
    # CaptureInfo{time.Unix(0x01020304, 0xAA*1000), Length 0xABCD, CaptureLength 10}, data 9..0
    "packet": {"name": "TestWritePacket", "source": src("TestWritePacket"),
               "ts_ns": 0x01020304 * 1_000_000_000 + 0xAA * 1000, "length": 0xABCD, "caplen": 10,
               "data": bytes(range(9, -1, -1)).hex(),
               "hex": MG.go_bytes_at(F, "w.WritePacket(ci, data)").hex()},
    # TestCaptureInfoErrors: data {1, 2, 3, 4}, time.Unix(0, 0); both must be rejected
    "rejected": {"name": "TestCaptureInfoErrors", "source": src("TestCaptureInfoErrors"),
                 "data": "01020304", "ts_ns": 0,
                 "infos": [{"length": 5, "caplen": 5,
                            "error": "capture length 5 does not match data length 4"},
                           {"length": 3, "caplen": 4, "error": None}]},
}
assert len(bytes.fromhex(vectors["packet"]["hex"])) == 26
assert all(len(bytes.fromhex(h["hex"])) == 24 for h in vectors["headers"])
json.dump(vectors, open(os.path.join(OUT, "pcapgo_write_vectors.json"), "w"), indent=1)
print("pcapgo_write_vectors.json")
