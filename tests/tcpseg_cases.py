"""TEST INFRASTRUCTURE ONLY: what the tcpassembly hand-off's CPU and GPU tests share — the
reference's vectors (tests/golden/tcpassembly_vectors.json) and hand-built packets with the
record fields each must give, written out."""
import json
import os
import struct

import tcpassembly_ref as TA
from conftest import ROOT
from gopacket_amd import synth

ALL = 0xFFF
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "tcpassembly_vectors.json")))
A4, B4 = bytes(VEC["net_flow"]["src"]), bytes(VEC["net_flow"]["dst"])
A6, B6 = bytes(15) + b"\x01", bytes(15) + b"\x02"
ACK, PSH = 0x10, 0x08


def vec_bytes(b) -> bytes:
    return bytes(b["zeros"]) if isinstance(b, dict) else bytes(b)


def vec_want(step):
    return [(vec_bytes(w["bytes"]), w["skip"], w["start"], w["end"]) for w in step["want"]]


def vxlan_around(inner: bytes) -> bytes:
    vx = b"\x08\x00\x00\x00\x00\x00\x2a\x00" + inner
    udp = struct.pack(">HHHH", 40000, 4789, 8 + len(vx), 0) + vx
    ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 20 + len(udp), 9, 0, 64, 17, 0, bytes([10, 0, 0, 1]),
                     bytes([10, 0, 0, 2])) + udp
    return bytes(6) + bytes([2, 0, 0, 0, 0, 2]) + b"\x08\x00" + ip


def hand_built():
    """(frame, caplen or None, expected record fields or None when not handed over)."""
    ts_opt = bytes([1, 1, 8, 10, 0, 0, 0, 1, 0, 0, 0, 2])  # NOP NOP Timestamp
    udp = bytes(6) + bytes([2, 0, 0, 0, 0, 1]) + b"\x08\x00" + struct.pack(
        ">BBHHHBBH4s4s", 0x45, 0, 20 + 8 + 4, 1, 0, 64, 17, 0, A4, B4) + struct.pack(">HHHH", 3000, 3001, 12, 0) + b"abcd"
    f6 = synth.tcp_frame(A6, B6, 1, 2, 77, flags=ACK | PSH, payload=b"six")
    inner = synth.tcp_frame(A4, B4, 1, 2, 900, ack=5, flags=ACK | PSH, payload=b"inner!")
    E = lambda **kw: dict(dict(tcp_off=34, lookup_only=0, ack=0), **kw)
    return [
        # a bare ACK in a frame padded to 60 bytes: the IPv4 Length trims the padding, nothing left
        (synth.tcp_frame(A4, B4, 1, 2, 1000, ack=7, flags=ACK, pad_to=60), None, None),
        # the same frame with SYN: kept, no payload; a SYN is never lookup_only
        (synth.tcp_frame(A4, B4, 1, 2, 1000, flags=TA.SYN, pad_to=60), None,
         E(seq=1000, flags=TA.SYN, payload_off=54, payload_len=0)),
        # FIN and RST without payload: kept, but only to look the connection up
        (synth.tcp_frame(A4, B4, 1, 2, 1001, ack=7, flags=TA.FIN | ACK, pad_to=60), None,
         E(seq=1001, ack=7, flags=TA.FIN | ACK, payload_off=54, payload_len=0, lookup_only=1)),
        (synth.tcp_frame(A4, B4, 1, 2, 1002, flags=TA.RST, pad_to=60), None,
         E(seq=1002, flags=TA.RST, payload_off=54, payload_len=0, lookup_only=1)),
        # payload behind padding: three bytes, not nine
        (synth.tcp_frame(A4, B4, 1, 2, 1003, flags=ACK | PSH, payload=b"xyz", pad_to=60), None,
         E(seq=1003, flags=ACK | PSH, payload_off=54, payload_len=3)),
        # TCP options move the payload
        (synth.tcp_frame(A4, B4, 1, 2, 1006, flags=ACK, payload=b"opts", options=ts_opt), None,
         E(seq=1006, flags=ACK, payload_off=66, payload_len=4)),
        # IPv4 Length 0 (TSO): everything captured is the datagram
        (synth.tcp_frame(A4, B4, 1, 2, 1010, flags=ACK, payload=b"tso-bytes", ip_length=0), None,
         E(seq=1010, flags=ACK, payload_off=54, payload_len=9)),
        # a capture that cuts the segment
        (synth.tcp_frame(A4, B4, 1, 2, 1019, flags=ACK, payload=bytes(100)), 70,
         E(seq=1019, flags=ACK, payload_off=54, payload_len=16)),
        # one 802.1Q tag
        (synth.tcp_frame(A4, B4, 1, 2, 1119, flags=ACK | 0x100, payload=b"v", tags=1), None,
         E(seq=1119, flags=ACK | 0x100, tcp_off=38, payload_off=58, payload_len=1)),
        # IPv6
        (f6, None, E(seq=77, flags=ACK | PSH, tcp_off=54, payload_off=74, payload_len=3)),
        # IPv6 with trailing bytes past the payload length
        (f6 + bytes(7), None, E(seq=77, flags=ACK | PSH, tcp_off=54, payload_off=74, payload_len=3)),
        # VXLAN: the inner segment (outer 14 + 20 + 8 + 8 = 50 bytes in front of the inner frame)
        (vxlan_around(inner), None,
         E(seq=900, ack=5, flags=ACK | PSH, tcp_off=84, payload_off=104, payload_len=6)),
        # DataOffset < 5: the TCP layer fails to decode
        (synth.tcp_frame(A4, B4, 1, 2, 1, flags=TA.SYN, payload=b"bad", doff=4), None, None),
        # UDP
        (udp, None, None),
    ]
