"""Writes tests/golden/dhcp_vectors.json: what the reference's own DHCP tests assert, as data.

The reference has no DHCP byte literals: layers/dhcp_test.go and layers/dhcpv6_test.go build a
struct, serialise it, decode the bytes and compare the two structs.  The structs' values are
transcribed here as the expected values, and the wire bytes are built from the wire layout that
SerializeTo writes: RFC 2131 section 2 (the 236-byte BOOTP header, the magic cookie 0x63825363,
then options as type, length, data with a one-byte Pad and a closing End) and RFC 8415 section 8
(msg-type, a 3-byte transaction-id, then options as 16-bit code, 16-bit length, data), with
FixLengths: HardwareLen = len(ClientHWAddr), option lengths = len(Data).

Which fields each reference test compares:
  TestDHCPv4EncodeRequest, TestDHCPv4EncodeResponse (dhcp_test.go:17-68) through testDHCPEqual
    (:122-181): Operation, HardwareType, HardwareLen, HardwareOpts, Xid, Secs, Flags, ClientIP,
    YourClientIP, NextServerIP, RelayAgentIP, ClientHWAddr, ServerName, File, len(Options), and per
    option Type and Data (not Length).
  TestDHCPv6EncodeRequest, TestDHCPv6EncodeReply (dhcpv6_test.go:16-55) through testDHCPv6Equal
    (:58-93): MsgType, HopCount, LinkAddr, PeerAddr, TransactionID, len(Options), and per option
    Code, Length and Data.
  TestDHCPv4DecodeOption (dhcp_test.go:70-120): the error (*DHCPOption).decode returns for six
    buffers, compared by identity with nil, DecOptionNotEnoughData or DecOptionMalformed.

  python tests/golden/make_dhcp_vectors.py
"""
import json
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))

HW = [0x12, 0x34, 0x56, 0x78, 0x9A, 0xBC]
V4 = [
    {"test": "TestDHCPv4EncodeRequest", "Operation": 1, "HardwareType": 1, "HardwareLen": 6, "HardwareOpts": 0,
     "Xid": 0x12345678, "Secs": 0, "Flags": 0, "ClientIP": [0, 0, 0, 0], "YourClientIP": [0, 0, 0, 0],
     "NextServerIP": [0, 0, 0, 0], "RelayAgentIP": [0, 0, 0, 0], "ClientHWAddr": HW, "ServerName": [0] * 64,
     "File": [0] * 128,
     "Options": [{"Type": 53, "Data": [1]}, {"Type": 12, "Data": list(b"example.com")}, {"Type": 0, "Data": None},
                 {"Type": 55, "Data": [1, 28, 2, 3, 15, 6, 119, 12, 44, 26, 121, 42]}]},
    {"test": "TestDHCPv4EncodeResponse", "Operation": 2, "HardwareType": 1, "HardwareLen": 6, "HardwareOpts": 0,
     "Xid": 0x12345678, "Secs": 0, "Flags": 0, "ClientIP": [0, 0, 0, 0], "YourClientIP": [192, 168, 0, 123],
     "NextServerIP": [192, 168, 0, 1], "RelayAgentIP": [0, 0, 0, 0], "ClientHWAddr": HW, "ServerName": [0] * 64,
     "File": [0] * 128,
     "Options": [{"Type": 53, "Data": [2]}, {"Type": 1, "Data": [255, 255, 255, 0]}, {"Type": 0, "Data": None},
                 {"Type": 58, "Data": [0, 0, 0x0E, 0x10]}, {"Type": 59, "Data": [0, 0, 0x0E, 0x10]},
                 {"Type": 51, "Data": [0, 0, 0x0E, 0x10]}, {"Type": 54, "Data": [192, 168, 0, 1]}]},
]

# DHCPv6DUID.Encode of a DUID-LLT: type 1, the hardware type, the time, the link-layer address
CLIENT = [0, 1, 0, 1, 28, 56, 38, 45, 8, 0, 39, 254, 143, 149]
SERVER = [0, 1, 0, 1, 28, 56, 37, 232, 8, 0, 39, 212, 16, 187]
V6 = [
    {"test": "TestDHCPv6EncodeRequest", "MsgType": 3, "HopCount": 0, "LinkAddr": None, "PeerAddr": None,
     "TransactionID": [87, 25, 88],
     "Options": [{"Code": 1, "Length": 14, "Data": CLIENT}, {"Code": 2, "Length": 14, "Data": SERVER}]},
    {"test": "TestDHCPv6EncodeReply", "MsgType": 7, "HopCount": 0, "LinkAddr": None, "PeerAddr": None,
     "TransactionID": [87, 25, 88],
     "Options": [{"Code": 1, "Length": 14, "Data": CLIENT}, {"Code": 2, "Length": 14, "Data": SERVER}]},
]

# TestDHCPv4DecodeOption: err is null (nil), "Not enough data to decode" or "Option is malformed"
OPTION_CASES = [
    {"msg": "DHCPOptPad", "buf": [0], "err": None},
    {"msg": "Option with zero length", "buf": [119, 0], "err": None},
    {"msg": "Option with maximum length", "buf": [119, 255] + [0] * 255, "err": None},
    {"msg": "Too short option", "buf": [], "err": "Not enough data to decode"},
    {"msg": "Too short option when option is not 0 or 255", "buf": [119], "err": "Not enough data to decode"},
    {"msg": "Malformed option", "buf": [119, 1], "err": "Option is malformed"},
]


def wire_v4(s):
    """RFC 2131: op, htype, hlen, hops, xid, secs, flags, ciaddr, yiaddr, siaddr, giaddr, chaddr
    (16), sname (64), file (128), the magic cookie, the options, End."""
    b = struct.pack(">BBBBIHH", s["Operation"], s["HardwareType"], s["HardwareLen"], s["HardwareOpts"], s["Xid"],
                    s["Secs"], s["Flags"])
    for f in ("ClientIP", "YourClientIP", "NextServerIP", "RelayAgentIP"):
        b += bytes(s[f])
    b += bytes(s["ClientHWAddr"]).ljust(16, b"\0") + bytes(s["ServerName"]) + bytes(s["File"])
    b += struct.pack(">I", 0x63825363)
    for o in s["Options"]:
        b += bytes([0]) if o["Type"] == 0 else bytes([o["Type"], len(o["Data"])]) + bytes(o["Data"])
    return b + b"\xff"


def wire_v6(s):
    """RFC 8415: msg-type, transaction-id, options."""
    b = bytes([s["MsgType"]]) + bytes(s["TransactionID"])
    for o in s["Options"]:
        b += struct.pack(">HH", o["Code"], o["Length"]) + bytes(o["Data"])
    return b


def main():
    out = {"source": "google/gopacket layers/dhcp_test.go, layers/dhcpv6_test.go (values transcribed; wire bytes "
                     "built from RFC 2131 / RFC 8415, see make_dhcp_vectors.py)",
           "v4": [dict(s, hex=wire_v4(s).hex()) for s in V4],
           "v6": [dict(s, hex=wire_v6(s).hex()) for s in V6],
           "option_cases": OPTION_CASES}
    with open(os.path.join(HERE, "dhcp_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
