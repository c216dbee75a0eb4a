"""TLS messages for the tests of the TLS record decode (tests/test_tls.py, tests/test_tls_gpu.py):
the reference's vectors (tests/golden/tls_vectors.json), hand-built messages for every error return
and length rule of layers/tls.go, seeded mutations, the frames that carry them (the encapsulations
of tests/dns_cases.py with TCP in place of UDP), and what the decode must produce for a batch
(from the CPU oracle's layer objects and tests/tls_ref.py)."""
import json
import os
import struct

import numpy as np

import tls_ref as R
from dns_cases import MAC, dot1q, eth, ip4, ip6, udp, vxlan  # noqa: F401  (the encapsulations)

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "tls_vectors.json")))


def vector(name):
    """The TLS data of a vector (testClientHello without its Ethernet/IPv4/TCP headers)."""
    v = next(v for v in VEC["vectors"] if v["name"] == name)
    return bytes.fromhex(v["hex"])[v["tls_off"]:]


def vector_messages():
    """(name, TLS data) of every vector and of the three error tests' inputs."""
    out = [(v["name"], vector(v["name"])) for v in VEC["vectors"]]
    out += [(e["test"], bytes.fromhex(e["hex"])) for e in VEC["errors"]]
    return out


# ---------------------------------------------------------------- hand-built messages
CCS, ALERT, HS, APP = 20, 21, 22, 23
V10, V12 = 0x0301, 0x0303


def rec(ct, body=b"", ver=V12, length=None):
    return struct.pack(">BHH", ct, ver, len(body) if length is None else length) + body


def named_cases():
    """name -> message: every reachable error return, the length rules and the edges."""
    c = {}
    whole = rec(HS, b"\x01\x00\x00\x02ab")
    for k in range(7):                                    # payload lengths 0 to 6
        c[f"len_{k}"] = whole[:k]
    c["exact_end"] = rec(APP, b"data")                    # the record ends where data ends
    for k in (1, 2, 3, 4):                                # a short tail behind a good record
        c[f"tail_{k}"] = rec(APP, b"data") + rec(HS, b"xy")[:k]
    for ct, nm in ((CCS, "ccs"), (ALERT, "alert"), (HS, "handshake"), (APP, "appdata")):
        c[f"length0_{nm}"] = rec(ct)                      # CCS: incorrect length; Alert: too short
    c["alert_len1"] = rec(ALERT, b"\x02")
    c["alert_len2"] = rec(ALERT, b"\x02\x28")             # fatal, handshake_failure
    c["alert_len3"] = rec(ALERT, b"\x02\x28\x00")         # Length != 2: EncryptedMsg
    c["alert_warning_close"] = rec(ALERT, b"\x01\x00") + rec(ALERT, b"\x07\x63")
    c["ccs_msg1"] = rec(CCS, b"\x01")
    c["ccs_msg0"] = rec(CCS, b"\x00")                     # -> 255
    c["ccs_msg2"] = rec(CCS, b"\x02")                     # -> 255
    c["ccs_len2"] = rec(CCS, b"\x01\x01")
    c["length_ffff_short"] = rec(APP, b"x" * 10, length=0xFFFF)
    c["length_ffff_full"] = rec(APP, bytes(range(256)) * 255 + bytes(255)) + rec(ALERT, b"\x01\x00")
    for ct in (0, 19, 24, 255):
        c[f"type_{ct}"] = rec(ct, b"abc")
    c["type_19_short_body"] = rec(19, b"abc", length=9)   # the type is tested before the length
    for ver in (0x0200, 0x0300, 0x0301, 0x0302, 0x0303, 0x0304, 0x0305):
        c[f"version_{ver:04x}"] = rec(HS, b"v", ver=ver)
    c["error_after_two"] = rec(HS, b"hello") + rec(CCS, b"\x01") + rec(APP, b"cut", length=200)
    c["unknown_after_two"] = rec(APP, b"a") + rec(APP, b"") + rec(99, b"zz") + rec(APP, b"never")
    c["ccs_error_after_alert"] = rec(ALERT, b"enc-alert-body") + rec(CCS, b"")
    c["all_four"] = rec(HS, b"h" * 9) + rec(CCS, b"\x01") + rec(APP, b"p" * 7) + rec(ALERT, b"\x01\x00") + rec(HS)
    c["handshake_300"] = rec(HS) * 300                    # 300 zero-length records, 1500 bytes
    return c


# cases that no TCP/IPv4 packet can carry: an empty payload never reaches the stop type, and a
# record of Length 0xFFFF is longer than an IPv4 datagram.  The host and ranges tests cover them.
NOT_IN_PACKETS = ("len_0", "length_ffff_full")


def packet_cases():
    return {k: v for k, v in named_cases().items() if k not in NOT_IN_PACKETS}


def zero_records(n, ct=HS):
    """n records of Length 0: work n."""
    return rec(ct) * n


def mutations(seed, count, bases):
    """`count` seeded mutations of the messages in `bases`: byte flips, a header's type, version or
    length rewritten, cuts, a record spliced in."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(bases[int(rng.integers(len(bases)))][:4096])
        kind = int(rng.integers(6))
        if len(b) < 6:
            kind = 0
        if kind == 0 and len(b):      # byte flips
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(len(b)))] ^= 1 << int(rng.integers(8))
        elif kind == 1:               # the first header's length
            b[3:5] = struct.pack(">H", int(rng.choice([0, 1, 2, 3, max(len(b) - 5, 0) & 0xFFFF, len(b) & 0xFFFF, 0xFFFF])))
        elif kind == 2:               # the first header's type
            b[0] = int(rng.choice([0, 19, 20, 21, 22, 23, 24, 255]))
        elif kind == 3:               # a random byte set
            b[int(rng.integers(len(b)))] = int(rng.integers(256))
        elif kind == 4:               # cut
            b = b[:int(rng.integers(len(b) + 1))]
        else:                         # a short record in front, so that the rest is a later invocation
            b = bytearray(rec(int(rng.choice([CCS, ALERT, HS, APP])), bytes(int(rng.integers(4))))) + b
        out.append(bytes(b))
    return out


# ---------------------------------------------------------------- frames
def tcp(payload, sport=40000, dport=443, flags=0x18, doff=5, seq=1):
    """A TCP header of `doff` words (options: NOPs) and the payload."""
    return struct.pack(">HHIIBBHHH", sport, dport, seq, 1, doff << 4, flags, 65535, 0, 0) + b"\x01" * (4 * (doff - 5)) + payload


ENCAPS = {
    "eth_ip4_tcp": lambda m: eth(ip4(tcp(m), 6)),
    "eth_ip6_tcp": lambda m: eth(ip6(tcp(m), 6), 0x86DD),
    "dot1q": lambda m: dot1q(ip4(tcp(m, sport=443, dport=40000), 6)),
    "vxlan": lambda m: vxlan(eth(ip4(tcp(m, dport=993), 6))),
    "doff6": lambda m: eth(ip4(tcp(m, doff=6), 6)),
    "doff11": lambda m: eth(ip4(tcp(m, doff=11, dport=5061), 6)),
    "doff15": lambda m: eth(ip6(tcp(m, doff=15, dport=636), 6), 0x86DD),
}

NOISE = [
    eth(ip4(tcp(b"GET / HTTP/1.0\r\n", dport=8080), 6)),           # non-TLS TCP
    eth(ip4(udp(b"not tls", dport=5000), 17)),                     # UDP
    MAC + struct.pack(">H", 0x0806) + bytes(28),                   # ARP
    MAC[:9],                                                       # a runt
    eth(ip4(tcp(b"", flags=0x10), 6)),                             # port 443, empty payload
    eth(ip4(udp(b"\x16\x03\x03\x00\x00", dport=443), 17)),         # UDP 443 is not TLS by default
    eth(ip4(tcp(b"x" * 20)[:14], 6)),                              # a cut TCP header: decode error
]


def interleave(frames):
    """The frames with the noise packets between them."""
    out = []
    for k, f in enumerate(frames):
        out.append(NOISE[k % len(NOISE)])
        out.append(f)
    out.append(NOISE[0])
    return out


# ---------------------------------------------------------------- what the decode must produce
def expect(batch, ref, max_records=1024):
    """(msgs, recs, models) for a PacketBatch and the CPU oracle's result `ref` (ext=True): the
    candidates are the packets whose decode stopped at LayerTypeTLS without an error; `data` is
    the Payload of the last decoded layer's object."""
    from gopacket_amd.results import OBJ_NAMES, st_class
    code_obj = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 4, 7: 4, 8: 4, 9: 5, 10: 6, 11: 7, 12: 8, 13: 9, 14: 10, 15: 11}
    msgs, recs, models, nrec = [], [], [], 0
    for i in range(batch.n):
        if (int(ref.layers[i]) & 0xFFFF) != 140 or st_class(int(ref.status[i])) == 2:
            continue
        words = ref.ext["layer_codes"][i]
        codes = [(int(words[k // 16]) >> (4 * (k % 16))) & 15 for k in range(32)]
        last = [c for c in codes if c][-1]
        (_, _), (p0, p1) = ref.layer(i, OBJ_NAMES[code_obj[last]])
        data = batch.packet(i)[p0:p1]
        t = R.decode(data)
        m, r = R.records(t, len(data), max_records, packet=i, data_off=p0, first_record=nrec)
        nrec += len(r)
        msgs.append(m)
        recs.append(r)
        models.append((data, t))
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    return cat(msgs, R.MSG_DTYPE), cat(recs, R.REC_DTYPE), models


def expect_ranges(datas, max_records=1024):
    """(msgs, recs, models) for messages decoded as ranges: packet is the index, data_off 0."""
    msgs, recs, models, nrec = [], [], [], 0
    for k, data in enumerate(datas):
        t = R.decode(data)
        m, r = R.records(t, len(data), max_records, packet=k, first_record=nrec)
        nrec += len(r)
        msgs.append(m)
        recs.append(r)
        models.append((data, t))
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    return cat(msgs, R.MSG_DTYPE), cat(recs, R.REC_DTYPE), models


def same_object(got, want):
    """A TLS object of gopacket_amd.tls against the model's (tests/tls_ref.py), field by field."""
    assert (str(got.err) if got.err else None) == (str(want.err) if want.err else None)
    assert (got.err.code if got.err else 0) == (want.err.code if want.err else 0)
    assert got.truncated == want.truncated
    assert got.Contents == want.Contents
    head = lambda x: (x.ContentType, x.Version, x.Length)
    assert [head(x) + (x.Message,) for x in got.ChangeCipherSpec] == [head(x) + (x.Message,) for x in want.ChangeCipherSpec]
    assert [head(x) for x in got.Handshake] == [head(x) for x in want.Handshake]
    assert [head(x) + (x.Payload,) for x in got.AppData] == [head(x) + (x.Payload,) for x in want.AppData]
    assert [head(x) + (x.Level, x.Description, x.EncryptedMsg) for x in got.Alert] == \
        [head(x) + (x.Level, x.Description, x.EncryptedMsg) for x in want.Alert]
