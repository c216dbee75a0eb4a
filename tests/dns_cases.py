"""DNS messages for the tests of the DNS decode (tests/test_dns.py, tests/test_dns_gpu.py): the
reference's vectors (tests/golden/dns_vectors.json), hand-built messages for every error return
and name quirk of layers/dns.go, seeded mutations, the frames that carry them, and what the
decode must produce for a batch (from the CPU oracle's layer objects and tests/dns_ref.py)."""
import json
import os
import struct

import numpy as np

import dns_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "dns_vectors.json")))


def vector_messages():
    """(name, message bytes) of every vector and fuzz input."""
    out = []
    for v in VEC["vectors"]:
        f = bytes.fromhex(v["frame_hex"])
        out.append((v["test"], f[v["dns_off"]:v["dns_off"] + v["dns_len"]]))
    out += [("fuzz-" + f["name"][:8], bytes.fromhex(f["hex"])) for f in VEC["fuzz"]]
    return out


# ---------------------------------------------------------------- hand-built messages
def hdr(qd=0, an=0, ns=0, ar=0, ident=0x1234, flags=0x8180):
    return struct.pack(">6H", ident, flags, qd, an, ns, ar)


def name(*labels):
    return b"".join(bytes([len(x)]) + x for x in labels) + b"\x00"


def ptr(off):
    return struct.pack(">H", 0xC000 | off)


def q(n, t=1, c=1):
    return n + struct.pack(">HH", t, c)


def rr(n, t, rdata, c=1, ttl=300, rdlen=None):
    return n + struct.pack(">HHIH", t, c, ttl, len(rdata) if rdlen is None else rdlen) + rdata


WWW = name(b"www", b"example", b"com")  # at offset 12 of a message that starts with a question


def compressed_response():
    """A response of about 120 bytes with pointers in names and rdata (the truncation sweep)."""
    m = hdr(1, 3, 1, 1) + q(WWW)
    m += rr(ptr(12), 5, name(b"web") + ptr(16))                      # CNAME web.example.com
    m += rr(ptr(12), 1, bytes([192, 0, 2, 1]))
    m += rr(ptr(16), 15, struct.pack(">H", 10) + name(b"mx") + ptr(16))   # MX
    m += rr(ptr(16), 2, name(b"ns1") + ptr(16))                      # NS (authority)
    m += rr(b"\x00", 41, struct.pack(">HH", 10, 2) + b"hi", c=4096, ttl=0x01000000)  # OPT, ext rcode 0x10
    return m


def named_cases():
    """name -> message: every reachable error return and the name quirks."""
    c = {}
    c["too_short"] = hdr()[:11]
    c["header_only"] = hdr()
    c["query"] = hdr(1) + q(WWW)
    c["forward_pointer"] = hdr(1) + ptr(18) + struct.pack(">HH", 1, 1) + name(b"fwd", b"org")
    c["self_pointer"] = hdr(1) + ptr(12) + struct.pack(">HH", 1, 1)                      # max recursion
    m = hdr(1) + ptr(0) + struct.pack(">HH", 1, 1)
    c["pointer_to_len"] = m[:12] + ptr(len(m)) + m[14:]                                  # name offset too high
    c["pointer_past_len"] = m[:12] + ptr(len(m) + 1) + m[14:]                            # pointer too high
    c["pointer_cut"] = hdr(1) + b"\xc0"                                                 # index + 2 > len
    c["offset_at_len"] = hdr(1)                                                          # offset >= len at level 1
    c["empty_by_pointer"] = hdr(1) + ptr(16) + struct.pack(">HH", 1, 0)                  # byte 16 is the class's zero
    c["label_40"] = hdr(1) + b"\x41" + b"x" * 8
    c["label_80"] = hdr(1) + b"\x03abc\x85" + b"x" * 8
    c["invalid_index"] = hdr(1) + b"\x09abc"
    c["index_range"] = hdr(1) + b"\x03abc"
    lab = lambda n: bytes([n]) + b"a" * n
    c["level_255"] = hdr(1) + q(lab(63) * 3 + lab(62) + b"\x00")                         # index2 - offset == 255
    c["level_256"] = hdr(1) + q(lab(63) * 4 + b"\x00")                                   # 256: too long
    # 255 is per level: a second level of 250 bytes behind a first of 250
    second = lab(63) * 3 + lab(57) + b"\x00"
    first = lab(63) * 3 + lab(57)
    m = hdr(1) + first + ptr(12 + len(first) + 2 + 4) + struct.pack(">HH", 1, 1) + second
    c["two_levels_500"] = m
    c["question_small"] = hdr(1) + WWW + b"\x00\x01\x00"
    c["record_small"] = hdr(0, 1) + WWW + b"\x00\x01\x00\x01\x00\x00\x00\x00\x00"
    c["record_length"] = hdr(0, 1) + rr(WWW, 1, b"\x01\x02", rdlen=4)
    c["rdata_pointer_past_end"] = hdr(0, 2) + rr(WWW, 5, ptr(12 + len(WWW) + 10 + 2 + 2), rdlen=2) + rr(WWW, 1, b"abcd")
    c["rdata_pointer_to_end"] = hdr(0, 2) + rr(WWW, 5, ptr(12 + len(WWW) + 10 + 2), rdlen=2) + rr(WWW, 1, b"abcd")
    c["char_string"] = hdr(0, 1) + rr(WWW, 16, b"\x03ab")
    c["hinfo_ok"] = hdr(0, 1) + rr(WWW, 13, b"\x03cpu\x02os")
    c["txt_empty_strings"] = hdr(0, 1) + rr(WWW, 16, b"\x00\x00\x01a")
    soa = name(b"ns") + name(b"root")
    c["soa_ok"] = hdr(0, 1) + rr(WWW, 6, soa + struct.pack(">5I", 1, 2, 3, 4, 5))
    c["soa_small"] = hdr(0, 1) + rr(WWW, 6, soa + struct.pack(">4I", 1, 2, 3, 4) + b"\x00\x00\x00")
    c["mx_small"] = hdr(0, 1) + rr(WWW, 15, b"\x00")
    c["mx_no_name"] = hdr(0, 1) + rr(WWW, 15, b"\x00\x0a")                              # name offset == end
    c["uri_small"] = hdr(0, 1) + rr(WWW, 256, b"\x00\x01\x00")
    c["uri_ok"] = hdr(0, 1) + rr(WWW, 256, b"\x00\x01\x00\x02http://x")
    c["srv_small"] = hdr(0, 1) + rr(WWW, 33, b"\x00\x01\x00\x02\x00")
    c["srv_ok"] = hdr(0, 1) + rr(WWW, 33, struct.pack(">3H", 1, 2, 443) + name(b"svc"))
    c["opt_short"] = hdr(0, 0, 0, 1) + rr(b"\x00", 41, b"\x00\x01\x00")
    c["opt_malformed"] = hdr(0, 0, 0, 1) + rr(b"\x00", 41, struct.pack(">HH", 1, 1) + b"x" + b"\x00\x02")
    c["opt_length"] = hdr(0, 0, 0, 1) + rr(b"\x00", 41, struct.pack(">HH", 1, 9) + b"x")
    c["opt_in_answers"] = hdr(0, 1) + rr(b"\x00", 41, b"", ttl=0xFF000000)              # no rcode extension there
    c["opt_rcode"] = hdr(0, 0, 0, 2, flags=0x8183) + rr(b"\x00", 41, b"", ttl=0x12000000) + rr(b"\x00", 41, b"", ttl=0x04000000)
    for t, nm in ((1, "a"), (28, "aaaa"), (2, "ns"), (5, "cname"), (12, "ptr"), (6, "soa"), (15, "mx"), (16, "txt"),
                  (13, "hinfo"), (33, "srv"), (41, "opt"), (256, "uri"), (99, "unknown")):
        c["rdlen0_" + nm] = hdr(0, 1) + rr(WWW, t, b"")
    c["error_after_entries"] = hdr(1, 2) + q(WWW) + rr(ptr(12), 1, b"\x01\x02\x03\x04") + rr(ptr(12), 16, b"\x09a")
    c["sections"] = hdr(1, 1, 1, 1) + q(WWW) + rr(ptr(12), 1, b"\x7f\x00\x00\x01") + \
        rr(ptr(16), 2, name(b"ns") + ptr(16)) + rr(ptr(16), 28, bytes(16))
    c["compressed_response"] = compressed_response()
    return c


def pointer_chain(levels, tail=b"\x03end\x00"):
    """A question whose name is `levels` pointers one after another, then `tail`: each pointer is
    a decodeName call and a loop iteration (work grows by 2 a level)."""
    m = bytearray(hdr(1) + ptr(18) + struct.pack(">HH", 1, 1))
    for k in range(levels - 1):
        m += ptr(len(m) + 2)
    return bytes(m + tail)


def bomb():
    """Thousands of records, each a long pointer chain into one long name: a message of a few
    KiB whose work is in the hundreds of thousands."""
    lab = lambda n: bytes([n]) + b"b" * n
    long_name = lab(63) * 3 + lab(61) + b"\x00"
    m = bytearray(hdr(1, 400) + q(long_name))
    at = 12
    for _ in range(400):
        m += ptr(at) + struct.pack(">HHIH", 5, 1, 0, 2)
        at = len(m)
        m += ptr(12)
    return bytes(m)


def mutations(seed, count, bases):
    """`count` seeded mutations of the messages in `bases`: byte flips, pointer rewrites, count
    rewrites, cuts."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        b = bytearray(bases[int(rng.integers(len(bases)))])
        kind = int(rng.integers(5))
        if len(b) < 13:
            kind = 0
        if kind == 0 and len(b):      # byte flips
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(len(b)))] ^= 1 << int(rng.integers(8))
        elif kind == 1:               # a pointer written somewhere behind the header
            i = int(rng.integers(12, len(b) - 1)) if len(b) > 13 else 12
            b[i:i + 2] = ptr(int(rng.integers(0, min(len(b) + 3, 0x3FFF))))
        elif kind == 2:               # a count rewritten
            i = 4 + 2 * int(rng.integers(4))
            b[i:i + 2] = struct.pack(">H", int(rng.choice([0, 1, 2, 3, 7, 255, 65535])))
        elif kind == 3:               # a length byte or a random byte set
            b[int(rng.integers(12, len(b)))] = int(rng.integers(256))
        else:                         # cut, sometimes with a flip
            b = b[:int(rng.integers(len(b) + 1))]
            if len(b) and rng.integers(2):
                b[int(rng.integers(len(b)))] ^= 0xC0
        out.append(bytes(b))
    return out


# ---------------------------------------------------------------- frames
MAC = bytes.fromhex("0022 19b6 7e22 000f 35bb 0b40".replace(" ", ""))
A4, B4 = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])
A6, B6 = bytes(15) + b"\x01", bytes(15) + b"\x02"


def udp(payload, sport=40000, dport=53, length=None):
    return struct.pack(">4H", sport, dport, 8 + len(payload) if length is None else length, 0) + payload


def tcp(payload, sport=40000, dport=53, flags=0x18):
    return struct.pack(">HHIIBBHHH", sport, dport, 1, 1, 5 << 4, flags, 65535, 0, 0) + payload


def ip4(payload, proto, length=None, frag=0, ident=1):
    h = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(payload) if length is None else length, ident, frag, 64, proto, 0)
    return h + A4 + B4 + payload


def ip6(payload, nh):
    return struct.pack(">IHBB", 0x60000000, len(payload), nh, 64) + A6 + B6 + payload


def eth(payload, etype=0x0800):
    return MAC + struct.pack(">H", etype) + payload


def dot1q(payload, etype=0x0800, vlan=5):
    return MAC + struct.pack(">HHH", 0x8100, vlan, etype) + payload


def vxlan(inner):
    return eth(ip4(udp(struct.pack(">II", 0x08000000, 42 << 8) + inner, dport=4789), 17))


ENCAPS = {
    "eth_ip4_udp": lambda m: eth(ip4(udp(m), 17)),
    "eth_ip6_udp": lambda m: eth(ip6(udp(m), 17), 0x86DD),
    "eth_ip4_tcp": lambda m: eth(ip4(tcp(m), 6)),
    "dot1q": lambda m: dot1q(ip4(udp(m, sport=53, dport=40000), 17)),
    "vxlan": lambda m: vxlan(eth(ip4(udp(m), 17))),
}

NOISE = [
    eth(ip4(udp(b"not dns", dport=5000), 17)),                     # non-DNS UDP
    eth(ip4(tcp(b"GET / HTTP/1.0\r\n", dport=8080), 6)),           # non-DNS TCP
    MAC + struct.pack(">H", 0x0806) + bytes(28),                   # ARP
    MAC[:9],                                                       # a runt
    eth(ip4(udp(b""), 17)),                                        # port 53, empty payload
    eth(ip4(tcp(b"", flags=0x10), 6)),                             # TCP 53, bare ACK
    eth(ip4(udp(b"x" * 20)[:6], 17)),                              # a cut UDP header: decode error
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
def expect(batch, ref, max_work=4096):
    """(msgs, entries, names, models) for a PacketBatch and the CPU oracle's result `ref`
    (ext=True): the candidates are the packets whose decode stopped at LayerTypeDNS without an
    error; `data` is the Payload of the last decoded layer's object."""
    from gopacket_amd.results import OBJ_NAMES, st_class
    code_obj = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 4, 7: 4, 8: 4, 9: 5, 10: 6, 11: 7, 12: 8, 13: 9, 14: 10, 15: 11}
    msgs, ents, names, models = [], [], bytearray(), []
    for i in range(batch.n):
        if (int(ref.layers[i]) & 0xFFFF) != 107 or st_class(int(ref.status[i])) == 2:
            continue
        words = ref.ext["layer_codes"][i]
        codes = [(int(words[k // 16]) >> (4 * (k % 16))) & 15 for k in range(32)]
        last = [c for c in codes if c][-1]
        (_, _), (p0, p1) = ref.layer(i, OBJ_NAMES[code_obj[last]])
        data = batch.packet(i)[p0:p1]
        d = R.decode(data)
        m, e, n = R.records(d, len(data), max_work, packet=i, data_off=p0, first_entry=sum(len(x) for x in ents),
                            name_base=len(names))
        msgs.append(m)
        ents.append(e)
        names += n
        models.append((data, d))
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    return cat(msgs, R.MSG_DTYPE), cat(ents, R.ENTRY_DTYPE), bytes(names), models


def same_object(got, want):
    """A DNS object of gopacket_amd.dns against the model's (tests/dns_ref.py), field by field."""
    assert (str(got.err) if got.err else None) == (str(want.err) if want.err else None)
    assert got.truncated == want.truncated
    if want.err is not None and want.err.code == R.E_TOO_SHORT:
        return
    for f in ("ID", "QR", "OpCode", "AA", "TC", "RD", "RA", "Z", "ResponseCode", "QDCount", "ANCount", "NSCount",
              "ARCount"):
        assert getattr(got, f) == getattr(want, f), f
    assert [(x.Name, x.Type, x.Class) for x in got.Questions] == [(x.Name, x.Type, x.Class) for x in want.Questions]
    for sec in ("Answers", "Authorities", "Additionals"):
        g, w = getattr(got, sec), getattr(want, sec)
        assert len(g) == len(w), sec
        for a, b in zip(g, w):
            for f in ("Name", "Type", "Class", "TTL", "DataLength", "Data", "IP", "NS", "CNAME", "PTR", "TXT", "TXTs"):
                assert getattr(a, f) == getattr(b, f), (sec, f)
            assert (a.SOA.MName, a.SOA.RName, a.SOA.Serial, a.SOA.Refresh, a.SOA.Retry, a.SOA.Expire, a.SOA.Minimum) == \
                (b.SOA.MName, b.SOA.RName, b.SOA.Serial, b.SOA.Refresh, b.SOA.Retry, b.SOA.Expire, b.SOA.Minimum)
            assert (a.SRV.Priority, a.SRV.Weight, a.SRV.Port, a.SRV.Name) == \
                (b.SRV["Priority"], b.SRV["Weight"], b.SRV["Port"], b.SRV["Name"])
            assert (a.MX.Preference, a.MX.Name) == (b.MX["Preference"], b.MX["Name"])
            assert (a.URI.Priority, a.URI.Weight, a.URI.Target) == (b.URI["Priority"], b.URI["Weight"], b.URI["Target"])
            assert (None if a.OPT is None else [(o.Code, o.Data) for o in a.OPT]) == b.OPT
