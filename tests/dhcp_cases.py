"""DHCP messages for the tests of the DHCP decode (tests/test_dhcp.py, tests/test_dhcp_gpu.py): the
reference's test structs as wire bytes (tests/golden/dhcp_vectors.json), hand-built messages for
every reachable error return and quirk of layers/dhcpv4.go and layers/dhcpv6.go, seeded mutations,
the frames that carry them (the encapsulations of tests/dns_cases.py on the DHCP ports), and what
the decode must produce for a batch (from the CPU oracle's layer objects and tests/dhcp_ref.py).
A message is a (version, bytes) pair throughout."""
import json
import os
import struct

import numpy as np

import dhcp_ref as R
from dns_cases import MAC, dot1q, eth, ip4, ip6, tcp, udp, vxlan  # noqa: F401  (the encapsulations)

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "dhcp_vectors.json")))


def vector_messages():
    """(name, (version, bytes)) of the four transcribed structs."""
    return [(s["test"], (4, bytes.fromhex(s["hex"]))) for s in VEC["v4"]] + \
        [(s["test"], (6, bytes.fromhex(s["hex"]))) for s in VEC["v6"]]


# ---------------------------------------------------------------- hand-built messages
def bootp(op=1, htype=1, hlen=6, hops=0, xid=0xDEADBEEF, secs=3, flags=0x8000, magic=R.MAGIC):
    """The 240 bytes in front of the options."""
    b = struct.pack(">BBBBIHH", op, htype, hlen, hops, xid, secs, flags)
    b += bytes([10, 0, 0, 5, 10, 0, 0, 6, 10, 0, 0, 1, 10, 0, 0, 254])
    b += bytes(range(0x20, 0x30)) + b"server".ljust(64, b"\0") + b"boot/file".ljust(128, b"\0")
    return b + struct.pack(">I", magic)


def o4(t, data=b"", length=None):
    return bytes([t, len(data) if length is None else length]) + data


def o6(code, data=b"", length=None):
    return struct.pack(">HH", code, len(data) if length is None else length) + data


DISCOVER = bootp() + o4(53, b"\x01") + o4(61, b"\x01" + bytes(range(0x20, 0x26))) + o4(12, b"host-a") + b"\x00" + \
    o4(60, b"MSFT 5.0") + o4(55, bytes([1, 3, 6, 15, 31, 33, 43, 44])) + o4(57, b"\x05\xdc") + o4(50, bytes([10, 0, 0, 9])) + b"\xff"

SOLICIT = bytes([1, 0xAB, 0xCD, 0xEF]) + o6(1, bytes(14)) + o6(6, struct.pack(">3H", 23, 24, 39)) + o6(8, b"\x00\x00") + \
    o6(3, bytes(12) + o6(5, bytes(24)))
RELAY = bytes([12, 3]) + bytes(range(16)) + bytes(range(16, 32)) + o6(18, b"eth0/7") + o6(9, SOLICIT) + o6(37, bytes(6))


def named_cases():
    """name -> (version, message): every reachable error return, the quirks and the edges."""
    c = {}
    v4 = lambda name, b: c.__setitem__("v4_" + name, (4, b))
    v6 = lambda name, b: c.__setitem__("v6_" + name, (6, b))
    h = bootp()
    v4("len_0", b"")
    v4("len_1", h[:1])
    v4("len_239", h[:239])                                     # too short, nothing assigned
    v4("len_240", h)                                           # nil, Contents not set
    v4("len_241_end", h + b"\xff")
    v4("len_241_pad", h + b"\x00")
    v4("len_241_type", h + b"\x77")                            # a lone type byte: not enough data
    v4("bad_magic_240", bootp(magic=0x63825362))
    v4("bad_magic_options", bootp(magic=0) + o4(53, b"\x01") + b"\xff")
    v4("bad_magic_hlen_227", bootp(hlen=227, magic=1))         # the flag and the cookie error together
    v4("bad_magic_hlen_228", bootp(hlen=228, magic=1))         # the panic at :143 comes before the cookie
    # 28+HardwareLen is a uint8 sum: up to 227 it can pass data (213 and 227 pass the 240 bytes, 213
    # fits 241 exactly), from 228 up it wraps below 28 and the reference panics at every length
    for hl in (0, 16, 212, 213, 227, 228, 255):
        v4(f"hlen_{hl}_240", bootp(hlen=hl))
        v4(f"hlen_{hl}_241", bootp(hlen=hl) + b"\xff")
    v4("hlen_227_254", bootp(hlen=227) + b"\x00" * 14)         # one byte short of 28 + 227: clipped, OK
    v4("hlen_227_255", bootp(hlen=227) + b"\x00" * 15)         # fits exactly
    v4("hlen_227_256", bootp(hlen=227) + b"\x00" * 15 + b"\xff")
    v4("hlen_228_256", bootp(hlen=228) + b"\x00" * 15 + b"\xff")  # 28 + 228 would fit: it wraps to 0
    v4("hlen_255_282", bootp(hlen=255) + b"\x00" * 42)
    v4("hlen_255_283", bootp(hlen=255) + b"\x00" * 43)         # 28 + 255 would fit: it wraps to 27
    v4("discover", DISCOVER)
    v4("no_end", DISCOVER[:-1])                                # the list runs to the end of data: OK
    v4("pads_only", h + b"\x00" * 9)
    v4("end_then_garbage", h + o4(53, b"\x02") + b"\xff" + b"\x77\xf0garbage")
    v4("end_first", h + b"\xff" + o4(53, b"\x02"))
    v4("zero_length", h + o4(119) + b"\xff")
    v4("max_length", h + o4(119, bytes(255)) + b"\xff")
    v4("max_length_cut", h + o4(119, bytes(254), length=255))  # malformed by one byte
    v4("exact_fit", h + o4(12, b"abc"))                        # Length ends where data ends
    v4("tail_type_after_two", h + o4(53, b"\x01") + b"\x00" + b"\x0c")
    v4("malformed_first", h + o4(119, b"", length=1))
    v4("malformed_after_three", h + o4(53, b"\x03") + b"\x00" + o4(12, b"xy") + o4(55, b"ab", length=200) + b"\xff")
    v4("type_254", h + o4(254, b"z") + b"\xff")
    v4("htype_op_255", bootp(op=255, htype=255, hops=255, xid=0xFFFFFFFF, secs=0xFFFF, flags=0xFFFF) + b"\xff")
    v4("pads_600", h + b"\x00" * 600 + b"\xff")
    s = SOLICIT
    for k in range(4):
        v6(f"len_{k}", s[:k])
    v6("len_4", s[:4])                                         # no options: OK
    for t in (12, 13):
        r = bytes([t]) + RELAY[1:]
        v6(f"relay_{t}_3", r[:3])                              # the first length test comes first
        v6(f"relay_{t}_4", r[:4])
        v6(f"relay_{t}_33", r[:33])
        v6(f"relay_{t}_34", r[:34])
        v6(f"relay_{t}_full", r)
    v6("type_11_34", bytes([11]) + RELAY[1:34])                # not a relay type: options at 4
    v6("type_14_4", bytes([14, 1, 2, 3]))
    v6("solicit", s)
    for k in (1, 2, 3):
        v6(f"tail_{k}", s[:4] + o6(1, b"abcd") + o6(2, b"xy")[:k])
    v6("size_short", s[:4] + o6(1, b"abc", length=10))         # %d = 14
    v6("size_wrap_fffc", s[:4] + o6(1, b"abc", length=0xFFFC)) # %d = 0
    v6("size_wrap_fffe", s[:4] + o6(1, b"abc", length=0xFFFE)) # %d = 2
    v6("size_wrap_ffff", s[:4] + o6(1, b"", length=0xFFFF))    # %d = 3
    v6("size_after_two", s[:4] + o6(1, b"a") + o6(2, b"") + o6(3, b"cut", length=4))
    v6("zero_length", s[:4] + o6(14) + o6(14))
    v6("relay_size_error", RELAY[:34] + o6(9, b"short", length=600))
    v6("relay_tail_2", RELAY + b"\x00\x09")
    v6("opts_300", s[:4] + o6(7) * 300)
    return c


# an empty payload never reaches the stop type; the host tests cover those
NOT_IN_PACKETS = ("v4_len_0", "v6_len_0")


def packet_cases():
    return {k: v for k, v in named_cases().items() if k not in NOT_IN_PACKETS}


def pads(n, end=True):
    """A DHCPv4 message of n Pad options (and End): work n (+ 1)."""
    return (4, bootp() + b"\x00" * n + (b"\xff" if end else b""))


def empty_opts6(n):
    """A DHCPv6 message of n options of Length 0: work n."""
    return (6, SOLICIT[:4] + o6(7) * n)


def mutations(seed, count, bases, version):
    """`count` seeded mutations of the messages of `version` in `bases`: byte flips, an option's
    length or type rewritten, the header's hlen / message type, cuts, an option spliced in."""
    rng = np.random.default_rng(seed)
    bases = [b for v, b in bases if v == version]
    first = 240 if version == 4 else 4
    out = []
    for _ in range(count):
        b = bytearray(bases[int(rng.integers(len(bases)))][:2048])
        kind = int(rng.integers(7))
        if len(b) <= first + 2:
            kind = 0
        if kind == 0 and len(b):      # byte flips
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(len(b)))] ^= 1 << int(rng.integers(8))
        elif kind == 1:               # a byte of the option area set
            b[int(rng.integers(first, len(b)))] = int(rng.choice([0, 1, 2, 3, 4, 12, 13, 255, int(rng.integers(256))]))
        elif kind == 2:               # the first option's length
            if version == 4:
                b[first + 1] = int(rng.choice([0, 1, 2, (len(b) - first - 2) & 0xFF, (len(b) - first - 1) & 0xFF, 255]))
            else:
                rest = max(len(b) - first - 4, 0)
                b[first + 2:first + 4] = struct.pack(">H", int(rng.choice([0, 1, rest, rest + 1, 0xFFFB, 0xFFFC, 0xFFFF])))
        elif kind == 3:               # hlen / the message type
            if version == 4:
                b[2] = int(rng.choice([0, 6, 16, 212, 213, 214, 227, 228, 229, 255]))
            else:
                b[0] = int(rng.choice([0, 1, 11, 12, 13, 14, 255]))
        elif kind == 4:               # cut
            b = b[:int(rng.integers(len(b) + 1))]
        elif kind == 5:               # cut inside the option area
            b = b[:int(rng.integers(first, len(b) + 1))]
        else:                         # an option spliced in front of the list
            n = int(rng.integers(4))
            ins = (o4(int(rng.choice([0, 1, 53, 255])), bytes(n)) if version == 4 else o6(int(rng.integers(64)), bytes(n)))
            b = b[:first] + ins + b[first:]
        out.append((version, bytes(b)))
    return out


# ---------------------------------------------------------------- frames
PORTS = {4: (68, 67), 6: (546, 547)}


def _u(vm, swap=False, **kw):
    v, m = vm
    sp, dp = PORTS[v][::-1] if swap else PORTS[v]
    return udp(m, sport=sp, dport=dp, **kw)


ENCAPS = {
    "eth_ip4_udp": lambda vm: eth(ip4(_u(vm), 17)),
    "eth_ip6_udp": lambda vm: eth(ip6(_u(vm), 17), 0x86DD),
    "dot1q": lambda vm: dot1q(ip4(_u(vm, swap=True), 17)),
    "vxlan": lambda vm: vxlan(eth(ip4(_u(vm), 17))),
    "packed": lambda vm: eth(ip6(_u(vm, swap=True), 17), 0x86DD),   # (the batch is built with align=1)
}

NOISE = [
    eth(ip4(udp(b"not dhcp", dport=5000), 17)),                    # other UDP
    eth(ip4(tcp(bootp(), sport=68, dport=67), 6)),                 # TCP 67 is not DHCP
    MAC + struct.pack(">H", 0x0806) + bytes(28),                   # ARP
    MAC[:9],                                                       # a runt
    eth(ip4(udp(b"", sport=68, dport=67), 17)),                    # port 67, empty payload
    eth(ip4(udp(bootp(), dport=53), 17)),                          # a BOOTP header to the DNS port
    eth(ip4(udp(b"x" * 20, dport=67)[:6], 17)),                    # a cut UDP header: decode error
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
def expect(batch, ref, max_options=2048):
    """(msgs, opts, models) for a PacketBatch and the CPU oracle's result `ref` (ext=True): the
    candidates are the packets whose decode stopped at LayerTypeDHCPv4 or LayerTypeDHCPv6 without
    an error; `data` is the Payload of the last decoded layer's object."""
    from gopacket_amd.results import OBJ_NAMES, st_class
    code_obj = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 4, 7: 4, 8: 4, 9: 5, 10: 6, 11: 7, 12: 8, 13: 9, 14: 10, 15: 11}
    msgs, opts, models, nopt = [], [], [], 0
    for i in range(batch.n):
        stop = int(ref.layers[i]) & 0xFFFF
        if stop not in (118, 134) or st_class(int(ref.status[i])) == 2:
            continue
        words = ref.ext["layer_codes"][i]
        codes = [(int(words[k // 16]) >> (4 * (k % 16))) & 15 for k in range(32)]
        last = [c for c in codes if c][-1]
        (_, _), (p0, p1) = ref.layer(i, OBJ_NAMES[code_obj[last]])
        data = batch.packet(i)[p0:p1]
        version = 4 if stop == 118 else 6
        d = R.decode(version, data)
        m, o = R.records(d, len(data), max_options, packet=i, data_off=p0, first_opt=nopt)
        nopt += len(o)
        msgs.append(m)
        opts.append(o)
        models.append((data, d))
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    return cat(msgs, R.MSG_DTYPE), cat(opts, R.OPT_DTYPE), models


def same_object(got, want):
    """A DHCPv4 / DHCPv6 object of gopacket_amd.dhcp against the model's (tests/dhcp_ref.py)."""
    assert got.version == want.version
    assert (str(got.err) if got.err else None) == (str(want.err) if want.err else None)
    assert (got.err.code if got.err else 0) == (want.err.code if want.err else 0)
    assert got.truncated == want.truncated
    assert got.Contents == want.Contents and got.Payload is None
    if want.version == 4:
        for f in ("Operation", "HardwareType", "HardwareLen", "HardwareOpts", "Xid", "Secs", "Flags", "ClientIP",
                  "YourClientIP", "NextServerIP", "RelayAgentIP", "ClientHWAddr", "ServerName", "File", "hw_past_data"):
            assert getattr(got, f) == getattr(want, f), f
        assert [(o.Type, o.Length, o.Data) for o in got.Options] == [(o.Type, o.Length, o.Data) for o in want.Options]
    else:
        for f in ("MsgType", "HopCount", "LinkAddr", "PeerAddr", "TransactionID"):
            assert getattr(got, f) == getattr(want, f), f
        assert [(o.Code, o.Length, o.Data) for o in got.Options] == [(o.Code, o.Length, o.Data) for o in want.Options]
