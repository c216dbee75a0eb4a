"""DNS message decode: layers.DNS for a decoded device batch, on the GPU.

layers/ports.go:63,106 send UDP and TCP port 53 to LayerTypeDNS, which the engine carries as a
stop type: a DNS packet's `decoded` ends at UDP or TCP.  `DecodeDNS` runs
(*DNS).DecodeFromBytes (layers/dns.go:304-392) for every such packet of an HBM-resident batch the
parser just decoded (gpd_dns_decode, include/gpd_dns.h): the validation and the name
decompression on the device, one message record, one record per question / resource record and
the decompressed names.  `messages()` builds the reference's objects from them; fields that are
plain slices or fixed reads of rr.Data (IP, TXT, TXTs, OPT, URI, the MX/SRV numbers, the SOA
words) are read from the message bytes there.  A message whose work exceeds the budget comes back
deferred and is decoded by the host walker (gpd_dns_decode_host, the same code), so the caller
sees the reference's result for every candidate.

The entry points are bound onto the loaded library here, on first use, from DNS_EXPORTS.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib
from ._lib import GpdBatch, GpdResult, check
from ._names import DNS_CLASS_NAMES, DNS_OPCODE_NAMES, DNS_RCODE_NAMES, DNS_TYPE_NAMES

MSG_DTYPE = np.dtype([("packet", "<u4"), ("data_off", "<u4"), ("data_len", "<u4"), ("id", "<u2"), ("flags", "<u2"),
                      ("qdcount", "<u2"), ("ancount", "<u2"), ("nscount", "<u2"), ("arcount", "<u2"),
                      ("n_q", "<u2"), ("n_an", "<u2"), ("n_ns", "<u2"), ("n_ar", "<u2"),
                      ("rcode", "u1"), ("verdict", "u1"), ("truncated", "u1"), ("reserved", "u1"),
                      ("err_arg0", "<u4"), ("err_arg1", "<u4"), ("first_entry", "<u4")])
ENTRY_DTYPE = np.dtype([("name_off", "<u4"), ("name_len", "<u2"), ("rname1_len", "<u2"), ("rname2_len", "<u2"),
                        ("type", "<u2"), ("klass", "<u2"), ("rdlength", "<u2"), ("ttl", "<u4"),
                        ("rdata_off", "<u4"), ("fixed_off", "<u4"), ("section", "u1"), ("reserved", "u1", (3,))])
assert MSG_DTYPE.itemsize == 48 and ENTRY_DTYPE.itemsize == 32

DNS_OK, DNS_E_TOO_SHORT, DNS_E_COUNT, DNS_DEFERRED = 0, 1, 27, 255
MAX_WORK_DEFAULT, MAX_WORK_LIMIT = 4096, 65535
SEC_QUESTION, SEC_ANSWER, SEC_AUTHORITY, SEC_ADDITIONAL = range(4)
# candidates one block of the compaction and of the count scans takes, and block sums one round
# of their scan takes (gpd_compact.h kCompactBlock, compact_scan)
COMPACT_BLOCK = 2048
SCAN_ROUND = 1024

(DNSTypeA, DNSTypeNS, DNSTypeCNAME, DNSTypeSOA, DNSTypePTR, DNSTypeHINFO, DNSTypeMX, DNSTypeTXT, DNSTypeAAAA,
 DNSTypeSRV, DNSTypeOPT, DNSTypeURI) = 1, 2, 5, 6, 12, 13, 15, 16, 28, 33, 41, 256

# verdict -> the reference's error text (dns.go:1089-1107 and the inline errors); {0}, {1} are
# err_arg0 / err_arg1
ERROR_FORMATS = {
    1: "DNS packet too short",
    2: "max DNS recursion level hit",
    3: "dns name offset too high",
    4: "dns name offset is negative",
    5: "dns name is too long",
    6: "dns name uncomputable: invalid index",
    7: "dns offset pointer too high",
    8: "dns index walked out of range",
    9: "no dns data found for name",
    10: "qname '0x40' - RFC 2673 unsupported yet (data={0:x} index={1})",
    11: "qname '0x80' unsupported yet (data={0:x} index={1})",
    12: "DNS question too small",
    13: "DNS record too small",
    14: "resource record length exceeds data",
    15: "Insufficient data for a <character-string>",
    16: "SOA too small",
    17: "MX too small",
    18: "URI too small",
    19: "SRV too small",
    20: "DNSOPT record is of length {0}, it should be at least length 4",
    21: "Malformed DNSOPT record.  Length {0} < {1}",
    22: "Malformed DNSOPT record. The length ({0}) field implies a packet larger than the one received",
    23: "Invalid query decoding, not the right number of questions",
    24: "Invalid query decoding, not the right number of answers",
    25: "Invalid query decoding, not the right number of authorities",
    26: "Invalid query decoding, not the right number of additionals info",
}


class GpdDnsConfig(C.Structure):
    _fields_ = [("max_work", C.c_uint32), ("reserved", C.c_uint32)]


class GpdDnsOut(C.Structure):
    _fields_ = [("msgs", C.c_void_p), ("cap_msgs", C.c_uint64), ("entries", C.c_void_p), ("cap_entries", C.c_uint64),
                ("names", C.c_void_p), ("cap_names", C.c_uint64)]


class GpdDnsCounts(C.Structure):
    _fields_ = [("msgs", C.c_uint64), ("entries", C.c_uint64), ("name_bytes", C.c_uint64), ("deferred", C.c_uint64),
                ("work", C.c_uint64)]


DNS_EXPORTS = {
    # include/gpd_dns.h — name: (restype, argtypes)
    "gpd_dns_decode": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.POINTER(GpdResult), C.POINTER(GpdDnsConfig),
                                 C.POINTER(GpdDnsOut), C.POINTER(GpdDnsCounts), C.c_void_p]),
    "gpd_dns_decode_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_uint64, C.POINTER(GpdDnsCounts)]),
}

_bound = False


def dns_lib():
    """The loaded library with the DNS signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in DNS_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


def error_text(verdict: int, a0: int = 0, a1: int = 0) -> str:
    fmt = ERROR_FORMATS.get(int(verdict))
    if fmt is None:
        return f"gpd: unknown DNS verdict {verdict}"
    return fmt.format(int(a0), int(a1))


def dns_type_name(t: int) -> str:
    """DNSType.String() (dns.go:77-124)."""
    return DNS_TYPE_NAMES.get(int(t), "Unknown")


def dns_class_name(c: int) -> str:
    """DNSClass.String() (dns.go:32-48)."""
    return DNS_CLASS_NAMES.get(int(c), "Unknown")


def dns_response_code_name(c: int) -> str:
    """DNSResponseCode.String() (dns.go:151-195)."""
    return DNS_RCODE_NAMES.get(int(c), "Unknown")


def dns_opcode_name(c: int) -> str:
    """DNSOpCode.String() (dns.go:208-225)."""
    return DNS_OPCODE_NAMES.get(int(c), "Unknown")


class DNSDecodeError(Exception):
    """The error (*DNS).DecodeFromBytes returned; str() is the reference's err.Error()."""

    def __init__(self, code: int, arg0: int = 0, arg1: int = 0):
        self.code, self.arg0, self.arg1 = int(code), int(arg0), int(arg1)
        super().__init__(error_text(code, arg0, arg1))

    def Error(self) -> str:
        return str(self)


def decode_host(data, max_work: int = 0, caps=None):
    """One message in host memory through gpd_dns_decode_host (no device): (msg, entries, names,
    counts) with msg a MSG_DTYPE[1] array, entries ENTRY_DTYPE[], names bytes and counts a dict.
    caps None sizes the arrays with a first call; (cap_entries, cap_names) are passed as given,
    and a short one raises GpdError with the needs in its `counts` attribute."""
    buf = np.frombuffer(bytes(data), np.uint8)
    msg = np.zeros(1, MSG_DTYPE)
    cnt = GpdDnsCounts()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    lib = dns_lib()
    if caps is None:
        lib.gpd_dns_decode_host(ptr(buf), len(buf), max_work, ptr(msg), None, 0, None, 0, C.byref(cnt))
        caps = (int(cnt.entries), int(cnt.name_bytes))
    ents = np.zeros(caps[0], ENTRY_DTYPE)
    names = np.zeros(caps[1], np.uint8)
    rc = lib.gpd_dns_decode_host(ptr(buf), len(buf), max_work, ptr(msg), ptr(ents), caps[0], ptr(names), caps[1],
                                 C.byref(cnt))
    counts = {k: int(getattr(cnt, k)) for k, _ in GpdDnsCounts._fields_}
    if rc != 0:
        try:
            check(rc, "gpd_dns_decode_host")
        except _lib.GpdError as e:
            e.counts = counts
            raise
    return msg, ents[:counts["entries"]], names[:counts["name_bytes"]].tobytes(), counts


# ---------------------------------------------------------------- the reference's objects
class DNSQuestion:
    def __init__(self, Name=b"", Type=0, Class=0):
        self.Name, self.Type, self.Class = Name, Type, Class


class DNSSOA:
    def __init__(self):
        self.MName = self.RName = b""
        self.Serial = self.Refresh = self.Retry = self.Expire = self.Minimum = 0


class DNSSRV:
    def __init__(self):
        self.Priority = self.Weight = self.Port = 0
        self.Name = b""


class DNSMX:
    def __init__(self):
        self.Preference, self.Name = 0, b""


class DNSURI:
    def __init__(self):
        self.Priority = self.Weight = 0
        self.Target = b""


class DNSOPT:
    def __init__(self, Code, Data):
        self.Code, self.Data = Code, Data


class DNSResourceRecord:
    def __init__(self):
        self.Name, self.Type, self.Class, self.TTL, self.DataLength, self.Data = b"", 0, 0, 0, 0, b""
        self.IP = None
        self.NS = self.CNAME = self.PTR = b""
        self.TXTs = None
        self.TXT = None
        self.SOA, self.SRV, self.MX, self.URI = DNSSOA(), DNSSRV(), DNSMX(), DNSURI()
        self.OPT = None


class DNS:
    """layers.DNS as DecodeFromBytes leaves it (dns.go:255-285), with `err` the error it returned
    (None: nil), `truncated`, and `packet`, the index of its packet in the batch."""

    def __init__(self):
        self.ID = 0
        self.QR = self.AA = self.TC = self.RD = self.RA = False
        self.OpCode = self.Z = self.ResponseCode = 0
        self.QDCount = self.ANCount = self.NSCount = self.ARCount = 0
        self.Questions, self.Answers, self.Authorities, self.Additionals = [], [], [], []
        self.err = None
        self.truncated = False
        self.packet = 0
        self.Contents = b""


def _record(e, data: bytes, names: bytes):
    """One entry as the reference's object; the slices of rr.Data are read here."""
    o = int(e["name_off"])
    name = names[o:o + int(e["name_len"])]
    if int(e["section"]) == SEC_QUESTION:
        return DNSQuestion(name, int(e["type"]), int(e["klass"]))
    r = DNSResourceRecord()
    r.Name, r.Type, r.Class, r.TTL, r.DataLength = name, int(e["type"]), int(e["klass"]), int(e["ttl"]), int(e["rdlength"])
    off = int(e["rdata_off"])
    r.Data = data[off:off + r.DataLength]
    if r.DataLength == 0:  # dns.go:731: decodeRData is skipped
        return r
    o += int(e["name_len"])
    n1 = names[o:o + int(e["rname1_len"])]
    n2 = names[o + int(e["rname1_len"]):o + int(e["rname1_len"]) + int(e["rname2_len"])]
    t = r.Type
    if t in (DNSTypeA, DNSTypeAAAA):
        r.IP = r.Data
    elif t in (DNSTypeTXT, DNSTypeHINFO):
        r.TXT, r.TXTs, i = r.Data, [], 0
        while i != len(r.Data):  # (validated on the device: every string lies inside)
            r.TXTs.append(r.Data[i + 1:i + 1 + r.Data[i]])
            i += 1 + r.Data[i]
    elif t == DNSTypeNS:
        r.NS = n1
    elif t == DNSTypeCNAME:
        r.CNAME = n1
    elif t == DNSTypePTR:
        r.PTR = n1
    elif t == DNSTypeSOA:
        r.SOA.MName, r.SOA.RName = n1, n2
        (r.SOA.Serial, r.SOA.Refresh, r.SOA.Retry, r.SOA.Expire,
         r.SOA.Minimum) = struct.unpack_from(">5I", data, int(e["fixed_off"]))
    elif t == DNSTypeMX:
        r.MX.Preference, r.MX.Name = struct.unpack_from(">H", r.Data, 0)[0], n1
    elif t == DNSTypeURI:
        r.URI.Priority, r.URI.Weight = struct.unpack_from(">2H", r.Data, 0)
        r.URI.Target = r.Data[4:]
    elif t == DNSTypeSRV:
        r.SRV.Priority, r.SRV.Weight, r.SRV.Port = struct.unpack_from(">3H", r.Data, 0)
        r.SRV.Name = n1
    elif t == DNSTypeOPT:
        r.OPT, i = [], 0
        while i < len(r.Data):
            code, ln = struct.unpack_from(">2H", r.Data, i)
            r.OPT.append(DNSOPT(code, r.Data[i + 4:i + 4 + ln]))
            i += 4 + ln
    return r


def materialize(m, entries, names: bytes, data: bytes) -> DNS:
    """The DNS object of one message record `m` (its entries[first_entry..] in `entries`)."""
    d = DNS()
    d.packet = int(m["packet"])
    v = int(m["verdict"])
    if v == DNS_DEFERRED:
        raise ValueError("materialize: a deferred message has no entries; decode it with decode_host")
    d.truncated = bool(m["truncated"])
    if v != DNS_OK:
        d.err = DNSDecodeError(v, int(m["err_arg0"]), int(m["err_arg1"]))
    if v == DNS_E_TOO_SHORT:
        return d
    f = int(m["flags"])
    d.Contents = data
    d.ID = int(m["id"])
    d.QR, d.OpCode, d.AA, d.TC, d.RD = bool(f & 0x8000), (f >> 11) & 0xF, bool(f & 0x0400), bool(f & 0x0200), bool(f & 0x0100)
    d.RA, d.Z, d.ResponseCode = bool(f & 0x80), (f >> 4) & 7, int(m["rcode"])
    d.QDCount, d.ANCount, d.NSCount, d.ARCount = int(m["qdcount"]), int(m["ancount"]), int(m["nscount"]), int(m["arcount"])
    k = int(m["first_entry"])
    for lst, n in ((d.Questions, m["n_q"]), (d.Answers, m["n_an"]), (d.Authorities, m["n_ns"]),
                   (d.Additionals, m["n_ar"])):
        for _ in range(int(n)):
            lst.append(_record(entries[k], data, names))
            k += 1
    return d


def decode_bytes(data) -> DNS:
    """(*DNS).DecodeFromBytes of one message in host memory (the host walker, no budget)."""
    data = bytes(data)
    msg, ents, names, _ = decode_host(data, 0)
    return materialize(msg[0], ents, names, data)


class DNSResult:
    """gpd_dns_decode's arrays on the device: `msgs` (count x 48 B), `entries` (n_entries x 32 B)
    and `names`, uint8 tensors; `count`, `n_entries`, `name_bytes` and `deferred`."""

    def __init__(self, dbatch, msgs, entries, names, counts, max_work):
        self._dbatch = dbatch
        self.msgs, self.entries, self.names = msgs, entries, names
        self.count, self.n_entries = counts["msgs"], counts["entries"]
        self.name_bytes, self.deferred = counts["name_bytes"], counts["deferred"]
        self.max_work = max_work

    def to_host(self):
        """(MSG_DTYPE[count], ENTRY_DTYPE[n_entries], names bytes) copies."""
        m = self.msgs[:self.count * MSG_DTYPE.itemsize].cpu().numpy().view(MSG_DTYPE).copy()
        e = self.entries[:self.n_entries * ENTRY_DTYPE.itemsize].cpu().numpy().view(ENTRY_DTYPE).copy()
        return m, e, self.names[:self.name_bytes].cpu().numpy().tobytes()

    def message_bytes(self, msgs=None):
        """`data` of every candidate, gathered on the device and copied once: a list of bytes."""
        from .parser import _torch
        torch = _torch()
        if msgs is None:
            msgs = self.to_host()[0]
        if len(msgs) == 0:
            return []
        db = self._dbatch
        dev = db.data.device
        pk = torch.from_numpy(msgs["packet"].astype(np.int64)).to(dev)
        lens = torch.from_numpy(msgs["data_len"].astype(np.int64)).to(dev)
        start = (db.offset.to(torch.int64) & 0xFFFFFFFF)[pk] + torch.from_numpy(msgs["data_off"].astype(np.int64)).to(dev)
        ends = torch.cumsum(lens, 0)
        total = int(ends[-1])
        src = torch.repeat_interleave(start - (ends - lens), lens) + torch.arange(total, device=dev)
        flat = db.data[src].cpu().numpy().tobytes()
        e = ends.cpu().numpy()
        return [flat[int(b) - int(n):int(b)] for b, n in zip(e, msgs["data_len"])]

    def messages(self):
        """One DNS object per candidate, in packet order, as the reference leaves it.  Deferred
        messages are decoded by the host walker."""
        msgs, ents, names = self.to_host()
        datas = self.message_bytes(msgs)
        out = []
        for m, data in zip(msgs, datas):
            if int(m["verdict"]) == DNS_DEFERRED:
                d = decode_bytes(data)
                d.packet = int(m["packet"])
            else:
                d = materialize(m, ents, names, data)
            out.append(d)
        return out


def _call(parser, dbatch, dres, max_work, msgs, entries, names, caps, stream):
    b, r = dbatch.c_batch(), dres.c_result()
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    cfg = GpdDnsConfig(max_work, 0)
    out = GpdDnsOut(p(msgs), caps[0], p(entries), caps[1], p(names), caps[2])
    cnt = GpdDnsCounts()
    rc = dns_lib().gpd_dns_decode(parser.ctx().h, C.byref(b), C.byref(r), C.byref(cfg), C.byref(out), C.byref(cnt),
                                  C.c_void_p(stream.cuda_stream))
    return rc, {k: int(getattr(cnt, k)) for k, _ in GpdDnsCounts._fields_}


def DecodeDNS(parser, dbatch, dres, max_work: int = MAX_WORK_DEFAULT, stream=None, caps=None) -> DNSResult:
    """layers.DNS for every packet of the batch `parser` decoded into `dres` (hdr_off required)
    whose decode stopped at LayerTypeDNS.  The sizing call and the exact allocation happen here;
    caps (cap_msgs, cap_entries, cap_names) skips the sizing call and raises GpdError, with the
    needs in its `counts` attribute, when one is short.  Synchronises `stream`."""
    from .parser import _torch
    torch = _torch()
    if dres.hdr_off is None:
        raise ValueError("DecodeDNS needs a DeviceResult with hdr_off")
    dev = torch.device("cuda", parser.device)
    s = stream if stream is not None else torch.cuda.current_stream(parser.device)
    if caps is None:
        rc, counts = _call(parser, dbatch, dres, max_work, None, None, None, (0, 0, 0), s)
        if rc != 0 and not (counts["msgs"] or counts["entries"] or counts["name_bytes"]):
            check(rc, "gpd_dns_decode")
        caps = (counts["msgs"], counts["entries"], counts["name_bytes"])
        if rc == 0:  # no candidate at all
            z = torch.empty(0, dtype=torch.uint8, device=dev)
            return DNSResult(dbatch, z, z, z, counts, max_work)
    caps = tuple(int(c) for c in caps)
    msgs = torch.empty(max(caps[0], 1) * MSG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    entries = torch.empty(max(caps[1], 1) * ENTRY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    names = torch.empty(max(caps[2], 1), dtype=torch.uint8, device=dev)
    rc, counts = _call(parser, dbatch, dres, max_work, msgs, entries, names, caps, s)
    if rc != 0:
        try:
            check(rc, "gpd_dns_decode")
        except _lib.GpdError as e:
            e.counts = counts
            raise
    return DNSResult(dbatch, msgs[:counts["msgs"] * MSG_DTYPE.itemsize],
                     entries[:counts["entries"] * ENTRY_DTYPE.itemsize], names[:counts["name_bytes"]], counts, max_work)
