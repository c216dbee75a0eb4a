"""layers/dns.go's decode restated line by line (paths and line numbers of google/gopacket):
(*DNS).DecodeFromBytes :304-392, decodeName :538-627 (recursive, with the shared buffer, as the
reference writes it), DNSQuestion.decode :636-651, DNSResourceRecord.decode :710-738,
decodeCharacterStrings :864-875, decodeOPTs :877-904, decodeRData :906-993.

It is the model of gpd_dns_decode / gpd_dns_decode_host (include/gpd_dns.h): `decode` returns the
reference's DNS object with the error the call returned, and `work`, the step count the work
budget is defined on.  `records` flattens a DNS object into the ABI's three arrays."""
from __future__ import annotations

import struct
import sys

import numpy as np

sys.setrecursionlimit(max(sys.getrecursionlimit(), 5000))  # decodeName recurses 255 levels deep

MSG_DTYPE = np.dtype([("packet", "<u4"), ("data_off", "<u4"), ("data_len", "<u4"), ("id", "<u2"), ("flags", "<u2"),
                      ("qdcount", "<u2"), ("ancount", "<u2"), ("nscount", "<u2"), ("arcount", "<u2"),
                      ("n_q", "<u2"), ("n_an", "<u2"), ("n_ns", "<u2"), ("n_ar", "<u2"),
                      ("rcode", "u1"), ("verdict", "u1"), ("truncated", "u1"), ("reserved", "u1"),
                      ("err_arg0", "<u4"), ("err_arg1", "<u4"), ("first_entry", "<u4")])
ENTRY_DTYPE = np.dtype([("name_off", "<u4"), ("name_len", "<u2"), ("rname1_len", "<u2"), ("rname2_len", "<u2"),
                        ("type", "<u2"), ("klass", "<u2"), ("rdlength", "<u2"), ("ttl", "<u4"),
                        ("rdata_off", "<u4"), ("fixed_off", "<u4"), ("section", "u1"), ("reserved", "u1", (3,))])
assert MSG_DTYPE.itemsize == 48 and ENTRY_DTYPE.itemsize == 32

# verdict codes (include/gpd_dns.h) and the texts of dns.go:1089-1107 and the inline errors
(OK, E_TOO_SHORT, E_MAX_RECURSION, E_NAME_OFFSET_HIGH, E_NAME_OFFSET_NEG, E_NAME_TOO_LONG, E_NAME_INVALID_INDEX,
 E_POINTER_HIGH, E_INDEX_RANGE, E_NAME_NO_DATA, E_LABEL_40, E_LABEL_80, E_QUESTION_SMALL, E_RECORD_SMALL,
 E_RECORD_LENGTH, E_CHAR_STRING, E_SOA_SMALL, E_MX_SMALL, E_URI_SMALL, E_SRV_SMALL, E_OPT_SHORT, E_OPT_MALFORMED,
 E_OPT_LENGTH, E_BAD_QDCOUNT, E_BAD_ANCOUNT, E_BAD_NSCOUNT, E_BAD_ARCOUNT) = range(27)
DEFERRED = 255
UNREACHABLE = {E_NAME_OFFSET_NEG, E_NAME_NO_DATA, E_BAD_QDCOUNT, E_BAD_ANCOUNT, E_BAD_NSCOUNT, E_BAD_ARCOUNT}
REACHABLE = set(range(27)) - UNREACHABLE

FORMATS = {
    E_TOO_SHORT: "DNS packet too short",
    E_MAX_RECURSION: "max DNS recursion level hit",
    E_NAME_OFFSET_HIGH: "dns name offset too high",
    E_NAME_OFFSET_NEG: "dns name offset is negative",
    E_NAME_TOO_LONG: "dns name is too long",
    E_NAME_INVALID_INDEX: "dns name uncomputable: invalid index",
    E_POINTER_HIGH: "dns offset pointer too high",
    E_INDEX_RANGE: "dns index walked out of range",
    E_NAME_NO_DATA: "no dns data found for name",
    E_LABEL_40: "qname '0x40' - RFC 2673 unsupported yet (data={0:x} index={1})",
    E_LABEL_80: "qname '0x80' unsupported yet (data={0:x} index={1})",
    E_QUESTION_SMALL: "DNS question too small",
    E_RECORD_SMALL: "DNS record too small",
    E_RECORD_LENGTH: "resource record length exceeds data",
    E_CHAR_STRING: "Insufficient data for a <character-string>",
    E_SOA_SMALL: "SOA too small",
    E_MX_SMALL: "MX too small",
    E_URI_SMALL: "URI too small",
    E_SRV_SMALL: "SRV too small",
    E_OPT_SHORT: "DNSOPT record is of length {0}, it should be at least length 4",
    E_OPT_MALFORMED: "Malformed DNSOPT record.  Length {0} < {1}",
    E_OPT_LENGTH: "Malformed DNSOPT record. The length ({0}) field implies a packet larger than the one received",
    E_BAD_QDCOUNT: "Invalid query decoding, not the right number of questions",
    E_BAD_ANCOUNT: "Invalid query decoding, not the right number of answers",
    E_BAD_NSCOUNT: "Invalid query decoding, not the right number of authorities",
    E_BAD_ARCOUNT: "Invalid query decoding, not the right number of additionals info",
}

(TypeA, TypeNS, TypeCNAME, TypeSOA, TypePTR, TypeHINFO, TypeMX, TypeTXT, TypeAAAA, TypeSRV, TypeOPT,
 TypeURI) = 1, 2, 5, 6, 12, 13, 15, 16, 28, 33, 41, 256


class DNSError(Exception):
    def __init__(self, code, a0=0, a1=0):
        self.code, self.a0, self.a1 = code, a0, a1
        super().__init__(FORMATS[code].format(a0, a1))


class Work:
    def __init__(self):
        self.n = 0


def be16(b, i):
    return struct.unpack_from(">H", b, i)[0]


def be32(b, i):
    return struct.unpack_from(">I", b, i)[0]


def decodeName(data, offset, buffer, level, w):
    """dns.go:538-627; `buffer` is a bytearray (the *[]byte)."""
    w.n += 1                                        # a decodeName call
    if level > 255:                                 # :539
        raise DNSError(E_MAX_RECURSION)
    elif offset >= len(data):                       # :541
        raise DNSError(E_NAME_OFFSET_HIGH)
    elif offset < 0:                                # :543
        raise DNSError(E_NAME_OFFSET_NEG)
    start = len(buffer)
    index = offset
    if data[index] == 0x00:                         # :548
        return b"", index + 1
    while data[index] != 0x00:                      # :552
        w.n += 1                                    # an iteration of its loop
        kind = data[index] & 0xC0
        if kind == 0xC0:                            # :573
            if index + 2 > len(data):               # :593
                raise DNSError(E_POINTER_HIGH)
            offsetp = be16(data, index) & 0x3FFF
            if offsetp > len(data):                 # :597
                raise DNSError(E_POINTER_HIGH)
            decodeName(data, offsetp, buffer, level + 1, w)  # :604
            index += 1                              # :608
            break
        elif kind == 0x40:                          # :611
            raise DNSError(E_LABEL_40, data[index], index)
        elif kind == 0x80:                          # :615
            raise DNSError(E_LABEL_80, data[index], index)
        else:                                       # :554-571
            index2 = index + data[index] + 1
            if index2 - offset > 255:               # :564
                raise DNSError(E_NAME_TOO_LONG)
            elif index2 < index + 1 or index2 > len(data):  # :566
                raise DNSError(E_NAME_INVALID_INDEX)
            buffer += b"."                          # :569
            buffer += data[index + 1:index2]        # :570
            w.n += 1 + (index2 - index - 1)         # bytes appended, the dot included
            index = index2
        if index >= len(data):                      # :619
            raise DNSError(E_INDEX_RANGE)
    if len(buffer) <= start:                        # :623
        return bytes(buffer[start:]), index + 1
    return bytes(buffer[start + 1:]), index + 1     # :626


class Question:
    def __init__(self):
        self.Name, self.Type, self.Class = b"", 0, 0

    def decode(self, data, offset, buffer, w):      # :636-651
        name, endq = decodeName(data, offset, buffer, 1, w)
        if len(data) < endq + 4:
            raise DNSError(E_QUESTION_SMALL)
        self.Name = name
        self.Type = be16(data, endq)
        self.Class = be16(data, endq + 2)
        return endq + 4


class SOA:
    def __init__(self):
        self.MName = self.RName = b""
        self.Serial = self.Refresh = self.Retry = self.Expire = self.Minimum = 0


class ResourceRecord:
    def __init__(self):
        self.Name, self.Type, self.Class, self.TTL = b"", 0, 0, 0
        self.DataLength, self.Data = 0, b""
        self.IP = None
        self.NS = self.CNAME = self.PTR = b""
        self.TXTs = None
        self.SOA = SOA()
        self.SRV = {"Priority": 0, "Weight": 0, "Port": 0, "Name": b""}
        self.MX = {"Preference": 0, "Name": b""}
        self.OPT = None
        self.URI = {"Priority": 0, "Weight": 0, "Target": b""}
        self.TXT = None
        # where the ABI's record finds things (not reference fields)
        self._rdata_off = 0
        self._fixed_off = 0

    def decode(self, data, offset, buffer, w):      # :710-738
        name, endq = decodeName(data, offset, buffer, 1, w)
        if len(data) < endq + 10:
            raise DNSError(E_RECORD_SMALL)
        self.Name = name
        self.Type = be16(data, endq)
        self.Class = be16(data, endq + 2)
        self.TTL = be32(data, endq + 4)
        self.DataLength = be16(data, endq + 8)
        end = endq + 10 + self.DataLength
        if end > len(data):
            raise DNSError(E_RECORD_LENGTH)
        self.Data = bytes(data[endq + 10:end])
        self._rdata_off = endq + 10
        if self.DataLength > 0:
            self.decodeRData(data[:end], endq + 10, buffer, w)   # :732
        return endq + 10 + self.DataLength

    def decodeRData(self, data, offset, buffer, w):  # :906-993
        t = self.Type
        if t == TypeA or t == TypeAAAA:
            self.IP = self.Data
        elif t == TypeTXT or t == TypeHINFO:
            self.TXT = self.Data
            self.TXTs = decodeCharacterStrings(self.Data, w)
        elif t == TypeNS:
            self.NS, _ = decodeName(data, offset, buffer, 1, w)
        elif t == TypeCNAME:
            self.CNAME, _ = decodeName(data, offset, buffer, 1, w)
        elif t == TypePTR:
            self.PTR, _ = decodeName(data, offset, buffer, 1, w)
        elif t == TypeSOA:
            name, endq = decodeName(data, offset, buffer, 1, w)
            self.SOA.MName = name
            name, endq = decodeName(data, endq, buffer, 1, w)
            if len(data) < endq + 20:
                raise DNSError(E_SOA_SMALL)
            self.SOA.RName = name
            (self.SOA.Serial, self.SOA.Refresh, self.SOA.Retry, self.SOA.Expire,
             self.SOA.Minimum) = struct.unpack_from(">5I", data, endq)
            self._fixed_off = endq
        elif t == TypeMX:
            if len(data) < offset + 2:
                raise DNSError(E_MX_SMALL)
            self.MX["Preference"] = be16(data, offset)
            self.MX["Name"], _ = decodeName(data, offset + 2, buffer, 1, w)
        elif t == TypeURI:
            if len(self.Data) < 4:
                raise DNSError(E_URI_SMALL)
            self.URI["Priority"] = be16(data, offset)
            self.URI["Weight"] = be16(data, offset + 2)
            self.URI["Target"] = self.Data[4:]
        elif t == TypeSRV:
            if len(data) < offset + 6:
                raise DNSError(E_SRV_SMALL)
            self.SRV["Priority"] = be16(data, offset)
            self.SRV["Weight"] = be16(data, offset + 2)
            self.SRV["Port"] = be16(data, offset + 4)
            self.SRV["Name"], _ = decodeName(data, offset + 6, buffer, 1, w)
        elif t == TypeOPT:
            self.OPT = decodeOPTs(data, offset, w)


def decodeCharacterStrings(data, w):                # :864-875
    strings = []
    end = len(data)
    index = 0
    while index != end:
        w.n += 1                                    # a character string visited
        index2 = index + 1 + data[index]
        if index2 > end:
            raise DNSError(E_CHAR_STRING)
        strings.append(bytes(data[index + 1:index2]))
        index = index2
    return strings


def decodeOPTs(data, offset, w):                    # :877-904
    allOPT = []
    end = len(data)
    if offset == end:
        return allOPT
    if offset + 4 > end:
        raise DNSError(E_OPT_SHORT, end - offset)
    i = offset
    while i < end:
        w.n += 1                                    # an option visited
        if len(data) < i + 4:
            raise DNSError(E_OPT_MALFORMED, len(data), i + 4)
        code = be16(data, i)
        ln = be16(data, i + 2)
        if i + 4 + ln > end:
            raise DNSError(E_OPT_LENGTH, ln)
        allOPT.append((code, bytes(data[i + 4:i + 4 + ln])))
        i += ln + 4
    return allOPT


class DNS:
    def __init__(self):
        self.ID = 0
        self.QR = self.AA = self.TC = self.RD = self.RA = False
        self.OpCode = self.Z = self.ResponseCode = 0
        self.QDCount = self.ANCount = self.NSCount = self.ARCount = 0
        self.Questions, self.Answers, self.Authorities, self.Additionals = [], [], [], []
        self.err = None        # the error DecodeFromBytes returned
        self.truncated = False
        self.work = 0
        self.flags = 0         # bytes 2..3 (not a reference field)

    def DecodeFromBytes(self, data):                # :304-392
        w = Work()
        try:
            self._decode(bytes(data), w)
        except DNSError as e:
            self.err = e
        self.work = w.n
        return self

    def _decode(self, data, w):
        buffer = bytearray()
        if len(data) < 12:                          # :307
            self.truncated = True
            raise DNSError(E_TOO_SHORT)
        self.ID = be16(data, 0)
        self.QR = data[2] & 0x80 != 0
        self.OpCode = (data[2] >> 3) & 0x0F
        self.AA = data[2] & 0x04 != 0
        self.TC = data[2] & 0x02 != 0
        self.RD = data[2] & 0x01 != 0
        self.RA = data[3] & 0x80 != 0
        self.Z = (data[3] >> 4) & 0x7
        self.ResponseCode = data[3] & 0xF
        self.flags = be16(data, 2)
        self.QDCount, self.ANCount, self.NSCount, self.ARCount = struct.unpack_from(">4H", data, 4)
        offset = 12
        for _ in range(self.QDCount):               # :336-342
            w.n += 1                                # a question begun
            q = Question()
            offset = q.decode(data, offset, buffer, w)
            self.Questions.append(q)
        for sec, count in ((self.Answers, self.ANCount), (self.Authorities, self.NSCount),
                           (self.Additionals, self.ARCount)):   # :356-380
            for _ in range(count):
                w.n += 1                            # a record begun
                r = ResourceRecord()
                offset = r.decode(data, offset, buffer, w)   # (an error strips the erroneous value)
                sec.append(r)
                if sec is self.Additionals and r.Type == TypeOPT:     # :377-379
                    self.ResponseCode = (self.ResponseCode | ((r.TTL >> 20) & 0xF0)) & 0xFF
        if len(self.Questions) & 0xFFFF != self.QDCount:       # :382-389
            raise DNSError(E_BAD_QDCOUNT)
        elif len(self.Answers) & 0xFFFF != self.ANCount:
            raise DNSError(E_BAD_ANCOUNT)
        elif len(self.Authorities) & 0xFFFF != self.NSCount:
            raise DNSError(E_BAD_NSCOUNT)
        elif len(self.Additionals) & 0xFFFF != self.ARCount:
            raise DNSError(E_BAD_ARCOUNT)


def decode(data) -> DNS:
    return DNS().DecodeFromBytes(data)


def rnames(r):
    """The rdata names of a record in the ABI's order."""
    if isinstance(r, Question):
        return b"", b""
    t = r.Type
    if r.DataLength == 0:
        return b"", b""
    n1 = {TypeNS: r.NS, TypeCNAME: r.CNAME, TypePTR: r.PTR, TypeMX: r.MX["Name"], TypeSRV: r.SRV["Name"],
          TypeSOA: r.SOA.MName}.get(t, b"")
    return n1, (r.SOA.RName if t == TypeSOA else b"")


def records(d: DNS, data_len: int, max_work: int = 0, packet: int = 0, data_off: int = 0, first_entry: int = 0,
            name_base: int = 0):
    """The ABI's (msg, entries, names) of a decoded message (include/gpd_dns.h)."""
    m = np.zeros(1, MSG_DTYPE)
    m["packet"], m["data_off"], m["data_len"], m["first_entry"] = packet, data_off, data_len, first_entry
    deferred = max_work and d.work > max_work
    code = d.err.code if d.err else OK
    if code != E_TOO_SHORT:
        m["id"], m["flags"] = d.ID, d.flags
        m["qdcount"], m["ancount"], m["nscount"], m["arcount"] = d.QDCount, d.ANCount, d.NSCount, d.ARCount
    m["truncated"] = d.truncated
    if deferred:
        m["verdict"] = DEFERRED
        m["rcode"] = d.flags & 0xF
        return m, np.zeros(0, ENTRY_DTYPE), b""
    m["verdict"] = code
    m["rcode"] = d.ResponseCode
    if d.err:
        m["err_arg0"], m["err_arg1"] = d.err.a0, d.err.a1
    m["n_q"], m["n_an"], m["n_ns"], m["n_ar"] = len(d.Questions), len(d.Answers), len(d.Authorities), len(d.Additionals)
    ents, names = [], bytearray()
    for sec, lst in enumerate((d.Questions, d.Answers, d.Authorities, d.Additionals)):
        for r in lst:
            e = np.zeros(1, ENTRY_DTYPE)
            n1, n2 = rnames(r)
            e["name_off"], e["name_len"], e["rname1_len"], e["rname2_len"] = name_base + len(names), len(r.Name), len(n1), len(n2)
            e["type"], e["klass"], e["section"] = r.Type, r.Class, sec
            if sec:
                e["rdlength"], e["ttl"], e["rdata_off"], e["fixed_off"] = r.DataLength, r.TTL, r._rdata_off, r._fixed_off
            names += r.Name + n1 + n2
            ents.append(e)
    return m, (np.concatenate(ents) if ents else np.zeros(0, ENTRY_DTYPE)), bytes(names)
