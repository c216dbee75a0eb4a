"""TLS record decode: layers.TLS for a decoded device batch and for reassembled TCP streams, on
the GPU.

layers/ports.go:64-73 send TCP 443, 636, 989, 990, 992-995 and 5061 to LayerTypeTLS, which the
engine carries as a stop type: a TLS packet's `decoded` ends at TCP.  `DecodeTLS` runs
(*TLS).DecodeFromBytes (layers/tls.go:118-194) for every such packet of an HBM-resident batch the
parser just decoded (gpd_tls_decode, include/gpd_tls.h): one message record and one 16-byte entry
per appended record.  Records span segments, so `DecodeTLSRanges` runs the same walk over byte
ranges of a device buffer and `DecodeTLSStreams` over the streams `tcpstream.TCPStreams` (or the
stateful assembler) gathered, where they lie.  `messages()` builds the reference's objects; a
message whose work exceeds the budget comes back deferred and is decoded by the host walker
(gpd_tls_decode_host, the same code), so the caller sees the reference's result for every message.

The entry points are bound onto the loaded library here, on first use, from TLS_EXPORTS.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import GpdBatch, GpdResult, check

MSG_DTYPE = np.dtype([("packet", "<u4"), ("data_off", "<u4"), ("data_len", "<u4"), ("first_record", "<u4"),
                      ("n_ccs", "<u4"), ("n_handshake", "<u4"), ("n_appdata", "<u4"), ("n_alert", "<u4"),
                      ("contents_off", "<u4"), ("err_off", "<u4"), ("verdict", "u1"), ("truncated", "u1"),
                      ("reserved", "u1", (6,))])
REC_DTYPE = np.dtype([("off", "<u4"), ("version", "<u2"), ("length", "<u2"), ("index_in_kind", "<u4"),
                      ("content_type", "u1"), ("a", "u1"), ("b", "u1"), ("flags", "u1")])
assert MSG_DTYPE.itemsize == 48 and REC_DTYPE.itemsize == 16

(TLS_OK, TLS_E_TOO_SHORT, TLS_E_UNKNOWN_TYPE, TLS_E_LENGTH_MISMATCH, TLS_E_CCS_LENGTH, TLS_E_ALERT_SHORT,
 TLS_E_APPDATA_LENGTH, TLS_E_COUNT) = range(8)
TLS_DEFERRED = 255
MAX_RECORDS_DEFAULT, MAX_RECORDS_LIMIT = 1024, 1 << 20
REC_ENCRYPTED = 1
# messages one block of the compaction and of the count scan takes, and block sums one round of
# their scan takes (gpd_compact.h kCompactBlock, compact_scan)
COMPACT_BLOCK = 2048
SCAN_ROUND = 1024

TLSChangeCipherSpec, TLSAlert, TLSHandshake, TLSApplicationData, TLSUnknown = 20, 21, 22, 23, 255
TLSChangecipherspecMessage, TLSChangecipherspecUnknown = 1, 255
TLSAlertWarning, TLSAlertFatal, TLSAlertUnknownLevel, TLSAlertUnknownDescription = 1, 2, 255, 255

# verdict -> the reference's error text (tls.go:133,147,154, tls_cipherspec.go:45, tls_alert.go:82,
# tls_appdata.go:29)
ERROR_TEXTS = {
    1: "TLS record too short",
    2: "Unknown TLS record type",
    3: "TLS packet length mismatch",
    4: "TLS Change Cipher Spec record incorrect length",
    5: "TLS Alert packet too short",
    6: "TLS Application Data length mismatch",
}

# the String() names (tls.go:29-65, tls_alert.go:98-165); data only
TLS_TYPE_NAMES = {20: "Change Cipher Spec", 21: "Alert", 22: "Handshake", 23: "Application Data"}
TLS_VERSION_NAMES = {0x0200: "SSL 2.0", 0x0300: "SSL 3.0", 0x0301: "TLS 1.0", 0x0302: "TLS 1.1", 0x0303: "TLS 1.2",
                     0x0304: "TLS 1.3"}
TLS_ALERT_LEVEL_NAMES = {1: "Warning", 2: "Fatal"}
TLS_ALERT_DESCR_NAMES = {
    0: "close_notify", 10: "unexpected_message", 20: "bad_record_mac", 21: "decryption_failed_RESERVED",
    22: "record_overflow", 30: "decompression_failure", 40: "handshake_failure", 41: "no_certificate_RESERVED",
    42: "bad_certificate", 43: "unsupported_certificate", 44: "certificate_revoked", 45: "certificate_expired",
    46: "certificate_unknown", 47: "illegal_parameter", 48: "unknown_ca", 49: "access_denied", 50: "decode_error",
    51: "decrypt_error", 60: "export_restriction_RESERVED", 70: "protocol_version", 71: "insufficient_security",
    80: "internal_error", 90: "user_canceled", 100: "no_renegotiation", 110: "unsupported_extension"}


class TLSType:
    @staticmethod
    def String(t: int) -> str:
        """TLSType.String() (tls.go:29-42)."""
        return TLS_TYPE_NAMES.get(int(t), "Unknown")


class TLSVersion:
    @staticmethod
    def String(v: int) -> str:
        """TLSVersion.String() (tls.go:48-65)."""
        return TLS_VERSION_NAMES.get(int(v), "Unknown")


class TLSAlertLevel:
    @staticmethod
    def String(v: int) -> str:
        """TLSAlertLevel.String() (tls_alert.go:98-107)."""
        return TLS_ALERT_LEVEL_NAMES.get(int(v), f"Unknown({int(v)})")


class TLSAlertDescr:
    @staticmethod
    def String(v: int) -> str:
        """TLSAlertDescr.String() (tls_alert.go:110-165)."""
        return TLS_ALERT_DESCR_NAMES.get(int(v), "Unknown")


class GpdTlsConfig(C.Structure):
    _fields_ = [("max_records", C.c_uint32), ("reserved", C.c_uint32)]


class GpdTlsOut(C.Structure):
    _fields_ = [("msgs", C.c_void_p), ("cap_msgs", C.c_uint64), ("recs", C.c_void_p), ("cap_recs", C.c_uint64)]


class GpdTlsCounts(C.Structure):
    _fields_ = [("msgs", C.c_uint64), ("records", C.c_uint64), ("deferred", C.c_uint64), ("work", C.c_uint64)]


class GpdTlsRanges(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("nbytes", C.c_uint64), ("off", C.c_void_p), ("len", C.c_void_p),
                ("n", C.c_uint64)]


TLS_EXPORTS = {
    # include/gpd_tls.h — name: (restype, argtypes)
    "gpd_tls_decode": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.POINTER(GpdResult), C.POINTER(GpdTlsConfig),
                                 C.POINTER(GpdTlsOut), C.POINTER(GpdTlsCounts), C.c_void_p]),
    "gpd_tls_decode_ranges": (C.c_int, [C.c_void_p, C.POINTER(GpdTlsRanges), C.POINTER(GpdTlsConfig),
                                        C.POINTER(GpdTlsOut), C.POINTER(GpdTlsCounts), C.c_void_p]),
    "gpd_tls_decode_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.POINTER(GpdTlsCounts)]),
}

_bound = False


def tls_lib():
    """The loaded library with the TLS signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in TLS_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


def error_text(verdict: int) -> str:
    return ERROR_TEXTS.get(int(verdict), f"gpd: unknown TLS verdict {verdict}")


class TLSDecodeError(Exception):
    """The error (*TLS).DecodeFromBytes returned; str() is the reference's err.Error()."""

    def __init__(self, code: int):
        self.code = int(code)
        super().__init__(error_text(code))

    def Error(self) -> str:
        return str(self)


def _counts(cnt):
    return {k: int(getattr(cnt, k)) for k, _ in GpdTlsCounts._fields_}


def _raise_with_counts(rc, who, counts):
    try:
        check(rc, who)
    except _lib.GpdError as e:
        e.counts = counts
        raise


def decode_host(data, max_records: int = 0, cap_recs=None):
    """One message in host memory through gpd_tls_decode_host (no device): (msg, recs, counts) with
    msg a MSG_DTYPE[1] array, recs REC_DTYPE[] and counts a dict.  cap_recs None sizes the array
    with a first call; otherwise it is passed as given, and a short one raises GpdError with the
    need in its `counts` attribute."""
    buf = np.frombuffer(bytes(data), np.uint8)
    msg = np.zeros(1, MSG_DTYPE)
    cnt = GpdTlsCounts()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    lib = tls_lib()
    if cap_recs is None:
        lib.gpd_tls_decode_host(ptr(buf), len(buf), max_records, ptr(msg), None, 0, C.byref(cnt))
        cap_recs = int(cnt.records)
    recs = np.zeros(cap_recs, REC_DTYPE)
    rc = lib.gpd_tls_decode_host(ptr(buf), len(buf), max_records, ptr(msg), ptr(recs), cap_recs, C.byref(cnt))
    counts = _counts(cnt)
    if rc != 0:
        _raise_with_counts(rc, "gpd_tls_decode_host", counts)
    return msg, recs[:counts["records"]], counts


# ---------------------------------------------------------------- the reference's objects
class TLSRecordHeader:
    """TLSRecordHeader (tls.go:95-99); TLSHandshakeRecord is this alone (tls_handshake.go:14-16)."""

    def __init__(self, ContentType=0, Version=0, Length=0):
        self.ContentType, self.Version, self.Length = ContentType, Version, Length

    def _key(self):
        return (self.ContentType, self.Version, self.Length)


class TLSHandshakeRecord(TLSRecordHeader):
    pass


class TLSChangeCipherSpecRecord(TLSRecordHeader):
    Message = 0

    def _key(self):
        return super()._key() + (self.Message,)


class TLSAppDataRecord(TLSRecordHeader):
    Payload = b""

    def _key(self):
        return super()._key() + (self.Payload,)


class TLSAlertRecord(TLSRecordHeader):
    Level = Description = 0
    EncryptedMsg = None

    def _key(self):
        return super()._key() + (self.Level, self.Description, self.EncryptedMsg)


class TLS:
    """layers.TLS as DecodeFromBytes leaves it (tls.go:84-92), with `err` the error it returned
    (None: nil), `truncated`, and `packet`, the index of its packet (or range)."""

    def __init__(self):
        self.Contents = b""
        self.ChangeCipherSpec, self.Handshake, self.AppData, self.Alert = [], [], [], []
        self.err = None
        self.truncated = False
        self.packet = 0


def materialize(m, recs, data: bytes) -> TLS:
    """The TLS object of one message record `m` (its recs[first_record..] in `recs`)."""
    t = TLS()
    t.packet = int(m["packet"])
    v = int(m["verdict"])
    if v == TLS_DEFERRED:
        raise ValueError("materialize: a deferred message has no entries; decode it with decode_host")
    t.truncated = bool(m["truncated"])
    if v != TLS_OK:
        t.err = TLSDecodeError(v)
    t.Contents = data[int(m["contents_off"]):]
    k = int(m["first_record"])
    n = int(m["n_ccs"]) + int(m["n_handshake"]) + int(m["n_appdata"]) + int(m["n_alert"])
    for r in recs[k:k + n]:
        ct, off, length = int(r["content_type"]), int(r["off"]), int(r["length"])
        body = data[off + 5:off + 5 + length]
        if ct == TLSChangeCipherSpec:
            o, lst = TLSChangeCipherSpecRecord(), t.ChangeCipherSpec
            o.Message = int(r["a"])
        elif ct == TLSAlert:
            o, lst = TLSAlertRecord(), t.Alert
            o.Level, o.Description = int(r["a"]), int(r["b"])
            if int(r["flags"]) & REC_ENCRYPTED:
                o.EncryptedMsg = body
        elif ct == TLSHandshake:
            o, lst = TLSHandshakeRecord(), t.Handshake
        else:
            o, lst = TLSAppDataRecord(), t.AppData
            o.Payload = body
        o.ContentType, o.Version, o.Length = ct, int(r["version"]), length
        assert len(lst) == int(r["index_in_kind"])
        lst.append(o)
    return t


def decode_bytes(data) -> TLS:
    """(*TLS).DecodeFromBytes of one message in host memory (the host walker, no budget)."""
    data = bytes(data)
    msg, recs, _ = decode_host(data, 0)
    return materialize(msg[0], recs, data)


class TLSResult:
    """The decode's arrays on the device: `msgs` (count x 48 B) and `recs` (n_records x 16 B),
    uint8 tensors; `count`, `n_records` and `deferred`."""

    def __init__(self, source, msgs, recs, counts, max_records):
        self._source = source  # ("batch", DeviceBatch) or ("ranges", bytes tensor, off tensor)
        self.msgs, self.recs = msgs, recs
        self.count, self.n_records, self.deferred = counts["msgs"], counts["records"], counts["deferred"]
        self.max_records = max_records

    def to_host(self):
        """(MSG_DTYPE[count], REC_DTYPE[n_records]) copies."""
        m = self.msgs[:self.count * MSG_DTYPE.itemsize].cpu().numpy().view(MSG_DTYPE).copy()
        r = self.recs[:self.n_records * REC_DTYPE.itemsize].cpu().numpy().view(REC_DTYPE).copy()
        return m, r

    def message_bytes(self, msgs=None):
        """`data` of every message, gathered on the device and copied once: a list of bytes.
        dhcp.py's DHCPResult uses this function as its own: it may read `_source` (as the "batch"
        form) and `to_host()[0]` (`packet`, `data_off`, `data_len`) of `self`, and nothing else."""
        from .parser import _torch
        torch = _torch()
        if msgs is None:
            msgs = self.to_host()[0]
        if len(msgs) == 0:
            return []
        if self._source[0] == "batch":
            db = self._source[1]
            data, dev = db.data, db.data.device
            pk = torch.from_numpy(msgs["packet"].astype(np.int64)).to(dev)
            start = (db.offset.to(torch.int64) & 0xFFFFFFFF)[pk] + \
                torch.from_numpy(msgs["data_off"].astype(np.int64)).to(dev)
        else:
            data, off = self._source[1], self._source[2]
            dev = data.device
            start = off.to(torch.int64)[torch.from_numpy(msgs["packet"].astype(np.int64)).to(dev)]
        lens = torch.from_numpy(msgs["data_len"].astype(np.int64)).to(dev)
        ends = torch.cumsum(lens, 0)
        total = int(ends[-1])
        if total == 0:
            return [b""] * len(msgs)
        src = torch.repeat_interleave(start - (ends - lens), lens) + torch.arange(total, device=dev)
        flat = data[src].cpu().numpy().tobytes()
        e = ends.cpu().numpy()
        return [flat[int(b) - int(n):int(b)] for b, n in zip(e, msgs["data_len"])]

    def messages(self):
        """One TLS object per message, in order, as the reference leaves it.  Deferred messages are
        decoded by the host walker."""
        msgs, recs = self.to_host()
        datas = self.message_bytes(msgs)
        out = []
        for m, data in zip(msgs, datas):
            if int(m["verdict"]) == TLS_DEFERRED:
                t = decode_bytes(data)
                t.packet = int(m["packet"])
            else:
                t = materialize(m, recs, data)
            out.append(t)
        return out


def _run(call, who, source, dev, max_records, caps):
    """The sizing call and the exact allocation around `call(msgs, recs, caps) -> (rc, counts)`."""
    from .parser import _torch
    torch = _torch()
    if caps is None:
        rc, counts = call(None, None, (0, 0))
        if rc != 0 and not (counts["msgs"] or counts["records"]):
            check(rc, who)
        caps = (counts["msgs"], counts["records"])
        if rc == 0:  # no message at all
            z = torch.empty(0, dtype=torch.uint8, device=dev)
            return TLSResult(source, z, z, counts, max_records)
    caps = tuple(int(c) for c in caps)
    msgs = torch.empty(max(caps[0], 1) * MSG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    recs = torch.empty(max(caps[1], 1) * REC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rc, counts = call(msgs, recs, caps)
    if rc != 0:
        _raise_with_counts(rc, who, counts)
    return TLSResult(source, msgs[:counts["msgs"] * MSG_DTYPE.itemsize],
                     recs[:counts["records"] * REC_DTYPE.itemsize], counts, max_records)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def DecodeTLS(parser, dbatch, dres, max_records: int = MAX_RECORDS_DEFAULT, stream=None, caps=None) -> TLSResult:
    """layers.TLS for every packet of the batch `parser` decoded into `dres` (hdr_off required)
    whose decode stopped at LayerTypeTLS.  The sizing call and the exact allocation happen here;
    caps (cap_msgs, cap_recs) skips the sizing call and raises GpdError, with the needs in its
    `counts` attribute, when one is short.  Synchronises `stream`."""
    from .parser import _torch
    torch = _torch()
    if dres.hdr_off is None:
        raise ValueError("DecodeTLS needs a DeviceResult with hdr_off")
    dev = torch.device("cuda", parser.device)
    s = stream if stream is not None else torch.cuda.current_stream(parser.device)
    b, r = dbatch.c_batch(), dres.c_result()
    cfg = GpdTlsConfig(int(max_records) if 0 <= int(max_records) < 1 << 32 else 0, 0)

    def call(msgs, recs, caps):
        out = GpdTlsOut(_ptr(msgs), caps[0], _ptr(recs), caps[1])
        cnt = GpdTlsCounts()
        rc = tls_lib().gpd_tls_decode(parser.ctx().h, C.byref(b), C.byref(r), C.byref(cfg), C.byref(out),
                                      C.byref(cnt), C.c_void_p(s.cuda_stream))
        return rc, _counts(cnt)

    return _run(call, "gpd_tls_decode", ("batch", dbatch), dev, max_records, caps)


def DecodeTLSRanges(parser, bytes_tensor, off, length, max_records: int = MAX_RECORDS_DEFAULT, stream=None,
                    caps=None) -> TLSResult:
    """The same decode over byte ranges of one device buffer: range k is
    bytes_tensor[off[k] : off[k] + length[k]] (off int64 / uint64, length int32 / uint32 device
    tensors of n elements).  Every range is one message; `packet` of its record is k.  A range
    that passes the buffer raises GpdError and nothing is written."""
    from .parser import _torch
    torch = _torch()
    dev = torch.device("cuda", parser.device)
    s = stream if stream is not None else torch.cuda.current_stream(parser.device)
    if bytes_tensor.dtype != torch.uint8 or not bytes_tensor.is_contiguous():
        raise ValueError("DecodeTLSRanges: bytes_tensor must be a contiguous uint8 tensor")
    if off.element_size() != 8 or length.element_size() != 4 or off.numel() != length.numel():
        raise ValueError("DecodeTLSRanges: off must hold 64-bit and length 32-bit integers, one each a range")
    off, length = off.contiguous(), length.contiguous()
    rg = GpdTlsRanges(_ptr(bytes_tensor), bytes_tensor.numel(), _ptr(off), _ptr(length), off.numel())
    cfg = GpdTlsConfig(int(max_records) if 0 <= int(max_records) < 1 << 32 else 0, 0)

    def call(msgs, recs, caps):
        out = GpdTlsOut(_ptr(msgs), caps[0], _ptr(recs), caps[1])
        cnt = GpdTlsCounts()
        rc = tls_lib().gpd_tls_decode_ranges(parser.ctx().h, C.byref(rg), C.byref(cfg), C.byref(out), C.byref(cnt),
                                             C.c_void_p(s.cuda_stream))
        return rc, _counts(cnt)

    return _run(call, "gpd_tls_decode_ranges", ("ranges", bytes_tensor, off), dev, max_records, caps)


def DecodeTLSStreams(parser, stream_result, max_records: int = MAX_RECORDS_DEFAULT, stream=None,
                     caps=None) -> TLSResult:
    """The same decode over the gathered streams of `tcpstream.TCPStreams` (a StreamResult) or of
    the stateful assembler (its result has the same `streams` / `bytes` fields): one message per
    48-byte stream record, its bytes[byte_off : byte_off + nbytes], read where they lie.  The
    ranges are built on the device.  Raises for a stream of 2^32 bytes or more."""
    from .parser import _torch
    torch = _torch()
    if stream_result.bytes is None:
        raise ValueError("DecodeTLSStreams needs gathered stream bytes (gather=True)")
    n = int(stream_result.nstreams)
    words = stream_result.streams[:n * 48].view(torch.int64).view(n, 6)  # STREAM_DTYPE: byte_off, nbytes at 16, 24
    off, nbytes = words[:, 2].contiguous(), words[:, 3]
    # the streams lie back to back in `bytes`: below 2^32 in all, none can reach it (no read-back)
    if int(stream_result.nbytes) >= 1 << 32 and n and bool(((nbytes < 0) | (nbytes >= 1 << 32)).any()):
        raise ValueError("DecodeTLSStreams: a stream of 2^32 bytes or more")
    # the low words of nbytes (little endian), as the 32-bit lengths
    length = nbytes.contiguous().view(torch.int32).view(n, 2)[:, 0].contiguous()
    return DecodeTLSRanges(parser, stream_result.bytes, off, length, max_records, stream, caps)
