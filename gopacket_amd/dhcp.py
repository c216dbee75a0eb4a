"""DHCP message decode: layers.DHCPv4 and layers.DHCPv6 for a decoded device batch, on the GPU.

layers/ports.go:109-112 send UDP 67 and 68 to LayerTypeDHCPv4 and UDP 546 and 547 to
LayerTypeDHCPv6, which the engine carries as stop types: a DHCP packet's `decoded` ends at UDP.
`DecodeDHCP` runs (*DHCPv4).DecodeFromBytes (layers/dhcpv4.go:126-179) or
(*DHCPv6).DecodeFromBytes (layers/dhcpv6.go:89-124) for every such packet of an HBM-resident batch
the parser just decoded (gpd_dhcp_decode, include/gpd_dhcp.h): one message record and one 8-byte
entry per appended option.  `messages()` builds the reference's objects; a message whose work
exceeds the budget comes back deferred and is decoded by the host walker (gpd_dhcp_decode_host,
the same code), so the caller sees the reference's result for every message.

The entry points are bound onto the loaded library here, on first use, from DHCP_EXPORTS.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import GpdBatch, GpdResult, check
from .tls import TLSResult

MSG_DTYPE = np.dtype([("packet", "<u4"), ("data_off", "<u4"), ("data_len", "<u4"), ("first_opt", "<u4"),
                      ("n_opts", "<u4"), ("xid", "<u4"), ("err_off", "<u4"), ("err_arg", "<u4"),
                      ("secs", "<u2"), ("flags", "<u2"), ("verdict", "u1"), ("truncated", "u1"), ("version", "u1"),
                      ("op", "u1"), ("htype", "u1"), ("hlen", "u1"), ("hops", "u1"), ("mflags", "u1"),
                      ("reserved", "u1", (4,))])
OPT_DTYPE = np.dtype([("off", "<u4"), ("code", "<u2"), ("length", "<u2")])
assert MSG_DTYPE.itemsize == 48 and OPT_DTYPE.itemsize == 8

(DHCP_OK, DHCP_E_V4_TOO_SHORT, DHCP_E_V4_BAD_MAGIC, DHCP_E_V4_OPT_NO_DATA, DHCP_E_V4_OPT_MALFORMED,
 DHCP_E_V6_TOO_SHORT, DHCP_E_V6_RELAY_SHORT, DHCP_E_V6_OPT_NO_DATA, DHCP_E_V6_OPT_SIZE, DHCP_E_V4_OPT_EMPTY,
 DHCP_E_V4_HW_PANIC, DHCP_E_COUNT) = range(12)
DHCP_DEFERRED = 255
MAX_OPTIONS_DEFAULT, MAX_OPTIONS_LIMIT = 2048, 1 << 16
F_CONTENTS, F_RELAY, F_HW_PAST_DATA = 1, 2, 4
LT_DHCPV4, LT_DHCPV6 = 118, 134
# messages one block of the compaction and of the count scan takes, and block sums one round of
# their scan takes (gpd_compact.h kCompactBlock, compact_scan)
COMPACT_BLOCK = 2048
SCAN_ROUND = 1024

DHCPOptPad, DHCPOptEnd = 0, 255
DHCPv6MsgTypeRelayForward, DHCPv6MsgTypeRelayReply = 12, 13
DHCPMagic = 0x63825363

# verdict -> the reference's error text (dhcpv4.go:129, :590-594, dhcpv6.go:92,102,
# dhcpv6_options.go:612,617); the %d are filled from err_arg and op.  10 is no return: HardwareLen >= 228
# makes dhcpv4.go:143 panic, and this is the error DecodeLayers makes of it (parser.go:328-332)
ERROR_TEXTS = {
    1: "DHCPv4 length %d too short",
    2: "Bad DHCP header",
    3: "Not enough data to decode",
    4: "Option is malformed",
    5: "DHCPv6 length %d too short",
    6: "DHCPv6 length %d too short for message type %d",
    7: "not enough data to decode",
    8: "dhcpv6 option size < length %d",
    9: "Not enough data to decode",
    10: "panic: runtime error: slice bounds out of range [28:%d]",
}


class GpdDhcpConfig(C.Structure):
    _fields_ = [("max_options", C.c_uint32), ("reserved", C.c_uint32)]


class GpdDhcpOut(C.Structure):
    _fields_ = [("msgs", C.c_void_p), ("cap_msgs", C.c_uint64), ("opts", C.c_void_p), ("cap_opts", C.c_uint64)]


class GpdDhcpCounts(C.Structure):
    _fields_ = [("msgs", C.c_uint64), ("options", C.c_uint64), ("deferred", C.c_uint64), ("work", C.c_uint64)]


DHCP_EXPORTS = {
    # include/gpd_dhcp.h — name: (restype, argtypes)
    "gpd_dhcp_decode": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.POINTER(GpdResult), C.POINTER(GpdDhcpConfig),
                                  C.POINTER(GpdDhcpOut), C.POINTER(GpdDhcpCounts), C.c_void_p]),
    "gpd_dhcp_decode_host": (C.c_int, [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_uint64, C.POINTER(GpdDhcpCounts)]),
}

_bound = False


def dhcp_lib():
    """The loaded library with the DHCP signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in DHCP_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


def error_text(verdict: int, err_arg: int = 0, op: int = 0) -> str:
    """The reference's err.Error() for a verdict with its arguments."""
    v = int(verdict)
    t = ERROR_TEXTS.get(v)
    if t is None:
        return f"gpd: unknown DHCP verdict {verdict}"
    if v == DHCP_E_V6_RELAY_SHORT:
        return t % (int(err_arg), int(op))
    return t % int(err_arg) if "%d" in t else t


class DHCPDecodeError(Exception):
    """The error DecodeFromBytes returned; str() is the reference's err.Error()."""

    def __init__(self, code: int, err_arg: int = 0, op: int = 0):
        self.code = int(code)
        super().__init__(error_text(code, err_arg, op))

    def Error(self) -> str:
        return str(self)


def _counts(cnt):
    return {k: int(getattr(cnt, k)) for k, _ in GpdDhcpCounts._fields_}


def _raise_with_counts(rc, who, counts):
    try:
        check(rc, who)
    except _lib.GpdError as e:
        e.counts = counts
        raise


def decode_host(version: int, data, max_options: int = 0, cap_opts=None):
    """One message in host memory through gpd_dhcp_decode_host (no device): (msg, opts, counts)
    with msg a MSG_DTYPE[1] array, opts OPT_DTYPE[] and counts a dict.  cap_opts None sizes the
    array with a first call; otherwise it is passed as given, and a short one raises GpdError with
    the need in its `counts` attribute."""
    buf = np.frombuffer(bytes(data), np.uint8)
    msg = np.zeros(1, MSG_DTYPE)
    cnt = GpdDhcpCounts()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    lib = dhcp_lib()
    if cap_opts is None:
        rc = lib.gpd_dhcp_decode_host(version, ptr(buf), len(buf), max_options, ptr(msg), None, 0, C.byref(cnt))
        if rc != 0 and not cnt.msgs:
            check(rc, "gpd_dhcp_decode_host")
        cap_opts = int(cnt.options)
    opts = np.zeros(cap_opts, OPT_DTYPE)
    rc = lib.gpd_dhcp_decode_host(version, ptr(buf), len(buf), max_options, ptr(msg), ptr(opts), cap_opts,
                                  C.byref(cnt))
    counts = _counts(cnt)
    if rc != 0:
        _raise_with_counts(rc, "gpd_dhcp_decode_host", counts)
    return msg, opts[:counts["options"]], counts


# ---------------------------------------------------------------- the reference's objects
class DHCPOption:
    """DHCPOption (dhcpv4.go:483-487): Type, Length, Data (None for Pad)."""

    def __init__(self, Type=0, Length=0, Data=None):
        self.Type, self.Length, self.Data = Type, Length, Data


class DHCPv6Option:
    """DHCPv6Option (dhcpv6_options.go:557-561): Code, Length, Data."""

    def __init__(self, Code=0, Length=0, Data=b""):
        self.Code, self.Length, self.Data = Code, Length, Data


class _Decoded:
    def __init__(self):
        self.Contents = None      # BaseLayer.Contents; None: not set by this call
        self.Payload = None       # both layers leave it nil
        self.Options = []
        self.err = None
        self.truncated = False
        self.packet = 0


class DHCPv4(_Decoded):
    """layers.DHCPv4 as DecodeFromBytes leaves it (dhcpv4.go:85-102), with `err` the error it
    returned (None: nil), `truncated`, and `packet`, the index of its packet.  After
    "DHCPv4 length %d too short" no field was assigned; after the panic of a HardwareLen >= 228
    (`err` is what DecodeLayers returns for it) ClientHWAddr, ServerName and File were not.
    `hw_past_data`: a HardwareLen below 228 passes the message and ClientHWAddr is clipped to it
    (include/gpd_dhcp.h)."""
    version = 4

    def __init__(self):
        super().__init__()
        self.Operation = self.HardwareType = self.HardwareLen = self.HardwareOpts = 0
        self.Xid = self.Secs = self.Flags = 0
        self.ClientIP = self.YourClientIP = self.NextServerIP = self.RelayAgentIP = None
        self.ClientHWAddr = self.ServerName = self.File = None
        self.hw_past_data = False


class DHCPv6(_Decoded):
    """layers.DHCPv6 as DecodeFromBytes leaves it (dhcpv6.go:75-83)."""
    version = 6

    def __init__(self):
        super().__init__()
        self.MsgType = self.HopCount = 0
        self.LinkAddr = self.PeerAddr = self.TransactionID = None


def materialize(m, opts, data: bytes):
    """The DHCPv4 or DHCPv6 object of one message record `m` (its opts[first_opt..] in `opts`)."""
    v = int(m["verdict"])
    if v == DHCP_DEFERRED:
        raise ValueError("materialize: a deferred message has no entries; decode it with decode_host")
    mf = int(m["mflags"])
    k, n = int(m["first_opt"]), int(m["n_opts"])
    if int(m["version"]) == 4:
        d = DHCPv4()
        if v != DHCP_E_V4_TOO_SHORT:
            d.Operation, d.HardwareType, d.HardwareLen, d.HardwareOpts = (int(m["op"]), int(m["htype"]),
                                                                          int(m["hlen"]), int(m["hops"]))
            d.Xid, d.Secs, d.Flags = int(m["xid"]), int(m["secs"]), int(m["flags"])
            d.ClientIP, d.YourClientIP, d.NextServerIP, d.RelayAgentIP = (data[12:16], data[16:20], data[20:24],
                                                                          data[24:28])
            if v != DHCP_E_V4_HW_PANIC:  # (the panic at :143 comes before these three)
                d.ClientHWAddr = data[28:28 + d.HardwareLen]  # clipped to data when hw_past_data
                d.ServerName, d.File = data[44:108], data[108:236]
            d.hw_past_data = bool(mf & F_HW_PAST_DATA)
        for o in opts[k:k + n]:
            off, code, length = int(o["off"]), int(o["code"]), int(o["length"])
            d.Options.append(DHCPOption(code, length, None if code == DHCPOptPad else data[off + 2:off + 2 + length]))
    else:
        d = DHCPv6()
        if v != DHCP_E_V6_TOO_SHORT:
            d.MsgType = int(m["op"])
            if mf & F_RELAY:
                d.HopCount, d.LinkAddr, d.PeerAddr = int(m["hops"]), data[2:18], data[18:34]
            elif v != DHCP_E_V6_RELAY_SHORT:
                d.TransactionID = data[1:4]
        for o in opts[k:k + n]:
            off, code, length = int(o["off"]), int(o["code"]), int(o["length"])
            d.Options.append(DHCPv6Option(code, length, data[off + 4:off + 4 + length]))
    d.packet = int(m["packet"])
    d.truncated = bool(m["truncated"])
    if v != DHCP_OK:
        d.err = DHCPDecodeError(v, int(m["err_arg"]), int(m["op"]))
    if mf & F_CONTENTS:
        d.Contents = data
    return d


def decode_bytes(version: int, data):
    """DecodeFromBytes of one message in host memory (the host walker, no budget)."""
    data = bytes(data)
    msg, opts, _ = decode_host(version, data, 0)
    return materialize(msg[0], opts, data)


class DHCPResult:
    """The decode's arrays on the device: `msgs` (count x 48 B) and `opts` (n_options x 8 B),
    uint8 tensors; `count`, `n_options` and `deferred`."""

    def __init__(self, dbatch, msgs, opts, counts, max_options):
        self._source = ("batch", dbatch)
        self.msgs, self.opts = msgs, opts
        self.count, self.n_options, self.deferred = counts["msgs"], counts["options"], counts["deferred"]
        self.max_options = max_options

    def to_host(self):
        """(MSG_DTYPE[count], OPT_DTYPE[n_options]) copies."""
        m = self.msgs[:self.count * MSG_DTYPE.itemsize].cpu().numpy().view(MSG_DTYPE).copy()
        o = self.opts[:self.n_options * OPT_DTYPE.itemsize].cpu().numpy().view(OPT_DTYPE).copy()
        return m, o

    # `data` of every message, gathered on the device and copied once: a list of bytes (the
    # gather of the TLS result's batch source, which reads _source and to_host()[0] only)
    message_bytes = TLSResult.message_bytes

    def messages(self):
        """One DHCPv4 or DHCPv6 object per message, in order, as the reference leaves it.  Deferred
        messages are decoded by the host walker."""
        msgs, opts = self.to_host()
        datas = self.message_bytes(msgs)
        out = []
        for m, data in zip(msgs, datas):
            if int(m["verdict"]) == DHCP_DEFERRED:
                d = decode_bytes(int(m["version"]), data)
                d.packet = int(m["packet"])
            else:
                d = materialize(m, opts, data)
            out.append(d)
        return out


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def DecodeDHCP(parser, dbatch, dres, max_options: int = MAX_OPTIONS_DEFAULT, stream=None, caps=None) -> DHCPResult:
    """layers.DHCPv4 / layers.DHCPv6 for every packet of the batch `parser` decoded into `dres`
    (hdr_off required) whose decode stopped at LayerTypeDHCPv4 or LayerTypeDHCPv6.  The sizing call
    and the exact allocation happen here; caps (cap_msgs, cap_opts) skips the sizing call and
    raises GpdError, with the needs in its `counts` attribute, when one is short.  Synchronises
    `stream`."""
    from .parser import _torch
    torch = _torch()
    if dres.hdr_off is None:
        raise ValueError("DecodeDHCP needs a DeviceResult with hdr_off")
    dev = torch.device("cuda", parser.device)
    s = stream if stream is not None else torch.cuda.current_stream(parser.device)
    b, r = dbatch.c_batch(), dres.c_result()
    cfg = GpdDhcpConfig(int(max_options) if 0 <= int(max_options) < 1 << 32 else 0, 0)
    who = "gpd_dhcp_decode"

    def call(msgs, opts, caps):
        out = GpdDhcpOut(_ptr(msgs), caps[0], _ptr(opts), caps[1])
        cnt = GpdDhcpCounts()
        rc = dhcp_lib().gpd_dhcp_decode(parser.ctx().h, C.byref(b), C.byref(r), C.byref(cfg), C.byref(out),
                                        C.byref(cnt), C.c_void_p(s.cuda_stream))
        return rc, _counts(cnt)

    if caps is None:
        rc, counts = call(None, None, (0, 0))
        if rc != 0 and not (counts["msgs"] or counts["options"]):
            check(rc, who)
        caps = (counts["msgs"], counts["options"])
        if rc == 0:  # no message at all
            z = torch.empty(0, dtype=torch.uint8, device=dev)
            return DHCPResult(dbatch, z, z, counts, max_options)
    caps = tuple(int(c) for c in caps)
    msgs = torch.empty(max(caps[0], 1) * MSG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    opts = torch.empty(max(caps[1], 1) * OPT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rc, counts = call(msgs, opts, caps)
    if rc != 0:
        _raise_with_counts(rc, who, counts)
    return DHCPResult(dbatch, msgs[:counts["msgs"] * MSG_DTYPE.itemsize],
                      opts[:counts["options"] * OPT_DTYPE.itemsize], counts, max_options)
