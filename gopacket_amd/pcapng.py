"""pcapng ingest: a pcapng capture in memory -> a PacketBatch over its own bytes.

The reference reads a pcapng capture block by block with pcapgo.NgReader (pcapgo/ngread.go),
copying each packet out.  Here the capture is read through the native reader of
include/gpd_pcapng.h, a restatement of NgReader (not of the pcapng standard) whose offsets point
into the capture buffer itself: the capture IS the batch buffer.  Errors keep pcapgo's texts; the
packets before the block the reference stops at are returned with the error, as a ReadPacketData
loop would have seen them.

The entry points are bound onto the loaded library here, on first use, from NG_EXPORTS: they
live in their own header and are not part of _lib.EXPORTS.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import GpdResult, check
from .batch import PAD, PacketBatch
from .pcap import capture_array

GPD_ERR_PCAPNG = -6
BLOCK_SECTION, BLOCK_INTERFACE, BLOCK_PACKET, BLOCK_SIMPLE, BLOCK_STATS, BLOCK_ENHANCED = \
    0x0A0D0D0A, 1, 2, 3, 5, 6
BYTE_ORDER_MAGIC = 0x1A2B3C4D
LINKTYPE_NULL, LINKTYPE_ETHERNET = 0, 1
(STOP_LIMIT, STOP_EOF, STOP_EOF_BLOCK, STOP_NEGATIVE, STOP_IFACE_ID, STOP_NO_IFACE, STOP_NO_FIRST,
 STOP_BYTE_ORDER, STOP_OPT_END, STOP_VERSION, STOP_LINKTYPE, STOP_PANIC, STOP_MAGIC) = range(13)


class PcapNgError(Exception):
    def __init__(self, text: str, stop: int = 0):
        super().__init__(text)
        self.stop = stop


class GpdPcapngOpts(C.Structure):
    _fields_ = [("want_mixed_linktype", C.c_uint32), ("error_on_mismatching_linktype", C.c_uint32),
                ("skip_unknown_version", C.c_uint32), ("device_walk", C.c_int32),
                ("chunk_bytes", C.c_uint64)]


class GpdPcapngStr(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint32), ("reserved", C.c_uint32)]


class GpdPcapngSectionInfo(C.Structure):
    _fields_ = [("hardware", GpdPcapngStr), ("os", GpdPcapngStr), ("application", GpdPcapngStr),
                ("comment", GpdPcapngStr), ("big_endian", C.c_uint32), ("reserved", C.c_uint32)]


class GpdPcapngIface(C.Structure):
    _fields_ = [("name", GpdPcapngStr), ("comment", GpdPcapngStr), ("description", GpdPcapngStr),
                ("filter", GpdPcapngStr), ("os", GpdPcapngStr), ("ts_offset", C.c_uint64),
                ("second_mask", C.c_uint64), ("scale_up", C.c_uint64), ("scale_down", C.c_uint64),
                ("linktype", C.c_uint32), ("snaplen", C.c_uint32), ("ts_resolution", C.c_uint32),
                ("reserved", C.c_uint32)]


NG_EXPORTS = {
    # include/gpd_pcapng.h — name: (restype, argtypes)
    "gpd_pcapng_open": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(GpdPcapngOpts),
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "gpd_pcapng_index": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 +
                         [C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "gpd_pcapng_linktype": (C.c_uint32, [C.c_void_p]),
    "gpd_pcapng_ninterfaces": (C.c_uint32, [C.c_void_p]),
    "gpd_pcapng_interface": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(GpdPcapngIface)]),
    "gpd_pcapng_section": (C.c_int, [C.c_void_p, C.POINTER(GpdPcapngSectionInfo)]),
    "gpd_pcapng_resolution": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpd_pcapng_skip_section": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "gpd_pcapng_pos": (C.c_uint64, [C.c_void_p]),
    "gpd_pcapng_close": (None, [C.c_void_p]),
    "gpd_pcapng_last_error": (C.c_char_p, []),
    "gpd_decode_pcapng": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(GpdResult),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_int]),
    "gpd_decode_pcapng_last_walk_counts": (None, [C.c_void_p]),
}

_bound = False


def ng_lib():
    """The loaded library with the pcapng entry points' signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in NG_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


@dataclass
class NgReaderOptions:
    """pcapgo.NgReaderOptions (ngread.go:22-36) + this library's knobs (gpd_pcapng_opts)."""
    WantMixedLinkType: bool = False
    ErrorOnMismatchingLinkType: bool = False
    SkipUnknownVersion: bool = False
    device_walk: int = -1      # DecodePcapNg: -1 automatic (on), 0 host walk only
    chunk_bytes: int = 0       # DecodePcapNg: bytes per H2D chunk (0 = 64 MiB)

    def c(self) -> GpdPcapngOpts:
        return GpdPcapngOpts(int(self.WantMixedLinkType), int(self.ErrorOnMismatchingLinkType),
                             int(self.SkipUnknownVersion), int(self.device_walk), int(self.chunk_bytes))


DefaultNgReaderOptions = NgReaderOptions()


@dataclass
class NgSectionInfo:
    """pcapgo.NgSectionInfo (pcapng.go:178-187); strings as bytes."""
    Hardware: bytes = b""
    OS: bytes = b""
    Application: bytes = b""
    Comment: bytes = b""
    big_endian: bool = False


@dataclass
class NgInterface:
    """pcapgo.NgInterface (pcapng.go:145-170) without Statistics; strings as bytes."""
    Name: bytes = b""
    Comment: bytes = b""
    Description: bytes = b""
    Filter: bytes = b""
    OS: bytes = b""
    LinkType: int = 0
    TimestampResolution: int = 0
    TimestampOffset: int = 0
    SnapLength: int = 0


@dataclass
class PcapNg:
    batch: PacketBatch        # data = the capture bytes (+ PAD), offsets into it
    ts_sec: np.ndarray        # int64[n]  CaptureInfo.Timestamp, Unix seconds ...
    ts_nsec: np.ndarray       # uint32[n] ... and nanoseconds (0, 0 for simple packet blocks)
    length: np.ndarray        # uint32[n] CaptureInfo.Length
    ifindex: np.ndarray       # uint32[n] CaptureInfo.InterfaceIndex
    linktype: np.ndarray      # uint32[n] the interface's link type (AncillaryData[0] when mixed)
    stop: int                 # STOP_*: how the ReadPacketData loop ended
    err: Optional[str]        # the reference's error text; None for the limit or a clean EOF
    next_pos: int = 0         # gpd_pcapng_pos after the call


class NgReader:
    """pcapgo.NgReader over an in-memory capture (an array from pcap.capture_array, or bytes)."""

    def __init__(self, buf, options: Optional[NgReaderOptions] = None, data_len: Optional[int] = None):
        self.cap = buf if isinstance(buf, np.ndarray) else capture_array(buf)
        self.data_len = self.cap.shape[0] - PAD if data_len is None else int(data_len)
        self.options = options or NgReaderOptions()
        self._lib = ng_lib()
        self._h = C.c_void_p()
        o, stop = self.options.c(), C.c_int()
        rc = self._lib.gpd_pcapng_open(self.cap.ctypes.data, self.data_len, C.byref(o), C.byref(self._h),
                                       C.byref(stop))
        if rc == GPD_ERR_PCAPNG:
            raise PcapNgError(self._lib.gpd_pcapng_last_error().decode(), stop.value)
        check(rc, "gpd_pcapng_open")

    @property
    def h(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.gpd_pcapng_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _str(self, s: GpdPcapngStr) -> bytes:
        if s.len and s.off == 0xFFFFFFFFFFFFFFFF:
            return bytes(s.len)
        return self.cap[s.off:s.off + s.len].tobytes()

    def LinkType(self) -> int:
        return self._lib.gpd_pcapng_linktype(self._h)

    def NInterfaces(self) -> int:
        return self._lib.gpd_pcapng_ninterfaces(self._h)

    def Interface(self, i: int) -> NgInterface:
        f = GpdPcapngIface()
        if self._lib.gpd_pcapng_interface(self._h, int(i), C.byref(f)) != 0:
            raise PcapNgError(self._lib.gpd_pcapng_last_error().decode())
        return NgInterface(self._str(f.name), self._str(f.comment), self._str(f.description),
                           self._str(f.filter), self._str(f.os), f.linktype, f.ts_resolution,
                           f.ts_offset, f.snaplen)

    def SectionInfo(self) -> NgSectionInfo:
        s = GpdPcapngSectionInfo()
        check(self._lib.gpd_pcapng_section(self._h, C.byref(s)), "gpd_pcapng_section")
        return NgSectionInfo(self._str(s.hardware), self._str(s.os), self._str(s.application),
                             self._str(s.comment), bool(s.big_endian))

    def Resolution(self):
        """(base, exponent) of interface 0's timestamps; (0, 0) with WantMixedLinkType."""
        b, e = C.c_int(), C.c_int()
        if self._lib.gpd_pcapng_resolution(self._h, C.byref(b), C.byref(e)) != 0:
            raise PcapNgError(self._lib.gpd_pcapng_last_error().decode())
        return b.value, e.value

    def SkipSection(self) -> None:
        stop = C.c_int()
        rc = self._lib.gpd_pcapng_skip_section(self._h, C.byref(stop))
        if rc == GPD_ERR_PCAPNG:
            raise PcapNgError(self._lib.gpd_pcapng_last_error().decode(), stop.value)
        check(rc, "gpd_pcapng_skip_section")

    def pos(self) -> int:
        return self._lib.gpd_pcapng_pos(self._h)

    def index(self, max_n: Optional[int] = None) -> PcapNg:
        """The next max_n ReadPacketData results (all that follow when None)."""
        if max_n is None:  # every packet block takes at least 12 bytes
            max_n = max(0, self.data_len - self.pos()) // 12 + 1
        m = int(max_n)
        off, ln, wl = (np.empty(m, np.uint32) for _ in range(3))
        sec, nsec = np.empty(m, np.int64), np.empty(m, np.uint32)
        ifx, lt = np.empty(m, np.uint32), np.empty(m, np.uint32)
        n, stop = C.c_uint64(), C.c_int()
        rc = self._lib.gpd_pcapng_index(self._h, m, off.ctypes.data, ln.ctypes.data, wl.ctypes.data,
                                        sec.ctypes.data, nsec.ctypes.data, ifx.ctypes.data, lt.ctypes.data,
                                        C.byref(n), C.byref(stop))
        err = None
        if rc == GPD_ERR_PCAPNG:
            err = self._lib.gpd_pcapng_last_error().decode()
        elif rc != 0:
            check(rc, "gpd_pcapng_index")
        k = n.value
        return PcapNg(PacketBatch(self.cap, self.data_len, off[:k], ln[:k]), sec[:k], nsec[:k], wl[:k],
                      ifx[:k], lt[:k], stop.value, err, self.pos())

    ReadAll = index


def NewNgReader(buf, options: Optional[NgReaderOptions] = None) -> NgReader:
    """pcapgo.NewNgReader (ngread.go:61-83)."""
    return NgReader(buf, options)


def parse_pcapng(buf, options: Optional[NgReaderOptions] = None) -> PcapNg:
    return NgReader(buf, options).ReadAll()


def read_pcapng(path: str, options: Optional[NgReaderOptions] = None) -> PcapNg:
    with open(path, "rb") as f:
        return parse_pcapng(f.read(), options)


def read_capture(path: str):
    """A capture file by its magic: pcap.Pcap for classic pcap, PcapNg for pcapng."""
    from . import pcap
    with open(path, "rb") as f:
        cap = capture_array(f.read())
    if cap.shape[0] - PAD >= 4 and cap[:4].tobytes() == b"\x0a\x0d\x0d\x0a":
        return NgReader(cap).ReadAll()
    return pcap.index(cap)


def last_walk_counts() -> List[int]:
    """gpd_decode_pcapng_last_walk_counts: [chunks walked on the device, whole chunks handed to
    the host, tails handed over at a state-changing block, refuted, not vouched for, uncovered,
    short, segments re-walked]."""
    c = (C.c_uint32 * 8)()
    ng_lib().gpd_decode_pcapng_last_walk_counts(c)
    return list(c)


# --- writing (the layout of pcapgo.NgWriter, pcapgo/ngwrite.go) -------------------------------

def _opt(code: int, val: bytes, e: str) -> bytes:
    return struct.pack(e + "HH", code, len(val)) + val + bytes(-len(val) % 4)


def _block(typ: int, body: bytes, e: str) -> bytes:
    total = 12 + len(body)
    return struct.pack(e + "II", typ, total) + body + struct.pack(e + "I", total)


def section_block(big_endian: bool = False, hardware: bytes = b"", os_: bytes = b"", application: bytes = b"",
                  comment: bytes = b"", version=(1, 0)) -> bytes:
    """A section header block (writeSectionHeader, ngwrite.go:187-235: options in the order
    application, comment, hardware, os)."""
    e = ">" if big_endian else "<"
    opts = b"".join(_opt(c, v, e) for c, v in ((4, application), (1, comment), (2, hardware), (3, os_)) if v)
    if opts:
        opts += struct.pack(e + "HH", 0, 0)
    body = struct.pack(e + "IHHq", BYTE_ORDER_MAGIC, version[0], version[1], -1) + opts
    return _block(BLOCK_SECTION, body, e)


def interface_block(linktype: int = LINKTYPE_ETHERNET, snaplen: int = 0, name: bytes = b"",
                    tsresol: Optional[int] = None, tsoffset: Optional[int] = None,
                    big_endian: bool = False) -> bytes:
    """An interface description block (AddInterface, ngwrite.go:237-299)."""
    e = ">" if big_endian else "<"
    opts = _opt(2, name, e) if name else b""
    if tsresol is not None:
        opts += _opt(9, bytes([tsresol]), e)
    if tsoffset is not None:
        opts += _opt(14, struct.pack(e + "Q", tsoffset), e)
    if opts:
        opts += struct.pack(e + "HH", 0, 0)
    return _block(BLOCK_INTERFACE, struct.pack(e + "HHI", linktype, 0, snaplen) + opts, e)


def enhanced_block(data: bytes, ifindex: int = 0, ts: int = 0, wirelen: Optional[int] = None,
                   big_endian: bool = False) -> bytes:
    """An enhanced packet block (WritePacket, ngwrite.go:356-393): ts in the interface's units."""
    e = ">" if big_endian else "<"
    wl = len(data) if wirelen is None else wirelen
    body = struct.pack(e + "IIIII", ifindex, ts >> 32, ts & 0xFFFFFFFF, len(data), wl) + data + bytes(-len(data) % 4)
    return _block(BLOCK_ENHANCED, body, e)


def write_pcapng(batch: PacketBatch, linktype: int = LINKTYPE_ETHERNET, snaplen: int = 0,
                 ts_sec=None, ts_nsec=None, length=None, big_endian: bool = False,
                 application: bytes = b"gopacket_amd", name: bytes = b"intf0") -> bytes:
    """One section, one interface with nanosecond resolution (if_tsresol 9, as NgWriter writes,
    ngwrite.go:273-274), every packet an enhanced packet block."""
    out = [section_block(big_endian, application=application),
           interface_block(linktype, snaplen, name, tsresol=9, big_endian=big_endian)]
    for i in range(batch.n):
        s = int(ts_sec[i]) if ts_sec is not None else i // 1000000
        ns = int(ts_nsec[i]) if ts_nsec is not None else (i % 1000000) * 1000
        wl = int(length[i]) if length is not None else None
        out.append(enhanced_block(batch.packet(i), 0, s * 1000000000 + ns, wl, big_endian))
    return b"".join(out)


def synth_capture_ng(batch: PacketBatch, snaplen: int = 0) -> np.ndarray:
    """The pcapng stream of a batch built with numpy (large synthetic captures): a section
    header, one Ethernet interface (microseconds), then packet i as a little-endian enhanced
    packet block {6, total, 0, ts_high, ts_low = i, caplen, caplen, bytes, padding, total}."""
    n = batch.n
    pre = section_block() + interface_block(LINKTYPE_ETHERNET, snaplen)
    ln = batch.caplen.astype(np.int64)
    padded = (ln + 3) & ~3
    rec = 32 + padded
    start = np.zeros(n, np.int64)
    if n > 1:
        np.cumsum(rec[:-1], out=start[1:])
    start += len(pre)
    total = len(pre) + int(rec.sum())
    cap = np.zeros(total + PAD, np.uint8)
    cap[:len(pre)] = np.frombuffer(pre, np.uint8)
    hdr = np.zeros((n, 7), np.uint32)
    idx = np.arange(n, dtype=np.uint64)
    hdr[:, 0] = BLOCK_ENHANCED
    hdr[:, 1] = rec
    hdr[:, 3] = (idx >> np.uint64(32)).astype(np.uint32)
    hdr[:, 4] = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hdr[:, 5] = batch.caplen
    hdr[:, 6] = batch.caplen
    pos = start[:, None] + np.arange(28)[None, :]
    cap[pos.ravel()] = hdr.view(np.uint8).reshape(n, 28).ravel()
    tail = (start + 28 + padded)[:, None] + np.arange(4)[None, :]
    cap[tail.ravel()] = np.ascontiguousarray(hdr[:, 1:2]).view(np.uint8).reshape(n, 4).ravel()
    src_off = batch.offset.astype(np.int64)
    for L in np.unique(ln):
        sel_all = np.nonzero(ln == L)[0]
        step = max(1, (1 << 24) // max(int(L), 1))  # bound the index arrays to ~16M entries
        for c in range(0, sel_all.size if L else 0, step):
            sel = sel_all[c:c + step]
            s = src_off[sel][:, None] + np.arange(L)[None, :]
            d = (start[sel] + 28)[:, None] + np.arange(L)[None, :]
            cap[d.ravel()] = batch.data[s.ravel()]
    return cap
