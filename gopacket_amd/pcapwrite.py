"""pcap writing (the writers): kept packets of a device batch -> a pcapgo stream.

The reference writes a capture one packet at a time: pcapgo.Writer.WritePacket puts a 16-byte
record header and the packet's bytes on an io.Writer (pcapgo/write.go:101-129).  Here the packets
are a DeviceBatch in HBM and a mask says which to keep: gpd_pcap_write (include/gpd_pcapwrite.h)
builds the stream on the device, a stream compaction over variable-length records, and
gpd_batch_select repacks the same packets into a new dense batch for more work on the device.
The pcapng form of the same way out is pcapgo.NgWriter (pcapgo/ngwrite.go): NgWriter below,
over gpd_pcapng_write and the host-built blocks of include/gpd_pcapngwrite.h.

The entry points are bound onto the loaded library here, on first use, from PW_EXPORTS: they
live in their own header and are not part of _lib.EXPORTS.
"""
from __future__ import annotations

import ctypes as C
import struct
import time
from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np

from . import _lib
from ._lib import GPD_ERR_INVALID, GPD_ERR_PCAP, GpdBatch, check
from .pcap import PcapError
from .pcapng import GpdPcapngIface, GpdPcapngSectionInfo, GpdPcapngStr, NgInterface, NgSectionInfo

GPD_PCAPW_NANOS, GPD_PCAPW_FILE_HEADER = 1, 2
NO_BAD_INDEX = 0xFFFFFFFFFFFFFFFF

PW_EXPORTS = {
    # include/gpd_pcapwrite.h — name: (restype, argtypes)
    "gpd_pcap_file_header": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gpd_pcap_write": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                 C.c_void_p]),
    "gpd_batch_select": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]),
}

_bound = False


def pw_lib():
    """The loaded library with the writer entry points' signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in PW_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


@dataclass
class CaptureInfo:
    """gopacket.CaptureInfo as the writer reads it; Timestamp in Unix nanoseconds (None: Go's
    zero time, for which WritePacket takes time.Now(), write.go:103-105)."""
    Timestamp: Optional[int] = None
    CaptureLength: int = 0
    Length: int = 0
    InterfaceIndex: int = 0   # the NgWriter's (ngwrite.go:357-359); pcapgo.Writer does not look at it


def file_header(snaplen: int, linktype: int, nanos: bool = False) -> bytes:
    """WriteFileHeader's 24 bytes (write.go:80-96), from gpd_pcap_file_header."""
    buf = (C.c_uint8 * 24)()
    check(pw_lib().gpd_pcap_file_header(GPD_PCAPW_NANOS if nanos else 0, int(snaplen) & 0xFFFFFFFF,
                                        int(linktype) & 0xFFFFFFFF, buf), "gpd_pcap_file_header")
    return bytes(buf)


def _dev(x, dtype, device, n, what):
    """A device tensor of n elements of `dtype` (numpy) from a torch tensor or a numpy array;
    None stays None.  The bytes are taken as they are: a tensor of the signed twin type is fine."""
    if x is None:
        return None
    import torch
    if isinstance(x, torch.Tensor):
        if x.element_size() != np.dtype(dtype).itemsize:
            raise TypeError(f"{what}: {x.dtype} has not the element size of {np.dtype(dtype).name}")
        t = x.to(torch.device("cuda", device)).contiguous()
    else:
        a = np.ascontiguousarray(np.asarray(x).astype(dtype, copy=False))
        signed = {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
        t = torch.from_numpy(a.view(signed)).to(torch.device("cuda", device))
    if t.numel() != n:
        raise ValueError(f"{what}: {t.numel()} entries for {n} packets")
    return t


def _keep_dev(keep, device, n):
    if keep is None:
        return None
    import torch
    if isinstance(keep, torch.Tensor) and keep.dtype == torch.bool:
        keep = keep.to(torch.uint8)
    elif not isinstance(keep, torch.Tensor) and np.asarray(keep).dtype == np.bool_:
        keep = np.asarray(keep).astype(np.uint8)
    return _dev(keep, np.uint8, device, n, "keep")


def _ctx_handle(parser_or_ctx):
    c = parser_or_ctx.ctx() if hasattr(parser_or_ctx, "ctx") else parser_or_ctx
    return c.h


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _write_call(h, dbatch, ts, wl, kp, flags, snaplen, linktype, out, stream):
    """One gpd_pcap_write: (rc, records, bytes, bad index); out None is the sizing call."""
    nw, nb, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    b = dbatch.c_batch()
    rc = pw_lib().gpd_pcap_write(h, C.byref(b), _ptr(ts), _ptr(wl), _ptr(kp), flags, snaplen, linktype,
                                 _ptr(out), out.numel() if out is not None else 0,
                                 C.byref(nw), C.byref(nb), C.byref(bad), C.c_void_p(stream.cuda_stream))
    return rc, nw.value, nb.value, bad.value


def write_device(parser_or_ctx, dbatch, ts_ns, length=None, keep=None, nanos: bool = False,
                 file_header=None, stream=None, out=None):
    """The kept packets of `dbatch` as a pcap stream in HBM (gpd_pcap_write): returns (uint8
    device tensor trimmed to the stream, records written).  ts_ns (uint64 Unix ns), length
    (CaptureInfo.Length; None: the capture length) and keep (nonzero or True = write; None: every
    packet) are torch device tensors or numpy arrays.  file_header: None, or (snaplen, linktype)
    for a stream that starts with WriteFileHeader's bytes.  `out` (a uint8 device tensor) is
    written in place when it is large enough.  Raises PcapError at the first kept packet with
    capture length > length; its .stream and .n_written hold what the loop wrote before it, and
    .bad_index the packet."""
    from .parser import _torch
    torch = _torch()
    dev, n = dbatch.device, dbatch.n
    h = _ctx_handle(parser_or_ctx)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    ts = _dev(ts_ns, np.uint64, dev, n, "ts_ns")
    wl = _dev(length, np.uint32, dev, n, "length")
    kp = _keep_dev(keep, dev, n)
    flags = (GPD_PCAPW_NANOS if nanos else 0) | (GPD_PCAPW_FILE_HEADER if file_header is not None else 0)
    snaplen, linktype = (int(file_header[0]), int(file_header[1])) if file_header is not None else (0, 0)
    # without an `out` that fits, a sizing call first (the scan alone), then the write
    rc, nw, nb, bad = _write_call(h, dbatch, ts, wl, kp, flags, snaplen, linktype, out, s)
    if rc not in (0, GPD_ERR_PCAP) and not (rc == GPD_ERR_INVALID and out is not None and nb > out.numel()):
        check(rc, "gpd_pcap_write")
    if out is None or nb > out.numel():
        # (a multiple of 16 and never empty: the allocation is 16-byte aligned either way)
        out = torch.empty(max(16, (nb + 15) & ~15), dtype=torch.uint8, device=torch.device("cuda", dev))
        rc, nw, nb, bad = _write_call(h, dbatch, ts, wl, kp, flags, snaplen, linktype, out, s)
    if rc == GPD_ERR_PCAP:
        e = PcapError(_lib.lib.gpd_last_error_string().decode())
        e.stream, e.n_written, e.bad_index = out[:nb], nw, bad
        raise e
    check(rc, "gpd_pcap_write")
    return out[:nb], nw


class Writer:
    """pcapgo.Writer (write.go:22-129) over any object with .write."""

    def __init__(self, w, nanos: bool = False):
        self.w = w
        self.nanos = bool(nanos)
        self.tsScaler = 1 if nanos else 1000  # write.go:98-99

    def WriteFileHeader(self, snaplen: int, linktype: int) -> None:
        """write.go:80-96."""
        self.w.write(file_header(snaplen, linktype, self.nanos))

    def WritePacket(self, ci, data: bytes) -> None:
        """write.go:117-129 for one host packet."""
        if ci.CaptureLength != len(data):
            raise PcapError(f"capture length {ci.CaptureLength} does not match data length {len(data)}")
        if ci.CaptureLength > ci.Length:
            raise PcapError(f"invalid capture info {ci!r}:  capture length > length")
        t = time.time_ns() if ci.Timestamp is None else int(ci.Timestamp)  # :103-105
        secs, nsec = divmod(t, 1000000000)
        self.w.write(struct.pack("<IIII", secs & 0xFFFFFFFF, (nsec // self.tsScaler) & 0xFFFFFFFF,
                                 ci.CaptureLength & 0xFFFFFFFF, ci.Length & 0xFFFFFFFF))
        self.w.write(bytes(data))

    def WritePackets(self, dbatch, ts_ns, length=None, keep=None, parser=None) -> int:
        """The WritePacket loop over the kept packets of a DeviceBatch, on the device
        (gpd_pcap_write); the stream is copied back and written to w.  Returns the records
        written.  At a rejected packet the records before it are written, then PcapError raised,
        as the loop would have.  `parser`: the DecodingLayerParser (or context) whose device
        context serves the call; one is made for the batch's device when None."""
        if parser is None:
            parser = self._parser(dbatch.device)
        try:
            stream, nw = write_device(parser, dbatch, ts_ns, length, keep, nanos=self.nanos)
        except PcapError as e:
            if getattr(e, "stream", None) is not None:
                self.w.write(e.stream.cpu().numpy().tobytes())
            raise
        self.w.write(stream.cpu().numpy().tobytes())
        return nw

    def _parser(self, device):
        p = getattr(self, "_own_parser", None)
        if p is None or p.device != device:
            from .layers import LayerTypeEthernet
            from .parser import DecodingLayerParser
            p = self._own_parser = DecodingLayerParser(LayerTypeEthernet, "Ethernet", device=device)
        return p


def NewWriter(w) -> Writer:
    """pcapgo.NewWriter (write.go:74-76): microsecond timestamps."""
    return Writer(w, nanos=False)


def NewWriterNanos(w) -> Writer:
    """pcapgo.NewWriterNanos (write.go:53-55): nanosecond timestamps."""
    return Writer(w, nanos=True)


def select(parser_or_ctx, dbatch, keep, stream=None):
    """The kept packets of `dbatch` as a new dense DeviceBatch (gpd_batch_select): packet j is
    the j-th kept packet in a 16-byte aligned slot.  Returns (DeviceBatch, int32 device tensor of
    the kept packets' indices in `dbatch`)."""
    from .parser import DeviceBatch, _torch
    torch = _torch()
    dev, n = dbatch.device, dbatch.n
    tdev = torch.device("cuda", dev)
    h = _ctx_handle(parser_or_ctx)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    kp = _keep_dev(keep, dev, n)
    b = dbatch.c_batch()
    k, nb = C.c_uint64(), C.c_uint64()
    lib = pw_lib()
    check(lib.gpd_batch_select(h, C.byref(b), _ptr(kp), None, 0, None, None, None, 0, C.byref(k), C.byref(nb),
                               C.c_void_p(s.cuda_stream)), "gpd_batch_select")
    m, total = k.value, nb.value
    from .batch import PAD
    data = torch.zeros(total + PAD, dtype=torch.uint8, device=tdev)
    pad = (-m) % 16
    desc = torch.zeros(2 * m + pad, dtype=torch.int32, device=tdev)
    index = torch.zeros(m, dtype=torch.int32, device=tdev)
    offset, caplen = desc[:m], desc[m + pad:]
    if m:
        check(lib.gpd_batch_select(h, C.byref(b), _ptr(kp), _ptr(data), total, _ptr(offset), _ptr(caplen),
                                   _ptr(index), m, C.byref(k), C.byref(nb), C.c_void_p(s.cuda_stream)),
              "gpd_batch_select")
    return DeviceBatch.from_tensors(data, total, offset, caplen, dev), index


# --- pcapng (pcapgo.NgWriter, pcapgo/ngwrite.go; include/gpd_pcapngwrite.h) ---------------------

NgNoValue64 = 2 ** 64 - 1  # pcapng.go:120-121
GPD_PCAPNGW_MAX_PREFIX = 65536
BAD_NONE, BAD_IFACE, BAD_LENGTH = 0, 1, 2


class GpdPcapngStats(C.Structure):
    _fields_ = [("last_update", C.c_uint64), ("start_time", C.c_uint64), ("end_time", C.c_uint64),
                ("packets_received", C.c_uint64), ("packets_dropped", C.c_uint64),
                ("has_last_update", C.c_uint32), ("has_start_time", C.c_uint32),
                ("has_end_time", C.c_uint32), ("reserved", C.c_uint32)]


_BLOCK_TAIL = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]  # out, out_cap, *len
NGW_EXPORTS = {
    # include/gpd_pcapngwrite.h — name: (restype, argtypes)
    "gpd_pcapng_section_block": (C.c_int, [C.POINTER(GpdPcapngSectionInfo), C.c_char_p, C.c_uint64] + _BLOCK_TAIL),
    "gpd_pcapng_interface_block": (C.c_int, [C.POINTER(GpdPcapngIface), C.c_char_p, C.c_uint64] + _BLOCK_TAIL),
    "gpd_pcapng_stats_block": (C.c_int, [C.c_int64, C.c_uint32, C.POINTER(GpdPcapngStats)] + _BLOCK_TAIL),
    "gpd_pcapng_write": (C.c_int, [C.c_void_p, C.POINTER(GpdBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_uint32, C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint32), C.c_void_p]),
}

_ng_bound = False


def ngw_lib():
    """The loaded library with the pcapng writer's signatures bound (once)."""
    global _ng_bound
    if not _ng_bound:
        for name, (res, args) in NGW_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _ng_bound = True
    return _lib.lib


@dataclass
class NgWriterOptions:
    """pcapgo.NgWriterOptions (ngwrite.go:22-25)."""
    SectionInfo: NgSectionInfo = field(default_factory=NgSectionInfo)


@dataclass
class NgInterfaceStatistics:
    """pcapgo.NgInterfaceStatistics (pcapng.go:123-136); a time is Unix ns, None Go's zero time."""
    LastUpdate: Optional[int] = None
    StartTime: Optional[int] = None
    EndTime: Optional[int] = None
    PacketsReceived: int = NgNoValue64
    PacketsDropped: int = NgNoValue64


# ngwrite.go:28-42, with what runtime.GOARCH / runtime.GOOS give on this platform
DefaultNgWriterOptions = NgWriterOptions(NgSectionInfo(Hardware=b"amd64", OS=b"linux", Application=b"gopacket"))
DefaultNgInterface = NgInterface(Name=b"intf0", OS=b"linux", SnapLength=0, TimestampResolution=9)


def _strs(values):
    """The strings back to back and their gpd_pcapng_str descriptors."""
    descs, pos = [], 0
    for v in values:
        descs.append(GpdPcapngStr(pos, len(v), 0))
        pos += len(v)
    return b"".join(bytes(v) for v in values), descs


def _built(fn, what, *args) -> bytes:
    """A builder's block: the sizing call, then the block into a buffer of that size."""
    n = C.c_uint64()
    rc = fn(*args, None, 0, C.byref(n))
    if rc == GPD_ERR_PCAP:
        raise PcapError(_lib.lib.gpd_last_error_string().decode())
    check(rc, what)
    buf = (C.c_uint8 * max(1, n.value))()
    check(fn(*args, buf, n.value, C.byref(n)), what)
    return bytes(buf[:n.value])


def ng_section_block(info: NgSectionInfo) -> bytes:
    """writeSectionHeader's block (ngwrite.go:187-234), from gpd_pcapng_section_block."""
    strs, d = _strs([info.Hardware, info.OS, info.Application, info.Comment])
    c = GpdPcapngSectionInfo(d[0], d[1], d[2], d[3], int(info.big_endian), 0)
    return _built(ngw_lib().gpd_pcapng_section_block, "gpd_pcapng_section_block", C.byref(c), strs, len(strs))


def ng_interface_block(intf: NgInterface) -> bytes:
    """AddInterface's block (ngwrite.go:237-298), from gpd_pcapng_interface_block."""
    strs, d = _strs([intf.Name, intf.Comment, intf.Description, intf.Filter, intf.OS])
    c = GpdPcapngIface(d[0], d[1], d[2], d[3], d[4], int(intf.TimestampOffset) & NgNoValue64, 0, 0, 0,
                       int(intf.LinkType) & 0xFFFFFFFF, int(intf.SnapLength) & 0xFFFFFFFF,
                       int(intf.TimestampResolution) & 0xFFFFFFFF, 0)
    return _built(ngw_lib().gpd_pcapng_interface_block, "gpd_pcapng_interface_block", C.byref(c), strs, len(strs))


def ng_stats_block(intf: int, n_ifaces: int, stats: NgInterfaceStatistics) -> bytes:
    """WriteInterfaceStats's block (ngwrite.go:301-353), from gpd_pcapng_stats_block; PcapError
    with the reference's text for an interface that was not added."""
    t = lambda v: (0 if v is None else int(v) & NgNoValue64)
    c = GpdPcapngStats(t(stats.LastUpdate), t(stats.StartTime), t(stats.EndTime),
                       int(stats.PacketsReceived) & NgNoValue64, int(stats.PacketsDropped) & NgNoValue64,
                       stats.LastUpdate is not None, stats.StartTime is not None, stats.EndTime is not None, 0)
    return _built(ngw_lib().gpd_pcapng_stats_block, "gpd_pcapng_stats_block", int(intf), int(n_ifaces), C.byref(c))


def _ng_write_call(h, dbatch, ts, wl, ifx, n_ifaces, kp, prefix, out, stream):
    """One gpd_pcapng_write: (rc, records, bytes, bad index, bad reason); out None is the sizing call."""
    nw, nb, bad, why = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
    b = dbatch.c_batch()
    rc = ngw_lib().gpd_pcapng_write(h, C.byref(b), _ptr(ts), _ptr(wl), _ptr(ifx), n_ifaces, _ptr(kp),
                                    prefix if prefix else None, len(prefix), _ptr(out),
                                    out.numel() if out is not None else 0, C.byref(nw), C.byref(nb),
                                    C.byref(bad), C.byref(why), C.c_void_p(stream.cuda_stream))
    return rc, nw.value, nb.value, bad.value, why.value


def write_device_ng(parser_or_ctx, dbatch, ts_ns, length=None, ifindex=None, n_ifaces: int = 1, keep=None,
                    prefix: bytes = b"", stream=None, out=None):
    """The kept packets of `dbatch` as enhanced packet blocks in HBM behind `prefix`
    (gpd_pcapng_write): returns (uint8 device tensor trimmed to the stream, records written).
    ts_ns (uint64, the bit pattern of Timestamp.UnixNano(), written raw), length
    (CaptureInfo.Length; None: the capture length), ifindex (CaptureInfo.InterfaceIndex; None:
    interface 0) and keep are torch device tensors or numpy arrays; n_ifaces is the number of
    interfaces the stream has described so far; prefix the host bytes in front of the first record
    (section and interface blocks).  Raises PcapError at the first kept packet on an interface
    that was not added or with capture length > length; its .stream and .n_written hold what the
    loop wrote before it, .bad_index the packet and .bad_reason which check (BAD_IFACE,
    BAD_LENGTH)."""
    from .parser import _torch
    torch = _torch()
    dev, n = dbatch.device, dbatch.n
    h = _ctx_handle(parser_or_ctx)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    ts = _dev(ts_ns, np.uint64, dev, n, "ts_ns")
    wl = _dev(length, np.uint32, dev, n, "length")
    ifx = _dev(ifindex, np.uint32, dev, n, "ifindex")
    kp = _keep_dev(keep, dev, n)
    prefix = bytes(prefix)
    args = (h, dbatch, ts, wl, ifx, int(n_ifaces), kp, prefix)
    # without an `out` that fits, a sizing call first (the scan alone), then the write
    rc, nw, nb, bad, why = _ng_write_call(*args, out, s)
    if rc not in (0, GPD_ERR_PCAP) and not (rc == GPD_ERR_INVALID and out is not None and nb > out.numel()):
        check(rc, "gpd_pcapng_write")
    if out is None or nb > out.numel():
        out = torch.empty(max(16, (nb + 15) & ~15), dtype=torch.uint8, device=torch.device("cuda", dev))
        rc, nw, nb, bad, why = _ng_write_call(*args, out, s)
    if rc == GPD_ERR_PCAP:
        e = PcapError(_lib.lib.gpd_last_error_string().decode())
        e.stream, e.n_written, e.bad_index, e.bad_reason = out[:nb], nw, bad, why
        raise e
    check(rc, "gpd_pcapng_write")
    return out[:nb], nw


class NgWriter:
    """pcapgo.NgWriter (ngwrite.go:45-397) over any object with .write: the section header and
    the first interface are written when it is made (NewNgWriterInterface, :66-79).  Written
    streams are little-endian with the interfaces' timestamp resolution fixed to 9."""

    def __init__(self, w, intf: NgInterface, options: NgWriterOptions):
        self.w = w
        self.options = options
        self.intf = 0  # interfaces added so far
        self.w.write(ng_section_block(options.SectionInfo))
        self.AddInterface(intf)

    def AddInterface(self, intf: NgInterface) -> int:
        """ngwrite.go:237-298: returns the new interface's id."""
        block = ng_interface_block(intf)
        i, self.intf = self.intf, self.intf + 1
        self.w.write(block)
        return i

    def WriteInterfaceStats(self, intf: int, stats: NgInterfaceStatistics) -> None:
        """ngwrite.go:301-353."""
        self.w.write(ng_stats_block(intf, self.intf, stats))

    def WritePacket(self, ci, data: bytes) -> None:
        """ngwrite.go:356-392 for one host packet.  The Timestamp is written as it is: the
        interface's TimestampOffset is not subtracted (a reader adds it again)."""
        if ci.InterfaceIndex >= self.intf or ci.InterfaceIndex < 0:
            raise PcapError(f"Can't send statistics for non existent interface {ci.InterfaceIndex}; "
                            f"have only {self.intf} interfaces")
        if ci.CaptureLength != len(data):
            raise PcapError(f"capture length {ci.CaptureLength} does not match data length {len(data)}")
        if ci.CaptureLength > ci.Length:
            raise PcapError(f"invalid capture info {ci!r}:  capture length > length")
        pad = (4 - (len(data) & 3)) & 3
        total = (len(data) + 32 + pad) & 0xFFFFFFFF
        ts = (0 if ci.Timestamp is None else int(ci.Timestamp)) & NgNoValue64
        self.w.write(struct.pack("<IIIIIII", 6, total, ci.InterfaceIndex, ts >> 32, ts & 0xFFFFFFFF,
                                 ci.CaptureLength & 0xFFFFFFFF, ci.Length & 0xFFFFFFFF))
        self.w.write(bytes(data))
        self.w.write(bytes(pad) + struct.pack("<I", total))

    def WritePackets(self, dbatch, ts_ns, length=None, ifindex=None, keep=None, parser=None) -> int:
        """The WritePacket loop over the kept packets of a DeviceBatch, on the device
        (gpd_pcapng_write); the records are copied back and written to w.  Returns the records
        written.  At a rejected packet the records before it are written, then PcapError raised
        with the reference's text, as the loop would have.  `parser` as for Writer.WritePackets."""
        if parser is None:
            parser = self._parser(dbatch.device)
        try:
            stream, nw = write_device_ng(parser, dbatch, ts_ns, length, ifindex, self.intf, keep)
        except PcapError as e:
            if getattr(e, "stream", None) is not None:
                self.w.write(e.stream.cpu().numpy().tobytes())
            raise
        self.w.write(stream.cpu().numpy().tobytes())
        return nw

    _parser = Writer._parser

    def Flush(self) -> None:
        """ngwrite.go:395-397: passes the flush on when w has one (nothing is buffered here)."""
        flush = getattr(self.w, "flush", None)
        if flush is not None:
            flush()


def NewNgWriterInterface(w, intf: NgInterface, options: NgWriterOptions) -> NgWriter:
    """pcapgo.NewNgWriterInterface (ngwrite.go:66-79)."""
    return NgWriter(w, intf, options)


def NewNgWriter(w, linktype: int) -> NgWriter:
    """pcapgo.NewNgWriter (ngwrite.go:56-60): DefaultNgInterface with the link type, and
    DefaultNgWriterOptions."""
    return NgWriter(w, replace(DefaultNgInterface, LinkType=int(linktype)), DefaultNgWriterOptions)
