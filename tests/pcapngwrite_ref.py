"""A plain-Python restatement of pcapgo's NgWriter (pcapgo/ngwrite.go, paths relative to
google/gopacket) — test infrastructure: the yardstick the builders and gpd_pcapng_write
(include/gpd_pcapngwrite.h) are compared with.  Nothing under gopacket_amd/ imports it, and it
imports nothing from there: every block is put together here with struct.pack.

  options          prepareNgOptions :102-115 + writeOptions :118-184
  section_block    writeSectionHeader :187-234
  interface_block  AddInterface :237-298
  stats_block      WriteInterfaceStats :301-353
  record           WritePacket :367-391
  write            the loop `for i in kept, ascending: w.WritePacket(ci[i], data[i])`, which ends at
                   the first kept packet on an interface that was not added (:357-359) or with
                   CaptureLength > Length (:363-365)
"""
import struct

import numpy as np

NO_BAD = 0xFFFFFFFFFFFFFFFF
NO_VALUE64 = 0xFFFFFFFFFFFFFFFF
BAD_NONE, BAD_IFACE, BAD_LENGTH = 0, 1, 2
IFACE_TEXT = "Can't send statistics for non existent interface %d; have only %d interfaces"
LENGTH_TEXT = "invalid capture info (packet %d: capture length %d, length %d):  capture length > length"


def _pad(k):
    return (4 - (k & 3)) & 3


def options(opts):
    """opts: (code, value) with value bytes, ("time", ns), ("u64", v) or ("u8", v)."""
    out = b""
    for code, val in opts:
        if isinstance(val, (bytes, bytearray)):
            body = bytes(val) + bytes(_pad(len(val)))
            ln = len(val)
        elif val[0] == "time":  # high word first
            ts = val[1] & 0xFFFFFFFFFFFFFFFF
            body, ln = struct.pack("<II", ts >> 32, ts & 0xFFFFFFFF), 8
        elif val[0] == "u64":
            body, ln = struct.pack("<Q", val[1]), 8
        else:  # one byte kept in four
            body, ln = struct.pack("<I", val[1] & 0xFF), 1
        out += struct.pack("<HH", code, ln) + body
    if opts:
        out += struct.pack("<HH", 0, 0)
    return out


def section_block(hardware=b"", os_=b"", application=b"", comment=b""):
    o = options([(c, v) for c, v in ((4, application), (1, comment), (2, hardware), (3, os_)) if v])
    total = len(o) + 24 + 4
    return (struct.pack("<IIIHHQ", 0x0A0D0D0A, total, 0x1A2B3C4D, 1, 0, 0xFFFFFFFFFFFFFFFF) + o +
            struct.pack("<I", total))


def interface_block(linktype=1, snaplen=0, name=b"", comment=b"", description=b"", filter_=b"", os_=b"",
                    tsoffset=0):
    opts = [(c, v) for c, v in ((2, name), (1, comment), (3, description)) if v]
    if filter_:
        opts.append((11, b"\0" + filter_))
    if os_:
        opts.append((12, os_))
    if tsoffset:
        opts.append((14, ("u64", tsoffset)))
    opts.append((9, ("u8", 9)))
    o = options(opts)
    total = len(o) + 16 + 4
    return struct.pack("<IIHHI", 1, total, linktype & 0xFFFF, 0, snaplen) + o + struct.pack("<I", total)


def stats_block(intf, n_ifaces, last_update=None, start=None, end=None, received=NO_VALUE64,
                dropped=NO_VALUE64):
    """Times in Unix ns, None for Go's zero time.  Returns the block, or raises ValueError with the
    reference's text."""
    if intf >= n_ifaces or intf < 0:
        raise ValueError(IFACE_TEXT % (intf, n_ifaces))
    opts = []
    if start is not None:
        opts.append((2, ("time", start)))
    if end is not None:
        opts.append((3, ("time", end)))
    if dropped != NO_VALUE64:
        opts.append((5, ("u64", dropped)))
    if received != NO_VALUE64:
        opts.append((4, ("u64", received)))
    o = options(opts)
    total = len(o) + 24
    ts = 0 if last_update is None else last_update & 0xFFFFFFFFFFFFFFFF
    return struct.pack("<IIIII", 5, total, intf, ts >> 32, ts & 0xFFFFFFFF) + o + struct.pack("<I", total)


def record(ts_ns, ifindex, caplen, length, data):
    total = 32 + caplen + _pad(caplen)
    ts = int(ts_ns) & 0xFFFFFFFFFFFFFFFF
    return (struct.pack("<IIIIIII", 6, total, ifindex, ts >> 32, ts & 0xFFFFFFFF, caplen, length & 0xFFFFFFFF) +
            bytes(data) + bytes(_pad(caplen)) + struct.pack("<I", total))


def kept_indices(n, keep):
    return np.arange(n) if keep is None else np.nonzero(np.asarray(keep) != 0)[0]


def write(batch, ts_ns, length=None, ifindex=None, n_ifaces=1, keep=None, prefix=b""):
    """(stream bytes, records written, bad index or NO_BAD, BAD_* reason).  A descriptor is
    clamped to the batch's data_len as the decode clamps it."""
    out = [bytes(prefix)]
    n_written, bad, reason = 0, NO_BAD, BAD_NONE
    data, off, cap, dlen = batch.data, batch.offset, batch.caplen, int(batch.data_len)
    for i in kept_indices(batch.n, keep):
        i = int(i)
        o = min(int(off[i]), dlen)
        c = min(int(cap[i]), dlen - o)
        wl = c if length is None else int(length[i])
        ifx = 0 if ifindex is None else int(ifindex[i])
        if ifx >= n_ifaces:
            bad, reason = i, BAD_IFACE
            break
        if c > wl:
            bad, reason = i, BAD_LENGTH
            break
        out.append(record(ts_ns[i], ifx, c, wl, data[o:o + c].tobytes()))
        n_written += 1
    return b"".join(out), n_written, bad, reason

