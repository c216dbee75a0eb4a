"""A plain-Python restatement of pcapgo's Writer (pcapgo/write.go:80-129, paths relative to
google/gopacket) — test infrastructure: the yardstick gpd_pcap_write and gpd_batch_select
(include/gpd_pcapwrite.h) are compared with.  Nothing under gopacket_amd/ imports it.

  file_header  WriteFileHeader :80-96
  record       writePacketHeader :101-114 + the data write of WritePacket :127
  write        the loop `for i in kept, ascending: w.WritePacket(ci[i], data[i])`, which ends at
               the first kept packet with CaptureLength > Length (:121-123)
  select       the kept packets as a dense batch of 16-byte aligned slots
"""
import struct

import numpy as np

MAGIC_MICRO, MAGIC_NANO = 0xA1B2C3D4, 0xA1B23C4D
NO_BAD = 0xFFFFFFFFFFFFFFFF


def file_header(snaplen, linktype, nanos=False):
    buf = bytearray(24)
    struct.pack_into("<I", buf, 0, MAGIC_NANO if nanos else MAGIC_MICRO)
    struct.pack_into("<HH", buf, 4, 2, 4)
    # bytes 8:16 stay 0 (timezone, sigfigs)
    struct.pack_into("<II", buf, 16, snaplen & 0xFFFFFFFF, linktype & 0xFFFFFFFF)
    return bytes(buf)


def record(ts_ns, caplen, length, data, nanos=False):
    secs, nsec = divmod(int(ts_ns), 1000000000)
    sub = nsec // (1 if nanos else 1000)
    return struct.pack("<IIII", secs & 0xFFFFFFFF, sub & 0xFFFFFFFF, caplen & 0xFFFFFFFF,
                       length & 0xFFFFFFFF) + bytes(data)


def kept_indices(n, keep):
    return np.arange(n) if keep is None else np.nonzero(np.asarray(keep) != 0)[0]


def write(batch, ts_ns, length=None, keep=None, nanos=False, header=None):
    """(stream bytes, records written, bad index or NO_BAD).  header: None or (snaplen, linktype)."""
    out = [file_header(header[0], header[1], nanos)] if header is not None else []
    n_written, bad = 0, NO_BAD
    data, off, cap = batch.data, batch.offset, batch.caplen
    for i in kept_indices(batch.n, keep):
        i = int(i)
        o, c = int(off[i]), int(cap[i])
        wl = c if length is None else int(length[i])
        if c > wl:
            bad = i
            break
        out.append(record(ts_ns[i], c, wl, data[o:o + c].tobytes(), nanos))
        n_written += 1
    return b"".join(out), n_written, bad


def select(batch, keep=None):
    """(data bytes, offsets, caplens, indices) of the kept packets in 16-byte slots."""
    idx = kept_indices(batch.n, keep)
    parts, offs, pos = [], [], 0
    for i in idx:
        o, c = int(batch.offset[i]), int(batch.caplen[i])
        slot = (c + 15) // 16 * 16
        parts.append(batch.data[o:o + c].tobytes() + bytes(slot - c))
        offs.append(pos)
        pos += slot
    return (b"".join(parts), np.array(offs, np.uint32), batch.caplen[idx].astype(np.uint32),
            idx.astype(np.uint32))
