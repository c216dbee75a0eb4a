"""A plain-Python sequential restatement of pcapgo's NgReader (pcapgo/ngread.go, paths relative
to google/gopacket) — test infrastructure: the yardstick the native reader of
include/gpd_pcapng.h is compared with.  Nothing under gopacket_amd/ imports it.

It follows the Go text method by method, with the stream as (bytes, position):
  readBytes :89-99, readBlock :127-152, readOption :155-193, readSectionHeader :197-269,
  skipSection :272-284, SkipSection :287-292, firstInterface :295-322,
  readInterfaceDescriptor :325-386, convertTime :389-392, readInterfaceStatistics :395-438,
  readPacketHeader :443-525, ReadPacketData :529-545.
Arithmetic on block lengths is Go's wrapping uint32 (uint16 for an option's length + padding,
uint64 in convertTime).  Two decisions of include/gpd_pcapng.h are restated with it: a stop of
its own (PANIC) where the reference panics (integer division by a zero secondMask), and where
an option value is shorter than the reference indexes it.
"""
import struct

(STOP_LIMIT, STOP_EOF, STOP_EOF_BLOCK, STOP_NEGATIVE, STOP_IFACE_ID, STOP_NO_IFACE, STOP_NO_FIRST,
 STOP_BYTE_ORDER, STOP_OPT_END, STOP_VERSION, STOP_LINKTYPE, STOP_PANIC, STOP_MAGIC) = range(13)

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
SHB, IDB, PB, SPB, ISB, EPB = 0x0A0D0D0A, 1, 2, 3, 5, 6


class Stop(Exception):
    def __init__(self, stop, text):
        super().__init__(text)
        self.stop, self.text = stop, text


class Interface:
    def __init__(self):
        self.Name = self.Comment = self.Description = self.Filter = self.OS = b""
        self.LinkType = self.SnapLength = self.TimestampResolution = self.TimestampOffset = 0
        self.secondMask = self.scaleUp = self.scaleDown = 0


class NgReaderRef:
    def __init__(self, data, want_mixed=False, error_on_mismatch=False, skip_unknown=False,
                 section_end=None):
        self.section_end, self.activeSection = section_end, False   # SectionEndCallback, :31-33
        self.d, self.pos, self.blk_pos = bytes(data), 0, 0
        self.want_mixed, self.error_on_mismatch, self.skip_unknown = want_mixed, error_on_mismatch, skip_unknown
        self.section = dict(Hardware=b"", OS=b"", Application=b"", Comment=b"")
        self.linkType = 0
        self.ifaces = []
        self.typ = self.length = 0
        self.code, self.value = 0, bytes(1024)   # currentOption.value: make([]byte, 1024), :64-66
        self.firstSectionFound = False
        self.bigEndian = False
        self.stopped = None                      # (stop, text) once the reader has failed
        try:                                     # NewNgReader :61-83
            self.readBlock()
            if self.typ != SHB:
                raise Stop(STOP_MAGIC, "Unknown magic %x" % self.typ)
            self.readSectionHeader()
        except Stop as s:
            self.stopped = (s.stop, s.text)

    # -- the stream ---------------------------------------------------------------------------
    def readBytes(self, n):
        if len(self.d) - self.pos < n:
            self.pos = len(self.d)
            raise Stop(STOP_EOF_BLOCK, "EOF")
        b = self.d[self.pos:self.pos + n]
        self.pos += n
        return b

    def discard(self, n):                        # bufio.Reader.Discard
        if n < 0:
            raise Stop(STOP_NEGATIVE, "bufio: negative count")
        if n:
            self.readBytes(n)

    def u16(self, b):
        return struct.unpack(">H" if self.bigEndian else "<H", b)[0]

    def u32(self, b):
        return struct.unpack(">I" if self.bigEndian else "<I", b)[0]

    def u64(self, b):
        return struct.unpack(">Q" if self.bigEndian else "<Q", b)[0]

    # -- blocks -------------------------------------------------------------------------------
    def readBlock(self):
        self.blk_pos = self.pos
        if self.pos == len(self.d):              # nothing where a block header would start
            raise Stop(STOP_EOF, "EOF")
        buf = self.readBytes(8)
        self.typ = self.u32(buf[0:4])
        if self.typ == SHB:
            bo = self.readBytes(4)
            if struct.unpack(">I", bo)[0] == 0x1A2B3C4D:
                self.bigEndian = True
            elif struct.unpack("<I", bo)[0] == 0x1A2B3C4D:
                self.bigEndian = False
            else:
                raise Stop(STOP_BYTE_ORDER, "Wrong byte order value in Section Header")
            self.length = (self.u32(buf[4:8]) - 12) & M32
            return
        self.length = (self.u32(buf[4:8]) - 8) & M32

    def readOption(self):
        """Returns the option's own length field (0: self.value keeps the previous option's)."""
        if self.length == 4:
            self.code = 0
            return 0
        buf = self.readBytes(4)
        self.length = (self.length - 4) & M32
        self.code = self.u16(buf[0:2])
        length = self.u16(buf[2:4])
        if self.code == 0:
            if length != 0:
                raise Stop(STOP_OPT_END, "End of Options must be zero length")
            return 0
        if length != 0:
            self.value = self.readBytes(length)
            padding = length % 4
            if padding > 0:
                padding = 4 - padding
                self.discard(padding)
            self.length = (self.length - ((length + padding) & 0xFFFF)) & M32
        return length

    @staticmethod
    def short(what, need, have):
        return Stop(STOP_PANIC, "the reference panics here: %s option of %d bytes read as %d" % (what, have, need))

    def readSectionHeader(self):
        if self.section_end is not None and self.activeSection:     # :198-204
            self.section_end(list(self.ifaces), dict(self.section))
        self.ifaces = []
        self.activeSection = False
        while True:
            buf = self.readBytes(12)
            self.length = (self.length - 12) & M32
            if self.u16(buf[0:2]) == 1 and self.u16(buf[2:4]) == 0:
                break
            if not self.skip_unknown:
                raise Stop(STOP_VERSION, "Unknown pcapng Version in Section Header")
            self.discard(self.length)
            self.skipSection()
        section = dict(Hardware=b"", OS=b"", Application=b"", Comment=b"")
        while True:
            self.readOption()
            if self.code == 0:
                break
            key = {1: "Comment", 2: "Hardware", 3: "OS", 4: "Application"}.get(self.code)
            if key:
                section[key] = self.value
        self.discard(self.length)
        self.activeSection = True
        self.section = section
        if not self.want_mixed:
            self.firstInterface()

    def skipSection(self):
        while True:
            self.readBlock()
            if self.typ == SHB:
                return
            self.discard(self.length)

    def SkipSection(self):
        if self.stopped:
            return self.stopped
        try:
            self.skipSection()
            self.readSectionHeader()
        except Stop as s:
            self.stopped = (s.stop, s.text)
            return self.stopped
        return (0, None)

    def firstInterface(self):
        while True:
            self.readBlock()
            if self.typ == IDB:
                self.readInterfaceDescriptor()
                if not self.firstSectionFound:
                    self.linkType = self.ifaces[0].LinkType
                    self.firstSectionFound = True
                elif self.linkType != self.ifaces[0].LinkType:
                    if self.error_on_mismatch:
                        raise Stop(STOP_LINKTYPE, "Link type of current interface is different from first one")
                    continue
                return
            if self.typ in (PB, EPB, SPB, ISB):
                raise Stop(STOP_NO_FIRST, "A section must have an interface before a packet block")
            self.discard(self.length)

    def readInterfaceDescriptor(self):
        buf = self.readBytes(8)
        self.length = (self.length - 8) & M32
        intf = Interface()
        intf.LinkType = self.u16(buf[0:2])
        intf.SnapLength = self.u32(buf[4:8])
        while True:
            n = self.readOption()
            c = self.code
            if c == 0:
                break
            if c == 2:
                intf.Name = self.value
            elif c == 1:
                intf.Comment = self.value
            elif c == 3:
                intf.Description = self.value
            elif c == 11:
                if n < 1:
                    raise self.short("if_filter", 1, n)
                intf.Filter = self.value[1:]
            elif c == 12:
                intf.OS = self.value
            elif c == 14:
                if n < 8:
                    raise self.short("if_tsoffset", 8, n)
                intf.TimestampOffset = self.u64(self.value[:8])
            elif c == 9:
                if n < 1:
                    raise self.short("if_tsresol", 1, n)
                intf.TimestampResolution = self.value[0]
        self.discard(self.length)
        if intf.TimestampResolution == 0:
            intf.TimestampResolution = 6
        e = intf.TimestampResolution & 0x7F
        if intf.TimestampResolution & 0x80:
            intf.secondMask = (1 << e) & M64
        else:
            intf.secondMask = pow(10, e) & M64   # the multiplication loop wraps
        intf.scaleDown = intf.scaleUp = 1
        if intf.secondMask < 10**9:
            if intf.secondMask == 0:
                raise Stop(STOP_PANIC, "the reference panics here: integer divide by zero "
                           "(timestamp resolution %d)" % intf.TimestampResolution)
            intf.scaleUp = 10**9 // intf.secondMask
        else:
            intf.scaleDown = intf.secondMask // 10**9
        self.ifaces.append(intf)

    def convertTime(self, i, ts):
        f = self.ifaces[i]
        sec = (ts // f.secondMask + f.TimestampOffset) & M64
        nsec = ((ts % f.secondMask) * f.scaleUp & M64) // f.scaleDown
        if nsec >= 1 << 63:
            nsec -= 1 << 64                      # int64(...)
        if nsec < 0 or nsec >= 10**9:            # time.Unix
            q = abs(nsec) // 10**9 * (1 if nsec > 0 else -1)   # Go's / truncates toward zero
            sec = (sec + q) & M64
            nsec -= q * 10**9
            if nsec < 0:
                nsec += 10**9
                sec = (sec - 1) & M64
        if sec >= 1 << 63:
            sec -= 1 << 64
        return sec, nsec

    def readInterfaceStatistics(self):
        buf = self.readBytes(12)
        self.length = (self.length - 12) & M32
        ifaceID = self.u32(buf[0:4])
        if ifaceID >= len(self.ifaces):
            raise Stop(STOP_IFACE_ID, "Interface id %d not present in section (have only %d interfaces)"
                       % (ifaceID, len(self.ifaces)))
        while True:
            n = self.readOption()
            if self.code == 0:
                break
            if 2 <= self.code <= 5 and n < 8:
                raise self.short("statistics", 8, n)
        self.discard(self.length)

    def readPacketHeader(self):
        while True:
            while True:
                self.readBlock()
                t = self.typ
                if t in (EPB, PB):
                    buf = self.readBytes(20)
                    self.length = (self.length - 20) & M32
                    idx = self.u32(buf[0:4]) if t == EPB else self.u16(buf[0:2])
                    if idx >= len(self.ifaces):
                        raise Stop(STOP_IFACE_ID, "Interface id %d not present in section (have only %d "
                                   "interfaces)" % (idx, len(self.ifaces)))
                    sec, nsec = self.convertTime(idx, self.u32(buf[4:8]) << 32 | self.u32(buf[8:12]))
                    ci = dict(ifindex=idx, sec=sec, nsec=nsec, caplen=self.u32(buf[12:16]),
                              wirelen=self.u32(buf[16:20]))
                    break
                if t == SPB:
                    buf = self.readBytes(4)
                    self.length = (self.length - 4) & M32
                    ln = self.u32(buf)
                    ci = dict(ifindex=0, sec=0, nsec=0, caplen=ln, wirelen=ln)
                    if not self.ifaces:
                        raise Stop(STOP_NO_IFACE, "At least one Interface is needed for a packet")
                    if self.ifaces[0].SnapLength != 0 and ci["caplen"] > self.ifaces[0].SnapLength:
                        ci["caplen"] = self.ifaces[0].SnapLength
                    break
                if t == IDB:
                    self.readInterfaceDescriptor()
                elif t == ISB:
                    self.readInterfaceStatistics()
                elif t == SHB:
                    self.readSectionHeader()
                else:
                    self.discard(self.length)
            ci["linktype"] = self.ifaces[ci["ifindex"]].LinkType
            if not self.want_mixed and ci["linktype"] != self.linkType:
                self.discard(self.length)
                if self.error_on_mismatch:
                    raise Stop(STOP_LINKTYPE, "Link type of current interface is different from first one")
                continue
            return ci

    def ReadPacketData(self):
        """One packet as a dict (off = where its bytes lie), or raises Stop."""
        ci = self.readPacketHeader()
        ci["off"] = self.pos
        self.readBytes(ci["caplen"])
        self.discard(self.length - ci["caplen"])
        return ci

    def read(self, max_n=None):
        """The ReadPacketData loop: (packets, stop, text or None).  LIMIT and a clean EOF carry no text."""
        out = []
        while max_n is None or len(out) < max_n:
            if self.stopped:
                s, t = self.stopped
                return out, s, (None if s == STOP_EOF else t)
            try:
                out.append(self.ReadPacketData())
            except Stop as s:
                self.stopped = (s.stop, s.text)
        return out, STOP_LIMIT, None

    def position(self):
        return self.blk_pos if self.stopped else self.pos
