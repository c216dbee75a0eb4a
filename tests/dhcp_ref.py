"""The model of the DHCP message decode: (*DHCPv4).DecodeFromBytes (layers/dhcpv4.go:126-179) with
(*DHCPOption).decode (:558-578), and (*DHCPv6).DecodeFromBytes (layers/dhcpv6.go:89-124) with
(*DHCPv6Option).decode (dhcpv6_options.go:610-621), in plain Python, written from the reference and
independent of gopacket_amd/csrc/gpd_dhcp_walk.h.  It works on slices as the reference does (each
option decode is handed options[start:] or data[offset:]); `records` turns its objects into the
arrays include/gpd_dhcp.h describes."""
import numpy as np

MSG_DTYPE = np.dtype([("packet", "<u4"), ("data_off", "<u4"), ("data_len", "<u4"), ("first_opt", "<u4"),
                      ("n_opts", "<u4"), ("xid", "<u4"), ("err_off", "<u4"), ("err_arg", "<u4"),
                      ("secs", "<u2"), ("flags", "<u2"), ("verdict", "u1"), ("truncated", "u1"), ("version", "u1"),
                      ("op", "u1"), ("htype", "u1"), ("hlen", "u1"), ("hops", "u1"), ("mflags", "u1"),
                      ("reserved", "u1", (4,))])
OPT_DTYPE = np.dtype([("off", "<u4"), ("code", "<u2"), ("length", "<u2")])

(OK, E_V4_TOO_SHORT, E_V4_BAD_MAGIC, E_V4_OPT_NO_DATA, E_V4_OPT_MALFORMED, E_V6_TOO_SHORT, E_V6_RELAY_SHORT,
 E_V6_OPT_NO_DATA, E_V6_OPT_SIZE, E_V4_OPT_EMPTY, E_V4_HW_PANIC) = range(11)
DEFERRED = 255
TEXTS = {
    E_V4_TOO_SHORT: "DHCPv4 length %d too short",
    E_V4_BAD_MAGIC: "Bad DHCP header",
    E_V4_OPT_NO_DATA: "Not enough data to decode",
    E_V4_OPT_MALFORMED: "Option is malformed",
    E_V6_TOO_SHORT: "DHCPv6 length %d too short",
    E_V6_RELAY_SHORT: "DHCPv6 length %d too short for message type %d",
    E_V6_OPT_NO_DATA: "not enough data to decode",
    E_V6_OPT_SIZE: "dhcpv6 option size < length %d",
    E_V4_OPT_EMPTY: "Not enough data to decode",
    # what DecodeLayers makes of the panic at dhcpv4.go:143 (parser.go:328-332)
    E_V4_HW_PANIC: "panic: runtime error: slice bounds out of range [28:%d]",
}
# E_V4_OPT_EMPTY (decode handed no byte) cannot be returned from inside `start < stop`
REACHABLE_V4 = {OK, E_V4_TOO_SHORT, E_V4_BAD_MAGIC, E_V4_OPT_NO_DATA, E_V4_OPT_MALFORMED, E_V4_HW_PANIC}
REACHABLE_V6 = {OK, E_V6_TOO_SHORT, E_V6_RELAY_SHORT, E_V6_OPT_NO_DATA, E_V6_OPT_SIZE}
REACHABLE = REACHABLE_V4 | REACHABLE_V6
F_CONTENTS, F_RELAY, F_HW_PAST_DATA = 1, 2, 4
MAGIC = 0x63825363


class Err(Exception):
    def __init__(self, code, *args):
        self.code, self.args_ = code, args
        super().__init__(TEXTS[code] % args if args else TEXTS[code])


class Opt:
    """One option: v4 (Type, Length uint8, Data or None), v6 (Code, Length uint16, Data); `off` is
    where it lay in data."""

    def __init__(self):
        self.Type = self.Code = self.Length = 0
        self.Data = None
        self.off = 0


def opt4_decode(o, data):                   # dhcpv4.go:558-578
    if len(data) < 1:
        return Err(E_V4_OPT_EMPTY)
    o.Type = data[0]
    if o.Type in (0, 255):
        o.Data = None
    else:
        if len(data) < 2:
            return Err(E_V4_OPT_NO_DATA)
        o.Length = data[1]
        if o.Length > len(data[2:]):
            return Err(E_V4_OPT_MALFORMED)
        o.Data = data[2:2 + o.Length]
    return None


def opt6_decode(o, data):                   # dhcpv6_options.go:610-621
    if len(data) < 4:
        return Err(E_V6_OPT_NO_DATA)
    o.Code = (data[0] << 8) | data[1]
    o.Length = (data[2] << 8) | data[3]
    if len(data) < 4 + o.Length:
        return Err(E_V6_OPT_SIZE, (4 + o.Length) & 0xFFFF)   # %d of a uint16 sum
    o.Data = data[4:4 + o.Length]
    return None


class Msg:
    def __init__(self, version):
        self.version = version
        self.Contents = None
        self.Options = []
        self.err = None
        self.truncated = False
        self.work = 0                       # option decodes begun
        self.err_off = 0
        self.assigned = False               # the header fields were assigned
        # v4
        self.Operation = self.HardwareType = self.HardwareLen = self.HardwareOpts = 0
        self.Xid = self.Secs = self.Flags = 0
        self.ClientIP = self.YourClientIP = self.NextServerIP = self.RelayAgentIP = None
        self.ClientHWAddr = self.ServerName = self.File = None
        self.hw_past_data = False
        # v6
        self.MsgType = self.HopCount = 0
        self.LinkAddr = self.PeerAddr = self.TransactionID = None
        self.relay = False


def decode4(data):
    """d.DecodeFromBytes(data) of a fresh DHCPv4 (a reused object would keep its Options through
    the too-short return; that is not modelled)."""
    data = bytes(data)
    d = Msg(4)
    if len(data) < 240:                     # :127-130
        d.truncated = True
        d.err = Err(E_V4_TOO_SHORT, len(data))
        return d
    d.assigned = True
    d.Options = []                          # :131
    d.Operation, d.HardwareType, d.HardwareLen, d.HardwareOpts = data[0], data[1], data[2], data[3]
    d.Xid = int.from_bytes(data[4:8], "big")
    d.Secs = int.from_bytes(data[8:10], "big")
    d.Flags = int.from_bytes(data[10:12], "big")
    d.ClientIP, d.YourClientIP, d.NextServerIP, d.RelayAgentIP = data[12:16], data[16:20], data[20:24], data[24:28]
    high = (28 + d.HardwareLen) & 0xFF      # :143: 28+d.HardwareLen is a uint8 sum
    if high < 28:                           # the slice expression panics, whatever the buffer
        d.err = Err(E_V4_HW_PANIC, high)
        d.err_off = 28
        return d
    # past len the reference slices by capacity; the model clips to data and says so (include/gpd_dhcp.h)
    d.hw_past_data = high > len(data)
    d.ClientHWAddr = data[28:high]
    d.ServerName, d.File = data[44:108], data[108:236]
    if int.from_bytes(data[236:240], "big") != MAGIC:   # :146-148
        d.err = Err(E_V4_BAD_MAGIC)
        d.err_off = 236
        return d
    if len(data) <= 240:                    # :150-153
        d.err_off = len(data)
        return d
    options = data[240:]
    stop, start = len(options), 0
    while start < stop:                     # :159-174
        o = Opt()
        d.work += 1
        e = opt4_decode(o, options[start:])
        if e is not None:
            d.err = e
            d.err_off = 240 + start
            return d
        if o.Type == 255:
            break
        o.off = 240 + start
        d.Options.append(o)
        start += 1 if o.Type == 0 else o.Length + 2
    d.Contents = data                       # :176
    d.err_off = len(data)
    return d


def decode6(data):
    data = bytes(data)
    d = Msg(6)
    if len(data) < 4:                       # :90-93
        d.truncated = True
        d.err = Err(E_V6_TOO_SHORT, len(data))
        return d
    d.assigned = True
    d.Contents = data                       # :94
    d.MsgType = data[0]
    if d.MsgType in (12, 13):               # :99-107
        if len(data) < 34:
            d.truncated = True
            d.err = Err(E_V6_RELAY_SHORT, len(data), d.MsgType)
            return d
        d.relay = True
        d.HopCount, d.LinkAddr, d.PeerAddr = data[1], data[2:18], data[18:34]
        offset = 34
    else:
        d.TransactionID = data[1:4]
        offset = 4
    stop = len(data)
    while offset < stop:                    # :114-121
        o = Opt()
        d.work += 1
        e = opt6_decode(o, data[offset:])
        if e is not None:
            d.err = e
            d.err_off = offset
            return d
        o.off = offset
        d.Options.append(o)
        offset += o.Length + 4
    d.err_off = len(data)
    return d


def decode(version, data):
    return decode4(data) if version == 4 else decode6(data)


def records(d, data_len, max_options=0, packet=0, data_off=0, first_opt=0):
    """(msg[1], opts[]) as include/gpd_dhcp.h describes them for the model's object `d`; with a
    budget (max_options > 0) a message whose work exceeds it is deferred."""
    m = np.zeros(1, MSG_DTYPE)
    m["packet"], m["data_off"], m["data_len"], m["version"] = packet, data_off, data_len, d.version
    m["first_opt"] = first_opt
    if max_options and d.work > max_options:
        m["verdict"] = DEFERRED
        return m, np.zeros(0, OPT_DTYPE)
    m["n_opts"], m["err_off"] = len(d.Options), d.err_off
    m["verdict"] = d.err.code if d.err else OK
    m["truncated"] = int(d.truncated)
    if d.err is not None and d.err.args_:
        m["err_arg"] = d.err.args_[0]
    flags = F_CONTENTS if d.Contents is not None else 0
    if d.version == 4 and d.assigned:
        m["op"], m["htype"], m["hlen"], m["hops"] = d.Operation, d.HardwareType, d.HardwareLen, d.HardwareOpts
        m["xid"], m["secs"], m["flags"] = d.Xid, d.Secs, d.Flags
        flags |= F_HW_PAST_DATA if d.hw_past_data else 0
    elif d.version == 6 and d.assigned:
        m["op"] = d.MsgType
        if d.relay:
            flags |= F_RELAY
            m["hops"] = d.HopCount
        elif d.TransactionID is not None:
            m["xid"] = int.from_bytes(d.TransactionID, "big")
    m["mflags"] = flags
    o = np.zeros(len(d.Options), OPT_DTYPE)
    for k, x in enumerate(d.Options):
        o[k]["off"], o[k]["code"], o[k]["length"] = x.off, x.Type if d.version == 4 else x.Code, x.Length
    return m, o
