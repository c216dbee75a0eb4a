"""The model of the TLS record decode: (*TLS).DecodeFromBytes (layers/tls.go:118-194) with the
four per-type decodeFromBytes (tls_cipherspec.go, tls_alert.go, tls_handshake.go, tls_appdata.go)
in plain Python, written from the reference and independent of gopacket_amd/csrc/gpd_tls_walk.h.
It works on slices as the reference does (each invocation is handed data[tl:]); `records` turns
its objects into the arrays include/gpd_tls.h describes."""
import numpy as np

MSG_DTYPE = np.dtype([("packet", "<u4"), ("data_off", "<u4"), ("data_len", "<u4"), ("first_record", "<u4"),
                      ("n_ccs", "<u4"), ("n_handshake", "<u4"), ("n_appdata", "<u4"), ("n_alert", "<u4"),
                      ("contents_off", "<u4"), ("err_off", "<u4"), ("verdict", "u1"), ("truncated", "u1"),
                      ("reserved", "u1", (6,))])
REC_DTYPE = np.dtype([("off", "<u4"), ("version", "<u2"), ("length", "<u2"), ("index_in_kind", "<u4"),
                      ("content_type", "u1"), ("a", "u1"), ("b", "u1"), ("flags", "u1")])

(OK, E_TOO_SHORT, E_UNKNOWN_TYPE, E_LENGTH_MISMATCH, E_CCS_LENGTH, E_ALERT_SHORT, E_APPDATA_LENGTH) = range(7)
DEFERRED = 255
TEXTS = {
    E_TOO_SHORT: "TLS record too short",
    E_UNKNOWN_TYPE: "Unknown TLS record type",
    E_LENGTH_MISMATCH: "TLS packet length mismatch",
    E_CCS_LENGTH: "TLS Change Cipher Spec record incorrect length",
    E_ALERT_SHORT: "TLS Alert packet too short",
    E_APPDATA_LENGTH: "TLS Application Data length mismatch",
}
# E_APPDATA_LENGTH cannot be returned (data[hl:tl] has Length bytes); tests/test_tls.py shows it
REACHABLE = {OK, E_TOO_SHORT, E_UNKNOWN_TYPE, E_LENGTH_MISMATCH, E_CCS_LENGTH, E_ALERT_SHORT}

TYPE_NAMES = {20: "Change Cipher Spec", 21: "Alert", 22: "Handshake", 23: "Application Data"}


class Err(Exception):
    def __init__(self, code):
        self.code = code
        super().__init__(TEXTS[code])


class Rec:
    """One appended record: the header, the per-type fields, and where it lay (off, in wire order)."""

    def __init__(self, h, off):
        self.ContentType, self.Version, self.Length = h
        self.off = off
        self.Message = self.Level = self.Description = 0
        self.Payload = b""
        self.EncryptedMsg = None


class TLS:
    def __init__(self):
        self.Contents = b""
        self.ChangeCipherSpec, self.Handshake, self.AppData, self.Alert = [], [], [], []
        self.err = None
        self.truncated = False
        self.work = 0          # decodeTLSRecords invocations
        self.order = []        # the appended records in wire order
        self.err_off = 0       # where the invocation that returned began
        self.contents_off = 0


def _ccs(r, data, t):                       # tls_cipherspec.go:37-54
    if len(data) != 1:
        t.truncated = True
        return Err(E_CCS_LENGTH)
    r.Message = data[0]
    if r.Message != 1:
        r.Message = 255
    return None


def _alert(r, data, t):                     # tls_alert.go:74-95
    if len(data) < 2:
        t.truncated = True
        return Err(E_ALERT_SHORT)
    if r.Length == 2:
        r.Level, r.Description = data[0], data[1]
    else:
        r.Level = r.Description = 255
        r.EncryptedMsg = data
    return None


def _handshake(r, data, t):                 # tls_handshake.go:19-28
    return None


def _appdata(r, data, t):                   # tls_appdata.go:22-34
    if len(data) != r.Length:
        return Err(E_APPDATA_LENGTH)
    r.Payload = data
    return None


def decode(data):
    """t.DecodeFromBytes(data): the TLS object as the call leaves it, with err, truncated, work."""
    data = bytes(data)
    t = TLS()
    t.Contents = data                       # :119
    base = 0                                # how far into the first call's data this invocation's begins
    while True:                             # decodeTLSRecords; `continue` is its tail call (:193)
        t.work += 1
        t.err_off = base
        if len(data) < 5:                   # :131-134
            t.truncated = True
            t.err = Err(E_TOO_SHORT)
            return t
        t.Contents = data                   # :139
        t.contents_off = base
        ct, ver, length = data[0], (data[1] << 8) | data[2], (data[3] << 8) | data[4]
        if TYPE_NAMES.get(ct, "Unknown") == "Unknown":  # :146-148
            t.err = Err(E_UNKNOWN_TYPE)
            return t
        hl = 5
        tl = hl + length
        if len(data) < tl:                  # :152-155
            t.truncated = True
            t.err = Err(E_LENGTH_MISMATCH)
            return t
        r = Rec((ct, ver, length), base)
        fn, lst = {20: (_ccs, t.ChangeCipherSpec), 21: (_alert, t.Alert), 22: (_handshake, t.Handshake),
                   23: (_appdata, t.AppData)}[ct]
        e = fn(r, data[hl:tl], t)
        if e is not None:
            t.err = e
            return t
        lst.append(r)
        t.order.append(r)
        if len(data) == tl:                 # :190-192
            t.err_off = base + tl
            return t
        data, base = data[tl:], base + tl


def records(t, data_len, max_records=0, packet=0, data_off=0, first_record=0):
    """(msg[1], recs[]) as include/gpd_tls.h describes them for the model's object `t`; with a
    budget (max_records > 0) a message whose work exceeds it is deferred."""
    m = np.zeros(1, MSG_DTYPE)
    m["packet"], m["data_off"], m["data_len"], m["first_record"] = packet, data_off, data_len, first_record
    if max_records and t.work > max_records:
        m["verdict"] = DEFERRED
        return m, np.zeros(0, REC_DTYPE)
    m["n_ccs"], m["n_handshake"], m["n_appdata"], m["n_alert"] = (len(t.ChangeCipherSpec), len(t.Handshake),
                                                                  len(t.AppData), len(t.Alert))
    m["contents_off"], m["err_off"] = t.contents_off, t.err_off
    m["verdict"] = t.err.code if t.err else OK
    m["truncated"] = int(t.truncated)
    r = np.zeros(len(t.order), REC_DTYPE)
    seen = {20: 0, 21: 0, 22: 0, 23: 0}
    for k, x in enumerate(t.order):
        r[k]["off"], r[k]["version"], r[k]["length"], r[k]["content_type"] = x.off, x.Version, x.Length, x.ContentType
        r[k]["index_in_kind"] = seen[x.ContentType]
        seen[x.ContentType] += 1
        if x.ContentType == 20:
            r[k]["a"] = x.Message
        elif x.ContentType == 21:
            r[k]["a"], r[k]["b"] = x.Level, x.Description
            r[k]["flags"] = 1 if x.EncryptedMsg is not None else 0
    return m, r
