"""The model of the connection tracker (include/gpd_tcptrack.h): reassembly's pool of
bidirectional connections as a dict with getHalf's two lookups (reassembly/memory.go:169-206), and
TCPSimpleFSM.CheckState restated line by line (reassembly/tcpcheck.go:167-246).  Pinned by the
reference's own FSM tests (tests/golden/tcpfsm_vectors.json) in tests/test_tcptrack.py; the kernels
are compared with it byte for byte in tests/test_tcptrack_gpu.py.
"""
import numpy as np

TCPStateClosed, TCPStateSynSent, TCPStateEstablished, TCPStateCloseWait, TCPStateLastAck, TCPStateReset = range(6)
STATE_NAMES = ("Closed", "SynSent", "Established", "CloseWait", "LastAck", "Reset")
TCPDirClientToServer, TCPDirServerToClient = False, True  # reassembly/tcpassembly.go: TCPFlowDirection bool
UNTRACKED = 0xFF
FLOW_NONE = 0xFFFFFFFF
# TCP header byte 13
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10


class TCPSimpleFSM:
    """tcpcheck.go:119-123; NewTCPSimpleFSM :141-146."""

    def __init__(self, support_missing_establishment=False):
        self.dir = TCPDirClientToServer
        self.state = TCPStateClosed
        self.SupportMissingEstablishment = bool(support_missing_establishment)

    def String(self):  # :148-164
        return STATE_NAMES[self.state] if 0 <= self.state < 6 else "?"

    def CheckState(self, SYN, ACK, FIN, RST, dir):  # :167-246
        t = self
        if t.state == TCPStateClosed and t.SupportMissingEstablishment and not (SYN and not ACK):
            # try to figure out state
            if SYN and ACK:
                t.state = TCPStateSynSent
                t.dir = not dir
            elif FIN and not ACK:
                t.state = TCPStateEstablished
            elif FIN and ACK:
                t.state = TCPStateCloseWait
                t.dir = not dir
            else:
                t.state = TCPStateEstablished
        if t.state == TCPStateClosed:
            if SYN and not ACK:
                t.dir = dir
                t.state = TCPStateSynSent
                return True
        elif t.state == TCPStateSynSent:
            if RST:
                t.state = TCPStateReset
                return True
            if SYN and ACK and dir == (not t.dir):
                t.state = TCPStateEstablished
                return True
            if SYN and not ACK and dir == t.dir:
                return True  # re-transmission
        elif t.state == TCPStateEstablished:
            if RST:
                t.state = TCPStateReset
                return True
            if FIN:
                t.state = TCPStateCloseWait
                t.dir = dir
                return True
            return True  # accept any packet
        elif t.state == TCPStateCloseWait:
            if RST:
                t.state = TCPStateReset
                return True
            if FIN and ACK and dir == (not t.dir):
                t.state = TCPStateLastAck
                return True
            if ACK:
                return True
        elif t.state == TCPStateLastAck:
            if RST:
                t.state = TCPStateReset
                return True
            if ACK and t.dir == dir:
                t.state = TCPStateClosed
                return True
        return False

    def carried(self):
        """The carried byte of include/gpd_tcptrack.h."""
        return self.state | (8 if self.dir else 0)


def step_table(support_missing_establishment):
    """CheckState for every (state, t.dir, code): rows (state, tdir, code, state', tdir', accept),
    code = SYN 1 | ACK 2 | FIN 4 | RST 8 | dir 16 (gpd_tcptrack_fsm.h)."""
    rows = []
    for state in range(6):
        for tdir in (False, True):
            for code in range(32):
                f = TCPSimpleFSM(support_missing_establishment)
                f.state, f.dir = state, tdir
                ok = f.CheckState(bool(code & 1), bool(code & 2), bool(code & 4), bool(code & 8), bool(code & 16))
                rows.append((state, int(tdir), code, f.state, int(f.dir), int(ok)))
    return rows


def reverse_key(k):
    """key.Reverse(): both flows reversed.  k = (src, dst, sport, dport) with anything hashable."""
    return (k[1], k[0], k[3], k[2])


class _Conn:
    def __init__(self, key, cid, sme):
        self.key, self.cid = key, cid
        self.fsm = TCPSimpleFSM(sme)


class Model:
    """StreamPool + one TCPSimpleFSM per connection.  `track` takes, per packet, its key (None:
    untracked), its TCP flag byte and its flow id (the connection's id is the flow id of the
    packet that created it, as the tracker's c is the record of the direction seen first)."""

    def __init__(self, support_missing_establishment=False, reverse=reverse_key):
        self.sme = bool(support_missing_establishment)
        self.conns = {}
        self.reverse = reverse  # key.Reverse() for the keys the caller uses

    def getHalf(self, k):  # memory.go:169-180
        conn = self.conns.get(k)
        if conn is not None:
            return conn, TCPDirClientToServer
        conn = self.conns.get(self.reverse(k))
        if conn is not None:
            return conn, TCPDirServerToClient
        return None, None

    def getConnection(self, k, flow_id):  # memory.go:185-206 with end == false
        conn, dir = self.getHalf(k)
        if conn is not None:
            return conn, dir
        conn = self.conns[k] = _Conn(k, flow_id, self.sme)
        return conn, TCPDirClientToServer

    def track(self, keys, flags, flow_ids):
        n = len(keys)
        verdict = np.full(n, UNTRACKED, np.uint8)
        conn_id = np.full(n, FLOW_NONE, np.uint32)
        touched = set()
        acc = 0
        for i in range(n):
            k = keys[i]
            if k is None:
                continue
            conn, dir = self.getConnection(k, int(flow_ids[i]))
            f = int(flags[i])
            ok = conn.fsm.CheckState(bool(f & SYN), bool(f & ACK), bool(f & FIN), bool(f & RST), dir)
            verdict[i] = int(ok) | (2 if dir else 0) | (conn.fsm.state << 2) | (0x20 if conn.fsm.dir else 0)
            conn_id[i] = conn.cid
            touched.add(conn.cid)
            acc += int(ok)
        tracked = int((verdict != UNTRACKED).sum())
        return verdict, conn_id, (tracked, acc, tracked - acc, len(touched))

    def states(self, id_bound):
        out = np.zeros(id_bound, np.uint8)
        for c in self.conns.values():
            out[c.cid] = c.fsm.carried()
        return out

    def forget(self, ids):
        """The listed connections back to the fresh FSM (their records, and so their direction,
        stay)."""
        ids = set(int(i) for i in ids)
        for c in self.conns.values():
            if c.cid in ids:
                c.fsm = TCPSimpleFSM(self.sme)

    def drop(self, keys, live=()):
        """StreamPool.remove of idle connections (memory.go:123-130): `keys` are the directional
        keys whose records left the pool, `live` the keys still in it.  A connection leaves once
        both of its records have: its own key is in `keys` and its reverse is not in `live`.  The
        tuple's next packet, from either side, then makes a new connection."""
        keys = set(keys)
        for k in [k for k in self.conns if k in keys and self.reverse(k) not in live]:
            del self.conns[k]

    def reset(self):
        for c in self.conns.values():
            c.fsm = TCPSimpleFSM(self.sme)
