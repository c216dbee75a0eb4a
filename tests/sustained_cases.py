"""TEST INFRASTRUCTURE ONLY: a long capture cut into batches, for the flow table with expiry, the
connection tracker and the stateful assembler run together (tests/test_sustained.py,
tests/test_sustained_gpu.py), and the truth they are compared with.

The device keeps the consumers' state in arrays indexed by record id, and expiry hands a removed
record's id to the next new key.  The reference keys everything by the connection's tuple
(tcpassembly.StreamPool, reassembly's getConnection, StreamPool.remove, FlushCloseOlderThan), so
`Truth` composes the existing models by tuple and never sees an id: tests/flow_expire_ref.Pool,
a tests/tcptrack_ref.Model whose connections leave with their records (`drop`), and one
tests/tcpasm_ref.StatefulAssembler per directional tuple.  `IdKeyed` is the same composition with
the state in slots by id, as the device has it, with the reset or the hold left out on request: what
the tests must be able to tell from the truth.

Traffic builds on tests/tcptrack_cases.py (LIFE, gen_connections, interleaved and its endpoints)
and tests/tcpstream_cases.gen_groups; TCP frames are synth.tcp_frame's, the noise frames are
tcptrack_cases.frames'.  Host only (numpy)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import flow_expire_ref as ER
import oracle_ref as O
import tcpasm_ref as AR
import tcpseg_ref as TS
import tcptrack_ref as TR
from gopacket_amd import layers as L
from gopacket_amd import synth
from gopacket_amd.batch import PacketBatch
from tcpstream_cases import gen_groups
from tcptrack_cases import ACK, FIN, LIFE, PSH, RST, SYN, TCP, UDP, endpoints, frames, gen_connections, interleaved

MASK = 0xFFF
SECOND = 10**9
IDLE = 2       # batches a record stays after its last packet before Expire takes it
FLUSH_AGE = 3  # batches a page or an idle connection waits for FlushOlderThan: an idle record can still be held
KINDS = ("full", "rst", "server_first", "oneway", "midstream", "displaced", "lost", "abandoned", "return_live",
         "return_expired", "chaos")
WEIGHTS = (0.20, 0.08, 0.08, 0.10, 0.08, 0.09, 0.08, 0.09, 0.07, 0.07, 0.06)
ISNS = (5, 1000, 1 << 31, (1 << 32) - 50, (1 << 32) - 1)
SPANS = (0.40, 0.25, 0.15, 0.10, 0.05, 0.05)  # a connection runs over 1 to 6 batches, short ones more often
PAYLOADS = (1, 3, 10, 100, 600, 1900, 1901, 4000)
PAYLOAD_WEIGHTS = (0.15, 0.15, 0.30, 0.25, 0.10, 0.02, 0.02, 0.01)

# a script: its kind, the connection number j (tcptrack_cases.endpoints), the batch it starts in
# and its steps (batch relative to start, from the server?, flag byte, seq, payload)
Script = namedtuple("Script", "kind j start steps")
# a batch: the frames, each packet's key (flow_expire_ref.key_of's 40 bytes; None: no key) and
# 4-tuple, whether it is TCP, its flag byte, seq, payload, timestamp (ns); index_base
Batch = namedtuple("Batch", "frames keys tuples tcp flags seq payload stamps base")


class _Stream:
    """The two directions' sequence counters of one connection: SYN and FIN take one number."""

    def __init__(self, rng):
        self.rng = rng
        self.seq = [int(ISNS[rng.integers(len(ISNS))]), int(rng.integers(1 << 32))]

    def step(self, fl, srv):
        n = 0
        if fl & PSH:
            n = int(PAYLOADS[self.rng.choice(len(PAYLOADS), p=PAYLOAD_WEIGHTS)])
        seq = self.seq[srv]
        self.seq[srv] = (seq + n + (1 if fl & (SYN | FIN) else 0)) & 0xFFFFFFFF
        return [srv, fl, seq, self.rng.bytes(n)]


def _rounds(rng, lo=2, hi=5):
    """Data both ways, LIFE[3:6] over and over: at least two segments per direction."""
    out = []
    for _ in range(int(rng.integers(lo, hi + 1))):
        out += [LIFE[3], LIFE[3]] if rng.random() < 0.4 else [LIFE[3]]
        out += [LIFE[4], LIFE[5]]
    return out


def _spread(rng, n, span):
    """n steps over `span` batches in order, none of the batches empty."""
    span = min(span, n)
    cuts = np.sort(rng.choice(np.arange(1, n), span - 1, replace=False)) if span > 1 else []
    return np.searchsorted(cuts, np.arange(n), side="right")


def _life(rng, kind):
    """One connection of `kind` as steps (relative batch, srv, flags, seq, payload)."""
    st = _Stream(rng)
    head, tail, span = LIFE[:3], LIFE[6:], 1 + int(rng.choice(6, p=SPANS))
    if kind == "rst":
        tail = [(RST | ACK, int(rng.integers(2)))]
    elif kind == "server_first":
        head = LIFE[1:3]
    elif kind == "midstream":
        head = []
    elif kind == "abandoned":
        tail = []
    elif kind in ("displaced", "lost"):
        span = int(rng.integers(3, 7))
    steps = [st.step(fl, srv) for fl, srv in list(head) + _rounds(rng) + list(tail)]
    at = _spread(rng, len(steps), span)
    steps = [(int(b), *s) for b, s in zip(at, steps)]
    if kind in ("displaced", "lost"):
        # a client data segment with another one behind it (in its own batch, where there is one)
        data = [k for k, s in enumerate(steps) if not s[1] and len(s[4])]
        near = [k for k, nxt in zip(data, data[1:]) if steps[nxt][0] == steps[k][0]]
        cand = near if near and kind == "displaced" else data[:-1]
        moved = steps.pop(cand[int(rng.integers(len(cand)))])
        if kind == "displaced":  # one or two batches late, behind what its new batch had of this connection
            steps.append((moved[0] + int(rng.integers(1, 3)), *moved[1:]))
            steps.sort(key=lambda s: s[0])
    return steps


def _oneway(rng, group):
    """A tcpstream_cases group (seq, flags, payload_len) as client-to-server steps over 1..3 batches."""
    at = _spread(rng, len(group), int(rng.integers(1, 4))) if len(group) > 1 else [0]
    return [(int(b), 0, (fl | ACK) if fl else PSH | ACK, seq, rng.bytes(plen)) for b, (seq, fl, plen) in zip(at, group)]


def _chaos(rng, script):
    """A tcptrack_cases.gen_connections script (flags, from_server) with consistent numbers."""
    st = _Stream(rng)
    at = _spread(rng, len(script), int(rng.integers(1, 4))) if len(script) > 1 else [0]
    return [(int(b), *st.step(fl, srv)) for b, (fl, srv) in zip(at, script)]


class Schedule:
    """`nbatches` batches with `rate` connections started in each of the first nbatches - 8.
    `interval`: batches between two expiries (a tuple that comes back after its record has been
    expired waits for that long)."""

    def __init__(self, seed, interval, rate, nbatches=60, noise=0.12):
        self.seed, self.interval, self.rate, self.nbatches = seed, interval, rate, nbatches
        rng = np.random.default_rng(seed)
        groups = iter(gen_groups(seed + 1, nbatches * rate, max_segments=10))
        chaos = iter(gen_connections(seed + 2, nbatches * rate, max_len=12))
        self.scripts, j = [], 0
        last_start = nbatches - 9
        for b in range(last_start + 1):
            for _ in range(rate):
                kind = KINDS[rng.choice(len(KINDS), p=WEIGHTS)]
                if kind == "oneway":
                    steps = _oneway(rng, next(groups))
                elif kind == "chaos":
                    steps = _chaos(rng, next(chaos))
                elif kind.startswith("return"):
                    steps = _life(rng, "full")
                    gap = int(rng.integers(1, 3)) if kind == "return_live" else IDLE + interval + 1
                    again = b + steps[-1][0] + gap
                    if again <= last_start:
                        self.scripts.append(Script("full", j, b, steps))
                        b2, steps = again, _life(rng, "full")
                        self.scripts.append(Script(kind, j, b2, steps))
                        j += 1
                        continue
                    kind = "full"
                else:
                    steps = _life(rng, kind)
                self.scripts.append(Script(kind, j, b, steps))
                j += 1
        self.nconn = j
        self.batches = self._batches(noise)

    def kinds(self):
        out = {k: 0 for k in KINDS}
        for s in self.scripts:
            out[s.kind] += 1
        return out

    def _batches(self, noise):
        per_batch = [[[] for _ in range(self.nconn)] for _ in range(self.nbatches)]
        for s in self.scripts:  # (a tuple's second script starts behind its first: the order holds)
            for (b, srv, fl, seq, pay) in s.steps:
                per_batch[s.start + b][s.j].append((srv, fl, seq, pay))
        out, base = [], 0
        for b, conns in enumerate(per_batch):
            pk = interleaved([[(fl, srv) for srv, fl, _, _ in c] for c in conns], self.seed * 1000 + b, noise=noise)
            at = [0] * self.nconn
            noise_frames = frames(pk.src, pk.dst, pk.sport, pk.dport, pk.flags, pk.kind) if len(pk) else None
            fr, keys, tuples, tcp, flags, seqs, pays = [], [], [], [], [], [], []
            for i in range(len(pk)):
                tup = (pk.src[i], pk.dst[i], pk.sport[i], pk.dport[i])
                if pk.kind[i] != TCP:
                    fr.append(bytes(noise_frames.packet(i)))
                    keys.append(ER.key_of(*tup, tp=5) if pk.kind[i] == UDP else None)
                    seq, pay = 0, b""
                else:
                    j = (tup[1] if tup[0] >> 24 == 0xC0 else tup[0]) - 0x0A000000
                    srv, fl, seq, pay = conns[j][at[j]]
                    at[j] += 1
                    assert fl == pk.flags[i] and (srv == 1) == (tup[0] >> 24 == 0xC0) and endpoints(j)[srv][0] == tup[0]
                    fr.append(synth.tcp_frame(int(tup[0]).to_bytes(4, "big"), int(tup[1]).to_bytes(4, "big"), tup[2],
                                              tup[3], seq, ack=1, flags=fl, payload=pay, pad_to=60))
                    keys.append(ER.key_of(*tup))
                tuples.append(tup)
                tcp.append(pk.kind[i] == TCP)
                flags.append(pk.flags[i])
                seqs.append(seq)
                pays.append(pay)
            stamps = b * SECOND + np.arange(len(fr), dtype=np.int64)
            out.append(Batch(fr, keys, tuples, tcp, flags, seqs, pays, stamps, base))
            base += len(fr)
        return out

    def expiry_after(self, b):
        """None, or (FlushOlderThan's T, Expire's cutoff) of the expiry that follows batch b."""
        if (b + 1) % self.interval or b + 1 < FLUSH_AGE:
            return None
        return (b + 1 - FLUSH_AGE) * SECOND, self.batches[b + 1 - IDLE].base


# the schedules of the GPU test: (seed, interval) -> Schedule arguments, chosen for a table of
# CAPACITY records (tests/test_sustained.py holds them to the conditions)
CAPACITY = 512
SCHEDULES = {(11, 1): dict(rate=22), (12, 1): dict(rate=22), (11, 4): dict(rate=16), (12, 4): dict(rate=16)}
_made = {}


def schedule(seed, interval):
    if (seed, interval) not in _made:
        _made[(seed, interval)] = Schedule(seed, interval, **SCHEDULES[(seed, interval)])
    return _made[(seed, interval)]


Step = namedtuple("Step", "keys verdict creator rows")
Row = namedtuple("Row", "nrec ncalls nbytes completed open next_seq pages")


def _rows(streams):
    return {s[0]: Row(s[2], s[3], s[5], s[6], s[7], s[8], s[9]) for s in streams}


class Truth:
    """The reference's pools for the capture, everything by tuple (the 40-byte key)."""

    def __init__(self, max_pages=0, sme=False):
        self.pool = ER.Pool()
        self.tracker = TR.Model(sme, reverse=ER.reverse_key)
        self.asm = AR.Model(None, max_pages)
        self.serial, self.key_of_serial = {}, []  # a pool record's number: what the tracker's model calls a flow id
        self.new_keys = []                        # the keys whose records the last batch created, in packet order
        self.peak = self.inserted = 0
        self.distinct = set()

    # ---- a batch
    def batch(self, B: Batch) -> Step:
        batch = PacketBatch.from_packets(B.frames)
        res = O.decode(batch, L.LayerTypeEthernet, MASK, ext=True)
        before = set(self.pool.flows)
        per = self.pool.insert(batch, res, B.base)
        assert per == B.keys, "the generator's keys are the oracle's"
        self.new_keys = []
        for k in per:
            if k is not None and k not in before:
                before.add(k)
                self.new_keys.append(k)
        self._created(self.new_keys)
        self.inserted += len(self.new_keys)
        self.distinct.update(self.new_keys)
        self.peak = max(self.peak, len(self.pool))
        tcp = [k if k is not None and t else None for k, t in zip(per, B.tcp)]
        verdict, creator = self._track(tcp, B.flags)
        segs = TS.segments(batch, res)
        work = {}
        for r in segs:
            work.setdefault(per[int(r["packet"])], []).append(r)
        return Step(per, verdict, creator, self._assemble(list(work.items()), batch.packet, B.stamps))

    def _created(self, keys):
        for k in keys:
            self.serial[k] = len(self.key_of_serial)
            self.key_of_serial.append(k)

    def _track(self, tcp, flags):
        verdict, conn, _ = self.tracker.track(tcp, flags, [self.serial[k] if k is not None else 0 for k in tcp])
        return verdict, [None if c == TR.FLOW_NONE else self.key_of_serial[int(c)] for c in conn]

    def _assemble(self, work, packet=None, ts=None, **flush):
        return _rows(self.asm.drive(work, packet, ts, **flush)[2])

    # ---- an expiry
    def flush(self, T):
        """FlushOlderThan(T): the stream rows of the keys it touched."""
        return self._assemble([], T=T, close_all=True)

    def flush_all(self):
        return self._assemble([], flush_all=True)

    def held(self):
        """The keys the assembler holds: open connections (only they have pages)."""
        return self.asm.open_keys()

    def expire(self, cutoff, pairs=True):
        gone = self.pool.expire(cutoff, self.held(), pairs)
        self._left(gone)
        return gone

    def remove(self, keys):
        """StreamPool.remove for `keys`."""
        self.pool.remove(keys)
        self._left(set(keys))

    def _left(self, gone):
        self.tracker.drop(gone, self.pool.flows)
        for k in gone:
            del self.serial[k]

    # ---- what the device must show
    def states(self):
        """{a connection's creating key: its carried byte}."""
        return {k: c.fsm.carried() for k, c in self.tracker.conns.items()}

    def conns(self):
        """{an open connection's key: (next_seq, flags, pages, page_bytes, last_seen_ns)}."""
        return {k: self.asm.info(k) for k in self.asm.open_keys()}

    def stats(self):
        c = list(self.conns().values())
        return {"connections": len(c), "connections_with_pages": sum(1 for x in c if x[2]),
                "pages": sum(x[2] for x in c), "page_bytes": sum(x[3] for x in c)}

    def order(self, k):
        """The key's "new" / "call" / "complete" over the run, and its call lists."""
        ev = self.asm.keys.get(k)
        return ([], []) if ev is None else (AR.order_of(ev), AR.call_lists(ev))

    def stream_keys(self):
        return list(self.asm.keys)


class IdKeyed(Truth):
    """The same composition with the consumers' state in slots by record id, the lowest free id
    going to each new key: what the device is.  forget=False leaves the tracker's reset out,
    hold=False the assembler's hold: the two mistakes the truth must be able to show."""

    def __init__(self, capacity, max_pages=0, sme=False, forget=True, hold=True):
        super().__init__(max_pages, sme)
        self.sme, self.forget, self.hold = sme, forget, hold
        self.free, self.id_of, self.owner = list(range(capacity)), {}, {}
        self.fsm = {}                       # id -> TCPSimpleFSM
        self.slots = AR.Model(capacity, max_pages)
        self.log, self.cursor = {}, {}      # key -> what its ids' streams were told; id -> entries seen

    def _created(self, keys):
        for k in keys:
            self.free.sort()
            self.id_of[k] = self.free.pop(0)
            self.owner[self.id_of[k]] = k

    def _track(self, tcp, flags):
        verdict, creator = np.full(len(tcp), TR.UNTRACKED, np.uint8), [None] * len(tcp)
        for i, k in enumerate(tcp):
            if k is None:
                continue
            rk, c = ER.reverse_key(k), k
            if rk in self.pool.flows and self.pool.flows[rk]["first"] < self.pool.flows[k]["first"]:
                c = rk
            fsm = self.fsm.setdefault(self.id_of[c], TR.TCPSimpleFSM(self.sme))
            f, d = int(flags[i]), c != k
            ok = fsm.CheckState(bool(f & SYN), bool(f & ACK), bool(f & FIN), bool(f & RST), d)
            verdict[i] = int(ok) | (2 if d else 0) | (fsm.state << 2) | (0x20 if fsm.dir else 0)
            creator[i] = c
        return verdict, creator

    def _assemble(self, work, packet=None, ts=None, **flush):
        streams = self.slots.drive([(self.id_of[k], rs) for k, rs in work], packet, ts, **flush)[2]
        for i, ev in self.slots.keys.items():
            self.log.setdefault(self.owner[i], []).extend(ev.order[self.cursor.get(i, 0):])
            self.cursor[i] = len(ev.order)
        return {self.owner[s[0]]: Row(s[2], s[3], s[5], s[6], s[7], s[8], s[9]) for s in streams}

    def held(self):
        return [self.owner[i] for i in self.slots.open_keys()] if self.hold else []

    def _left(self, gone):
        for k in gone:
            i = self.id_of.pop(k)
            self.free.append(i)
            if self.forget:
                self.fsm.pop(i, None)

    def order(self, k):
        o = self.log.get(k, [])
        return [x if isinstance(x, str) else "call" for x in o], [x[1] for x in o if isinstance(x, tuple)]

    def stream_keys(self):
        return list(self.log)


def run(model, sched, on_batch=None, on_expiry=None):
    """The schedule through `model`: every batch, FlushOlderThan and Expire after the batches the
    schedule says, FlushAll and a last Expire at the end.  Returns the verdict bytes of all
    packets."""
    verdicts = []
    for b, B in enumerate(sched.batches):
        st = model.batch(B)
        verdicts.append(st.verdict)
        if on_batch:
            on_batch(b, B, st)
        when = sched.expiry_after(b)
        if when is not None:
            rows = model.flush(when[0])
            held = set(model.held())
            idle = {k for k, f in model.pool.flows.items() if f["last"] < when[1]}
            gone = model.expire(when[1])
            if on_expiry:
                on_expiry(b, rows, held, gone, idle)
    model.flush_all()
    model.expire(1 << 62)
    return np.concatenate(verdicts)
