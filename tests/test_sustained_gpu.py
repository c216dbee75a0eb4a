"""A long capture through one flow table, one ConnTracker and one Assembler with expiry between
the batches (gopacket_amd/flowexpire.py's recipe, verbatim), against a truth that is keyed by the
connection's tuple and never sees a record id (tests/sustained_cases.py).  Record ids change hands
between tuples more than three times the table's capacity in every case; tests/test_sustained.py
holds the schedules to the conditions that make that so.

Device ids depend on timing where keys race for tombstones, so no id is compared with a model:
the test keeps the id -> key map of the batches it has seen, as tests/test_flow_expire_gpu.py's
Rig does, and compares everything else through it."""
import time

import numpy as np
import pytest

import flow_expire_ref as ER
import sustained_cases as SC
from gopacket_amd import layers as L
from gopacket_amd.batch import PacketBatch

pytestmark = pytest.mark.gpu

CAP = SC.CAPACITY
NONE = 0xFFFFFFFF
POISON = 0xA5


@pytest.fixture(scope="module")
def parser():
    from gopacket_amd import parser as P
    p = P.NewDecodingLayerParser(L.LayerTypeEthernet)
    p._mask = SC.MASK
    return p


class Streams:
    """The StreamFactory of the run: what every tuple's streams were told, in order.  New gets a
    flow id; the tuple is the one that holds the id at that moment."""

    def __init__(self, owner):
        self.owner, self.order = owner, {}

    def New(self, fid):
        log = self.order.setdefault(self.owner[int(fid)], [])
        log.append("new")

        class Stream:
            def Reassembled(self, rs):
                log.append(("call", [(bytes(r.Bytes), r.Skip, r.Start, r.End, r.Seen) for r in rs]))

            def ReassemblyComplete(self):
                log.append("complete")
        return Stream()

    def of(self, k):
        o = self.order.get(k, [])
        return [x if isinstance(x, str) else "call" for x in o], [x[1] for x in o if isinstance(x, tuple)]


class Sustained:
    """The three device objects beside the truth."""

    def __init__(self, parser, max_pages, sme):
        from gopacket_amd import tcpasm, tcptrack
        from gopacket_amd.flows import NewFlowTable
        self.parser = parser
        self.table = NewFlowTable(parser, CAP)
        assert self.table.Stats()["capacity"] == CAP
        self.tracker = tcptrack.NewConnTracker(parser, self.table, support_missing_establishment=sme)
        self.asm = tcpasm.NewAssembler(parser, self.table, max_pages_per_connection=max_pages)
        self.truth = SC.Truth(max_pages, sme)
        self.id_of, self.owner, self.last_holder, self.handovers = {}, {}, {}, 0
        self.log = Streams(self.owner)
        self.pool = {}  # deliver's streams by flow id

    def close(self):
        self.asm.close()
        self.tracker.close()

    # ---- the assembler's run with poisoned buffers: AssembleBatch's steps (tcpasm.py) on run_raw
    def assemble(self, db, dsegs, dgroups, count, ngroups, ts):
        import torch
        from gopacket_amd import tcpasm as M
        open_before = self.asm.open_ids()
        head = (db, dsegs, count, dgroups, ngroups, ts, 0, (0, False, False))
        rc, out = self.asm.run_raw(*head, None, 0, None, None, 0, None, 0)
        assert rc == 0
        nr, ns, nb = out[:3]
        full = lambda n, dt=torch.uint8: torch.full((n,), POISON if dt == torch.uint8 else -1, dtype=dt, device="cuda")
        recs, seen = full((nr + 1) * M.REASM_DTYPE.itemsize), full(nr + 1, torch.int64)
        streams, byts = full((ns + 1) * M.STREAM_DTYPE.itemsize), full(nb + 64)
        rc, out2 = self.asm.run_raw(*head, recs, nr, seen, streams, ns, byts, nb)
        assert rc == 0 and out2 == out
        assert bool((recs[nr * 32:] == POISON).all()) and bool((streams[ns * 48:] == POISON).all())
        assert bool((byts[nb:] == POISON).all()) and int(seen[nr]) == -1, "nothing behind the counted records"
        return M.AsmResult(recs[:nr * 32], seen[:nr], streams[:ns * 48], byts[:nb], *out[:7], open_before)

    # ---- a batch
    def batch(self, B):
        import torch
        from gopacket_amd import parser as P
        from gopacket_amd import tcpassembly as T
        batch = PacketBatch.from_packets(B.frames)
        db, dr = P.DeviceBatch(batch, 0), P.DeviceResult(batch.n, 0)
        self.parser.decode_device(db, dr)
        ids_t = torch.full((batch.n,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")  # 0xA5 in every byte
        ids_t = self.table.Insert(db, dr, flow_id=ids_t, index_base=B.base)
        r = self.tracker.TrackBatch(db, dr, ids_t, want_conn_id=True)
        dsegs, dgroups, count, ngroups, ungrouped = T.TCPSegments(self.parser, db, dr, flow_id=ids_t, table=self.table)
        assert ungrouped == 0
        res = self.assemble(db, dsegs, dgroups, count, ngroups, torch.from_numpy(B.stamps).cuda())
        st = self.truth.batch(B)
        ids = ids_t.cpu().numpy().view(np.uint32)
        # the id -> key map: a live key keeps its id; a new record's id may have been another tuple's
        for i, k in enumerate(st.keys):
            if k is None:
                assert ids[i] == NONE, (i, hex(ids[i]))
                continue
            assert ids[i] < CAP, (i, hex(ids[i]))
            if self.id_of.setdefault(k, int(ids[i])) != int(ids[i]):
                raise AssertionError(("a live key keeps its id", i, self.id_of[k], int(ids[i])))
        for k in self.truth.new_keys:
            i = self.id_of[k]
            self.handovers += self.last_holder.get(i, k) != k
            self.last_holder[i] = self.owner[i] = k
        self.check_table()
        # the tracker
        verdict = r.verdict.cpu().numpy()
        if not np.array_equal(verdict, st.verdict):
            i = int(np.nonzero(verdict != st.verdict)[0][0])
            raise AssertionError(("verdict", i, hex(verdict[i]), hex(st.verdict[i]), B.tuples[i], hex(B.flags[i])))
        want_conn = np.array([NONE if c is None else self.id_of[c] for c in st.creator], np.uint32)
        got_conn = r.conn_id.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_conn, want_conn), "conn_id: the record of the connection's creating direction"
        return self.streams(res, st.rows)

    def streams(self, res, rows):
        """A run's stream records against the truth's rows, by tuple; the calls go to the log.
        Returns the device's {key: Row}."""
        from gopacket_amd import tcpasm as M
        h = M.to_host(res)
        fields = ("nrec", "ncalls", "nbytes", "completed", "open", "next_seq", "reserved")  # (reserved: the pages)
        got = {self.owner[int(s["flow_id"])]: SC.Row(*(int(s[f]) for f in fields)) for s in h.streams}
        assert len(got) == len(h.streams)
        if got != rows:
            bad = [k for k in set(got) | set(rows) if got.get(k) != rows.get(k)][0]
            raise AssertionError(("stream", bad.hex(), got.get(bad), rows.get(bad)))
        M.deliver(h, self.log, self.pool)
        return got

    def check_table(self):
        from gopacket_amd import flowexpire as FE
        pool = self.truth.pool
        recs, idx = self.table.Export()
        assert ER.same_as_export(pool, recs)
        assert {ER.flow_ref.record_key(r): int(ix) for r, ix in zip(recs, idx)} == self.id_of
        assert len(set(self.id_of.values())) == len(self.id_of), "distinct live keys, distinct ids"
        st = self.table.Stats()
        assert (st["flows"], st["full"], st["collisions"]) == (len(pool), 0, 0)
        used, tombs = FE.Load(self.table)
        assert used == len(pool) and used + tombs <= CAP

    # ---- an expiry
    def left(self, got_ids, gone):
        assert list(got_ids) == sorted(self.id_of[k] for k in gone), "the removed ids are the truth's keys', ascending"
        for k in gone:
            del self.id_of[k]
        self.check_table()
        self.check_state()

    def expire(self, T, cutoff):
        from gopacket_amd import flowexpire as FE
        rows = self.truth.flush(T)
        self.streams(self.asm.FlushOlderThan(T), rows)
        ids, n = FE.Expire(self.table, cutoff, hold=FE.assembler_hold(self.asm), pairs=True)
        self.tracker.forget(ids[:n])
        gone = self.truth.expire(cutoff)
        assert n == len(gone)
        self.left(ids.cpu().numpy().view(np.uint32), gone)

    def remove(self, keys):
        from gopacket_amd import flowexpire as FE
        ids = np.array(sorted(self.id_of[k] for k in keys), np.uint32)
        FE.Remove(self.table, ids)
        self.tracker.forget(ids)
        self.truth.remove(keys)
        self.left(ids, keys)

    def check_state(self):
        from gopacket_amd import tcpasm as M
        want = np.zeros(CAP, np.uint8)
        for k, byte in self.truth.states().items():
            want[self.id_of[k]] = byte
        got = self.tracker.states()
        if not np.array_equal(got, want):
            i = int(np.nonzero(got != want)[0][0])
            raise AssertionError(("tracker state", i, got[i], want[i], i in self.owner and self.owner[i].hex()))
        conns = np.zeros(CAP, M.CONN_INFO_DTYPE)
        for k, info in self.truth.conns().items():
            conns[self.id_of[k]] = info
        have = self.asm.conns()
        if have.tobytes() != conns.tobytes():
            i = int(np.nonzero(have != conns)[0][0])
            raise AssertionError(("assembler state", i, have[i], conns[i]))
        assert self.asm.stats() == self.truth.stats()

    # ---- the end
    def finish(self):
        from gopacket_amd import flowexpire as FE
        self.streams(self.asm.FlushAll(), self.truth.flush_all())
        ids, n = FE.Expire(self.table, 1 << 62, hold=FE.assembler_hold(self.asm), pairs=True)
        self.tracker.forget(ids[:n])
        gone = self.truth.expire(1 << 62)
        self.left(ids.cpu().numpy().view(np.uint32), gone)
        assert FE.Load(self.table) == (0, 0) and not self.id_of and len(self.truth.pool) == 0
        assert not self.tracker.states().any() and not self.asm.conns().view(np.uint8).any()
        assert self.asm.stats()["connections"] == 0 and len(self.asm.open_ids()) == 0
        keys = set(self.truth.stream_keys()) | set(self.log.order)
        for k in keys:  # per directional tuple: new / Reassembled / ReassemblyComplete in order, every call's records
            got, want = self.log.of(k), self.truth.order(k)
            assert got[0] == want[0], ("order", k.hex(), got[0], want[0])
            if got[1] != want[1]:
                c = next(i for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b)
                raise AssertionError(("call", k.hex(), c, [x[1:] for x in got[1][c]], [x[1:] for x in want[1][c]]))
        assert len(keys) > CAP
        assert self.handovers >= 3 * CAP, self.handovers


def sustained(parser, seed, interval, max_pages, sme, removing=False):
    t0 = time.perf_counter()
    sched = SC.schedule(seed, interval)
    s = Sustained(parser, max_pages, sme)
    removed = 0
    for b, B in enumerate(sched.batches):
        got = s.batch(B)
        if removing:  # the pairs whose two halves both completed in this batch leave at once
            done = {k for k, r in got.items() if r.completed and not r.open}
            pair = sorted(k for k in done if ER.reverse_key(k) in done)
            if pair:
                s.remove(pair)
                removed += len(pair)
        when = sched.expiry_after(b)
        if when is not None:
            s.expire(*when)
    s.finish()
    s.close()
    print(f"sustained seed {seed} interval {interval} max_pages {max_pages} sme {sme} removing {removing}: peak live "
          f"{s.truth.peak}, distinct keys {len(s.truth.distinct)}, id hand-overs {s.handovers}, removed by Remove "
          f"{removed}, {time.perf_counter() - t0:.1f} s")
    return s, removed


@pytest.mark.parametrize("interval", [1, 4])
@pytest.mark.parametrize("sme", [False, True], ids=["strict", "missing_establishment"])
@pytest.mark.parametrize("max_pages", [0, 4])
@pytest.mark.parametrize("seed", [11, 12])
def test_sustained_capture_with_expiry(parser, seed, max_pages, sme, interval):
    """Decode, Insert, TrackBatch, TCPSegments, AssembleBatch per batch; every `interval` batches
    FlushOlderThan, Expire(hold=assembler_hold, pairs) and forget.  After every batch the table
    equals the pool, verdicts, connection ids and stream records equal the truth's; after every
    expiry the removed ids, the tracker's and the assembler's state by id; at the end everything
    is empty and every tuple's streams were told what the truth's were."""
    sustained(parser, seed, interval, max_pages, sme)


def test_sustained_capture_with_remove(parser):
    """The same capture with StreamPool.remove's path: after each batch the pairs whose two
    halves both completed in it are taken out with Remove and forgotten, before the idle test
    could find them.  What never completes as a pair (one-way connections, UDP flows, abandoned
    and half-closed connections) still leaves by Expire, or the table would fill."""
    s, removed = sustained(parser, 11, 4, 0, False, removing=True)
    assert removed >= CAP // 4
