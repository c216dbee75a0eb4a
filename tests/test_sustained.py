"""The schedules of tests/test_sustained_gpu.py held to their conditions on the CPU, from the
models alone (tests/sustained_cases.py), so that the GPU test cannot pass by testing nothing: the
table is never full but always crowded, ids change hands at least three times the capacity, every
kind of connection occurs, a held half keeps an idle pair, and the truth differs from a
composition that keeps the consumers' state by id when the tracker's reset or the assembler's hold
is left out."""
import numpy as np
import pytest

import flow_expire_ref as ER
import sustained_cases as SC
import tcptrack_ref as TR
from tcptrack_cases import endpoints

CAP = SC.CAPACITY
SCHEDS = sorted(SC.SCHEDULES)
_runs = {}


def truth_run(seed, interval, max_pages):
    """The truth over a schedule, once: the model, its verdicts and what the expiries saw."""
    key = (seed, interval, max_pages)
    if key in _runs:
        return _runs[key]
    sched, T = SC.schedule(seed, interval), SC.Truth(max_pages, False)
    seen = dict(live=[], new={}, half_held=0, closed_by_flush={}, flushed_then_expired=0)

    def on_batch(b, B, st):
        seen["live"].append(len(T.pool))
        seen["new"][b] = set(T.new_keys)

    def on_expiry(b, rows, held, gone, idle):
        for k in held & idle:
            rk = ER.reverse_key(k)
            if rk in idle and rk not in held:
                seen["half_held"] += 1
                assert k not in gone and rk not in gone, "a held half keeps its pair"
        for k, r in rows.items():
            if r.completed:
                seen["closed_by_flush"].setdefault(k, b)
        seen["flushed_then_expired"] += sum(1 for k in gone if seen["closed_by_flush"].pop(k, b) < b)

    verdicts = SC.run(T, sched, on_batch, on_expiry)
    _runs[key] = (sched, T, verdicts, seen)
    return _runs[key]


def client_key(j):
    c, s = endpoints(j)
    return ER.key_of(c[0], s[0], c[1], s[1])


@pytest.mark.parametrize("max_pages", [0, 4])
@pytest.mark.parametrize("seed,interval", SCHEDS)
def test_the_table_is_crowded_never_full_and_ids_change_hands(seed, interval, max_pages):
    sched, T, _, seen = truth_run(seed, interval, max_pages)
    assert 40 <= sched.nbatches <= 60 and 200 <= np.median([len(B.frames) for B in sched.batches]) <= 500
    assert T.peak == max(seen["live"]) and CAP // 2 <= T.peak <= CAP * 3 // 4, T.peak
    # every distinct key's first record sits on an id; at most CAP of them on an id nobody had before
    assert len(T.distinct) >= 4 * CAP and T.inserted >= len(T.distinct)
    assert seen["half_held"] >= 1 and seen["flushed_then_expired"] >= 1, seen
    assert len(T.pool) == 0 and not T.states() and not T.conns()
    # distinct stamps, batch * 10^9 + i, and index_base counting packets
    base = 0
    for b, B in enumerate(sched.batches):
        assert B.base == base and list(B.stamps) == [b * 10**9 + i for i in range(len(B.frames))]
        base += len(B.frames)


@pytest.mark.parametrize("seed,interval", SCHEDS)
def test_every_kind_of_connection_occurs(seed, interval):
    sched, T, _, seen = truth_run(seed, interval, 0)
    kinds = sched.kinds()
    assert set(kinds) == set(SC.KINDS) and all(n >= 8 for n in kinds.values()), kinds
    nokey = sum(1 for B in sched.batches for k in B.keys if k is None)
    udp = {k for B in sched.batches for k, t in zip(B.keys, B.tcp) if k is not None and not t}
    assert nokey >= 8 and len(udp) >= 8
    spans = {s.steps[-1][0] + 1 for s in sched.scripts if s.kind == "full"}
    assert spans >= {1, 2, 3, 4, 5, 6}
    got = {k: 0 for k in ("rst", "server_first", "oneway", "midstream", "displaced", "lost", "abandoned", "return_live",
                          "return_expired")}
    for s in sched.scripts:
        ck, sk = client_key(s.j), ER.reverse_key(client_key(s.j))
        order, calls = T.order(ck)
        flat = [r for c in calls for r in c]
        first_b, first_srv = s.steps[0][0], s.steps[0][1]
        if s.kind == "rst":
            got["rst"] += any(st[2] & TR.RST for st in s.steps)
        elif s.kind == "server_first":  # the server's record is the older one
            got["server_first"] += first_srv == 1 and sk in seen["new"][s.start + first_b]
        elif s.kind == "oneway":
            got["oneway"] += all(sk not in seen["new"][s.start + st[0]] for st in s.steps)
        elif s.kind == "midstream":
            got["midstream"] += not any(st[2] & TR.SYN for st in s.steps) and all(not r[2] for r in flat)
        elif s.kind == "displaced":  # everything the client sent comes out in order with no gap
            sent = [st for st in s.steps if not st[1] and len(st[4])]
            isn = next(st[3] for st in s.steps if not st[1] and st[2] & TR.SYN)
            sent.sort(key=lambda st: (st[3] - isn) & 0xFFFFFFFF)
            late = any(a[0] > b[0] for a, b in zip(sent, sent[1:]))
            whole = b"".join(r[0] for r in flat) == b"".join(st[4] for st in sent) and all(r[1] == 0 for r in flat)
            got["displaced"] += late and whole
        elif s.kind == "lost":      # the gap is closed by the flush, with Skip set
            got["lost"] += any(r[1] > 0 for r in flat)
        elif s.kind == "abandoned":  # no End, yet complete
            got["abandoned"] += order.count("complete") >= 1 and not any(r[3] for r in flat)
        elif s.kind == "return_live":
            got["return_live"] += ck not in seen["new"][s.start] and order.count("new") >= 2
        elif s.kind == "return_expired":
            got["return_expired"] += ck in seen["new"][s.start] and order.count("new") >= 2
    assert all(n >= 8 for n in got.values()), got


@pytest.mark.parametrize("seed,interval", SCHEDS)
def test_state_kept_by_id_without_the_reset_shows(seed, interval):
    """The consumers' state in slots by id, the lowest free id to each new key, and
    ConnTracker.forget left out: a verdict byte differs from the truth's.  With the reset and the
    hold in place the same composition equals the truth, packet for packet and call for call."""
    sched, T, verdicts, _ = truth_run(seed, interval, 0)
    good = SC.IdKeyed(CAP, 0, False)
    v_good = SC.run(good, sched)
    assert np.array_equal(v_good, verdicts)
    assert all(good.order(k) == T.order(k) for k in set(T.stream_keys()) | set(good.stream_keys()))
    bad = SC.IdKeyed(CAP, 0, False, forget=False)
    v_bad = SC.run(bad, sched)
    assert int((v_bad != verdicts).sum()) >= 1


@pytest.mark.parametrize("seed,interval", SCHEDS)
def test_state_kept_by_id_without_the_hold_shows(seed, interval):
    """The same with forget kept and the assembler's hold left out, so that open connections
    expire and their ids go to other tuples: a Reassembled call list differs."""
    sched, T, verdicts, _ = truth_run(seed, interval, 0)
    bad = SC.IdKeyed(CAP, 0, False, hold=False)
    SC.run(bad, sched)
    keys = set(T.stream_keys()) | set(bad.stream_keys())
    assert sum(1 for k in keys if T.order(k)[1] != bad.order(k)[1]) >= 1
