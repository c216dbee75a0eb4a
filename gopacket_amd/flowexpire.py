"""Flow expiry: idle flow records leave the flow table and their slots are used again.

The reference's pools shrink: StreamPool.remove drops a connection when it closes
(tcpassembly/assembly.go:659-676, reassembly/memory.go:123-130), and FlushOlderThan /
FlushCloseOlderThan close the idle ones.  `Remove` and `Expire` do that for a `FlowTable`
(include/gpd_flow_expire.h): a removed record becomes a tombstone that probes walk past, later
inserts claim tombstones before empty slots, and a sweep turns every run of tombstones that ends at
an empty slot back into empty slots.  Time is the packet sequence number (`index_base` + i).

A sustained capture, once per interval, with `a` an `Assembler` and `tracker` a `ConnTracker` over
`table`, and `cutoff` the index_base of the oldest batch still young:

    ids, n = Expire(table, cutoff, hold=assembler_hold(a), pairs=True)
    tracker.forget(ids[:n])

A record id is handed to the next new key that probes to it, so the consumers' state for the removed
ids is returned to the fresh state in the same step: the tracker by `forget`; the assembler needs
nothing, because `assembler_hold` keeps every record whose connection is open or holds pages, and a
closed connection's state is all zero already.

The entry points are bound onto the loaded library here, on first use, from FLOWEXPIRE_EXPORTS.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

EXPIRE_PAIRS = 0x1

FLOWEXPIRE_EXPORTS = {
    # include/gpd_flow_expire.h — name: (restype, argtypes)
    "gpd_flow_remove": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "gpd_flow_expire": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                  C.POINTER(C.c_uint64), C.c_void_p]),
    "gpd_flow_load": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
}

_bound = False


def flowexpire_lib():
    """The loaded library with the expiry signatures bound (once)."""
    global _bound
    if not _bound:
        for name, (res, args) in FLOWEXPIRE_EXPORTS.items():
            fn = getattr(_lib.lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return _lib.lib


def _device(table):
    from .parser import _torch
    return _torch().device("cuda", table.parser.device)


def Remove(table, ids, stream=None) -> None:
    """StreamPool.remove for the records `ids` (a 32-bit device tensor or an array of ids).  Ids
    at or above the capacity, ids of empty slots and duplicates are ignored."""
    from .parser import _torch
    torch = _torch()
    if isinstance(ids, torch.Tensor):
        if ids.element_size() != 4:
            raise ValueError("Remove: ids must be 32-bit")
        t = ids.contiguous().to(_device(table))
    else:
        a = np.ascontiguousarray(np.asarray(ids, np.uint32))
        t = torch.from_numpy(a.view(np.int32)).to(_device(table))
    if t.numel() == 0:
        return
    check(flowexpire_lib().gpd_flow_remove(table.h, C.c_void_p(t.data_ptr()), t.numel(), table._stream(stream)),
          "gpd_flow_remove")
    (stream if stream is not None else torch.cuda.current_stream(table.parser.device)).synchronize()  # (t may go)


def expire_raw(table, older_than_seq: int, hold, flags: int, ids, max_ids: int, stream=None):
    """gpd_flow_expire as it is: (rc, count)."""
    count = C.c_uint64()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = flowexpire_lib().gpd_flow_expire(table.h, int(older_than_seq), p(hold), int(flags), p(ids), int(max_ids),
                                          C.byref(count), table._stream(stream))
    return rc, int(count.value)


def Expire(table, older_than_seq: int, hold=None, pairs: bool = False, stream=None):
    """Removes every record whose last packet's sequence number is below `older_than_seq`
    (strictly, as time.Before; 0 removes nothing), except those with hold[id] != 0 (`hold`: a
    uint8 device tensor, one byte per record of the table).  With `pairs` a record leaves only
    together with the record of its reversed key.  Returns (int32 device tensor of the removed
    ids, ascending, the u32 bit patterns; their count).  Synchronises `stream`."""
    from .parser import _torch
    torch = _torch()
    cap = table.Stats(stream)["capacity"]
    if hold is not None:
        if hold.element_size() != 1 or hold.numel() < cap:
            raise ValueError("Expire: hold must hold one byte per record of the table")
        hold = hold.contiguous()
    ids = torch.empty(cap, dtype=torch.int32, device=_device(table))
    rc, count = expire_raw(table, older_than_seq, hold, EXPIRE_PAIRS if pairs else 0, ids, cap, stream)
    check(rc, "gpd_flow_expire")
    return ids[:count], count


def Load(table, stream=None):
    """(records in use, tombstones): the second counts removed slots that no sweep could turn
    empty yet, because a record sits behind them on its probe chain."""
    out = (C.c_uint64 * 2)()
    check(flowexpire_lib().gpd_flow_load(table.h, out, table._stream(stream)), "gpd_flow_load")
    return int(out[0]), int(out[1])


def assembler_hold(assembler, stream=None):
    """The `hold` mask of an `Assembler` (tcpasm.py): a uint8 device tensor, non-zero where the
    connection is open or holds pages.  (An assembler's id_bound is its table's capacity.)"""
    from .parser import _torch
    torch = _torch()
    c = assembler.conns(stream)
    t = torch.from_numpy(np.ascontiguousarray(c["flags"]).view(np.int32)).to(torch.device("cuda", assembler.device))
    pages = torch.from_numpy(np.ascontiguousarray(c["pages"]).view(np.int32)).to(t.device)
    return ((t != 0) | (pages != 0)).to(torch.uint8)
