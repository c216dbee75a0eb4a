/*
 * gpd_flow_expire.h — C-ABI of flow expiry: records leave the flow table (gpd_flow.h) and their
 * slots are used again, so a capture can run without gpd_flow_reset.
 *
 * The reference's pools shrink: StreamPool.remove drops a connection when it closes
 * (tcpassembly/assembly.go:659-676; reassembly/memory.go:123-130), and Assembler.FlushOlderThan /
 * FlushCloseOlderThan (tcpassembly/assembly.go:269-271; reassembly/tcpassembly.go:1288-1291)
 * close the connections that have been idle since a given time.  Here the table is open
 * addressing in HBM, so a removed record becomes a tombstone that probes walk past, later inserts
 * claim tombstones before empty slots, and a sweep after every removal turns each run of
 * tombstones that ends at an empty slot back into empty slots.
 *
 * Reference interfaces each entry point replaces (paths relative to google/gopacket):
 *   gpd_flow_remove   StreamPool.remove(conn)             tcpassembly/assembly.go:659-676;
 *                                                         reassembly/memory.go:123-130
 *   gpd_flow_expire   Assembler.FlushOlderThan(t) and FlushCloseOlderThan(t), the part that takes
 *                     idle connections out of the pool (conn.lastSeen.Before(t))
 *                                                         tcpassembly/assembly.go:235-271;
 *                                                         reassembly/tcpassembly.go:1260-1291
 *   gpd_flow_load     len(StreamPool.conns) beside the table's own bookkeeping
 *                                                         tcpassembly/assembly.go:311
 *
 * A record's id is its slot, and every stateful consumer (gpd_tcp_assembler, gpd_tcp_tracker)
 * indexes its state by it.  A removed id is handed to the next new key that probes to it, so the
 * caller returns the consumers' state for the removed ids to the fresh state in the same step:
 * gpd_tcp_tracker_forget(ids), and for the assembler a `hold` mask that keeps every record whose
 * connection is open or holds pages (a closed connection's info is all zero already).
 *
 * Time is the packet sequence number: a record's `last` is the highest index_base + i of its
 * packets, and the caller maps a time to a sequence number through its batches' index_base.
 *
 * These entry points came after ABI version 10 and do not change it (GPD_ABI_VERSION stays 10).
 * Like every call on a table, they are ordered with its inserts on one stream.
 */
#ifndef GPD_FLOW_EXPIRE_H_
#define GPD_FLOW_EXPIRE_H_
#include "gpd_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gpd_flow_expire flags */
#define GPD_FLOW_EXPIRE_PAIRS 0x1u  /* a record leaves only together with its reversed key's record */

/* StreamPool.remove for the records ids[0, m) (a device array).  Ids at or above the capacity,
 * ids of empty or removed slots and duplicates are ignored, so the call is idempotent.
 * gpd_flow_stats.flows goes down by the records removed.  Asynchronous on `stream`. */
int gpd_flow_remove(gpd_flowtable *ft, const uint32_t *ids, uint64_t m, void *stream);

/* Removes every occupied record with last < last_below: the comparison is strict, as
 * time.Before is, and last_below == 0 removes nothing.  A record is kept if hold != NULL and
 * hold[id] != 0 (`hold`: one device byte per record of the table, capacity bytes).  With
 * GPD_FLOW_EXPIRE_PAIRS a record is removed only if the record of its reversed key qualifies as
 * well (idle and not held); a record whose reverse is not in the table, or whose key is its own
 * reverse, counts as a complete pair: both halves of a `reassembly` connection
 * (reassembly/memory.go:169-206) leave together or not at all.
 * ids[] (device, max_ids entries) receives the removed ids in ascending order and *count (host)
 * how many there are.  ids == NULL with max_ids == 0 is the sizing call: *count is set and nothing
 * changes.  A count above max_ids removes nothing, sets *count and returns GPD_ERR_INVALID.
 * Synchronises `stream`. */
int gpd_flow_expire(gpd_flowtable *ft, uint64_t last_below, const uint8_t *hold, uint32_t flags,
                    uint32_t *ids, uint64_t max_ids, uint64_t *count, void *stream);

/* out[0] = records in use, out[1] = tombstones (removed slots no sweep could turn empty yet),
 * counted over the table.  Synchronises `stream`. */
int gpd_flow_load(gpd_flowtable *ft, uint64_t out[2], void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_FLOW_EXPIRE_H_ */
