/*
 * gpd_tcptrack.h — C-ABI of TCP connection tracking: the part of the reference's `reassembly`
 * package that stands on its own, as a device object over a flow table.
 *
 * The flow table (include/gpd_flow.h) is directional: one record is one half-connection.
 * `reassembly` pairs the two halves (StreamPool.getHalf looks a key up, then its Reverse(), and
 * newConnection makes the creator the client-to-server half: reassembly/memory.go:169-206), gives
 * every packet a TCPFlowDirection, and offers TCPSimpleFSM (reassembly/tcpcheck.go:119-246), which
 * its users call from Stream.Accept to drop packets a real stack would reject.  The tracker does
 * the three for a decoded batch in HBM and keeps every connection's FSM on the device from batch
 * to batch.  The verdict is a byte per packet; its accept bit is a keep mask of the kind
 * gpd_bpf_filter produces, for gpd_batch_select and both writers.
 *
 * Semantics.  Tracked are the packets the flow table keys (a network and a transport endpoint,
 * both header offsets below 0xFFFF) whose transport endpoint type is TCPPort and whose flow id is
 * below the table's capacity.  There is no SYN/FIN/RST/payload filter: AssembleWithContext has
 * none (reassembly/tcpassembly.go:638-672) and the FSM needs bare ACKs (LastAck -> Closed).
 * For a tracked packet with flow id f:
 *   peer        r = the record holding the reversed key (addresses swapped, ports swapped, same
 *               types), found by a read-only probe of the table; it may be absent; r == f when
 *               the key is its own reverse.
 *   connection  c = whichever of f and r has the smaller `first` (f without r): the direction
 *               the reference's pool saw first.  The packet's direction is ClientToServer iff
 *               c == f.
 *   state       the connection's FSM starts as the zero value (TCPStateClosed, dir false) and is
 *               stepped by CheckState(tcp, dir) for the connection's packets in capture order,
 *               both directions interleaved.  SupportMissingEstablishment is a creation option.
 * Every other packet (no key, not TCP, GPD_FLOW_FULL, an id flagged GPD_FLOW_COLLISION,
 * GPD_FLOW_NONE) is untracked: verdict GPD_TCP_UNTRACKED, no state changes.
 *
 * Preconditions.  flow_id[] comes from gpd_flow_insert of this batch into the tracker's table,
 * finished on (or ordered before) `stream`; the inserts' index_base grows from call to call, so
 * that no record's `first` ever falls (`first` is the sequence number of the packet that created
 * the record) and a connection's direction, once fixed, stays.  (With fingerprints narrowed by
 * gpd_flow_test_fingerprint_bits a record's `first` also covers the flagged packets that landed
 * on it in the launch that created it, so two directions created in one such batch may be ordered
 * by a foreign packet.  A production table has no collisions.)
 *
 * Out of scope:
 *   - TCPOptionCheck.Accept (tcpcheck.go:47-106): it needs half.nextSeq, the assembler's;
 *   - AssembleWithContext itself (ordering, buffering, ScatterGather delivery);
 *   - expiry by time (FlushCloseOlderThan) is the flow table's: gpd_flow_expire (gpd_flow_expire.h)
 *     removes idle records, a connection's two halves together, and its ids go to _forget here;
 *     within the tracker connections leave through _forget and _reset only — TCPStateReset is
 *     terminal in the reference, too;
 *   - tables filled through gpd_flow_insert_keys (sharding): their `first` words are the senders'.
 *
 * Reference interfaces the entry points replace (paths relative to google/gopacket):
 *   gpd_tcp_tracker_create / _destroy  NewStreamPool (reassembly/memory.go:134-141) with
 *                                      NewTCPSimpleFSM(TCPSimpleFSMOptions) per connection
 *                                      (reassembly/tcpcheck.go:125-146)
 *   gpd_tcp_tracker_run                StreamPool.getHalf / getConnection / newConnection
 *                                      (reassembly/memory.go:169-206, 153-167), the direction of
 *                                      AssembleWithContext (reassembly/tcpassembly.go:644-667) and
 *                                      TCPSimpleFSM.CheckState (reassembly/tcpcheck.go:167-246)
 *   gpd_tcp_tracker_states             TCPSimpleFSM.String's state (reassembly/tcpcheck.go:148-164)
 *   gpd_tcp_tracker_forget             StreamPool.remove (reassembly/memory.go:123-130)
 *   gpd_tcp_tracker_reset              a new StreamPool
 */
#ifndef GPD_TCPTRACK_H_
#define GPD_TCPTRACK_H_
#include "gpd.h"
#include "gpd_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpd_tcp_tracker gpd_tcp_tracker;

/* reassembly/tcpcheck.go:131-138 */
#define GPD_TCP_STATE_CLOSED 0u
#define GPD_TCP_STATE_SYN_SENT 1u
#define GPD_TCP_STATE_ESTABLISHED 2u
#define GPD_TCP_STATE_CLOSE_WAIT 3u
#define GPD_TCP_STATE_LAST_ACK 4u
#define GPD_TCP_STATE_RESET 5u

/* The verdict byte of a tracked packet. */
#define GPD_TCP_V_ACCEPT 0x01u      /* CheckState returned true */
#define GPD_TCP_V_DIR 0x02u         /* 1 = TCPDirServerToClient */
#define GPD_TCP_V_STATE_SHIFT 2     /* bits 2..4: t.state after the packet */
#define GPD_TCP_V_STATE_MASK 0x1Cu
#define GPD_TCP_V_FSM_DIR 0x20u     /* t.dir after the packet */
#define GPD_TCP_UNTRACKED 0xFFu     /* the verdict of every other packet */

/* The carried byte of a flow record (gpd_tcp_tracker_states): zero is a fresh FSM. */
#define GPD_TCP_C_STATE_MASK 0x07u  /* t.state */
#define GPD_TCP_C_FSM_DIR 0x08u     /* t.dir */

/* TCPSimpleFSMOptions (reassembly/tcpcheck.go:125-128). */
typedef struct gpd_tcp_track_opts {
  uint32_t support_missing_establishment; /* SupportMissingEstablishment */
  uint32_t reserved;                      /* zero */
} gpd_tcp_track_opts;

/* The object: one FSM per record of `flowtable` (created for ctx's device).  opts NULL: the
 * zero options.  It owns its carry and scratch, serves one call at a time, and must be destroyed
 * before its table and its context. */
int gpd_tcp_tracker_create(gpd_ctx *ctx, gpd_flowtable *flowtable, const gpd_tcp_track_opts *opts,
                           gpd_tcp_tracker **t);
void gpd_tcp_tracker_destroy(gpd_tcp_tracker *t);

/* One batch.  `in` is the batch gpd_decode read, `res` its results on the device (status, or
 * records; hdr_off required), flow_id the u32[in->n] device array gpd_flow_insert filled for it.
 *   verdict[in->n]  device bytes, in packet order (required)
 *   conn_id[in->n]  NULL, or device u32: the packet's connection c, GPD_FLOW_NONE when untracked
 *   out[4]          host words: {tracked, accepted, rejected, connections that had a packet}
 * Limits (GPD_ERR_INVALID otherwise): in->n <= 2^32 - 256, as for gpd_tcp_segments.  An empty
 * batch is a no-op (out[] zero).  Synchronises `stream`. */
int gpd_tcp_tracker_run(gpd_tcp_tracker *t, const gpd_batch *in, const gpd_result *res,
                        const uint32_t *flow_id, uint8_t *verdict, uint32_t *conn_id,
                        uint64_t out[4], void *stream);

/* The carried byte of every flow record into out[capacity] (device bytes; the id bound is the
 * table's capacity, gpd_flow_stats.capacity).  Only a connection's record c carries its state;
 * the peer record's byte stays zero.  Asynchronous on `stream`. */
int gpd_tcp_tracker_states(gpd_tcp_tracker *t, uint8_t *out, void *stream);

/* Returns the connections ids[0..m) (device u32; ids at or above the capacity are ignored) to
 * the fresh state.  Asynchronous on `stream`. */
int gpd_tcp_tracker_forget(gpd_tcp_tracker *t, const uint32_t *ids, uint64_t m, void *stream);

/* Every connection back to the fresh state.  Call it with gpd_flow_reset. */
int gpd_tcp_tracker_reset(gpd_tcp_tracker *t, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_TCPTRACK_H_ */
