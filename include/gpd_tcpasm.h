/*
 * gpd_tcpasm.h — C-ABI of the stateful TCP assembler: tcpassembly's Assembler + StreamPool as a
 * device object that keeps, per flow record, what the reference's `connection` keeps
 * (tcpassembly/assembly.go:374-383): nextSeq (invalidSequence included), lastSeen, pages and the
 * page list with each page's seq, bytes (<= 1900), End and Seen.  The page bytes are copied into
 * the object, so the caller may reuse a batch as soon as its run returns.
 *
 * gpd_tcp_assemble (include/gpd_tcpstream.h) treats a batch as the reordering horizon and drains
 * at its end.  Here nothing is drained: out-of-order data waits, across runs, for the segment
 * that fills the gap or for a flush by time, as in the reference.
 *
 * One run over a grouped hand-off (gpd_tcp_segments' segs[] / groups[]) does, for every
 * connection independently, what the reference does when its caller (paths relative to
 * google/gopacket, tcpassembly/assembly.go)
 *   1. calls AssembleWithTimestamp(netFlow, tcp, ts_ns[packet]) (:533-607) for each segment of
 *      the connection's group in capture order, starting from the carried connection and its
 *      carried page list (getConnection with end = lookup_only :495-511, conn.lastSeen :564-566,
 *      the first-SYN start :569-579, insertIntoConn :712-727 with pagesFromTCP :734-756,
 *      traverseConn :683-690, pushBetween :696-710 and the MaxBufferedPagesPerConnection pop
 *      :720-726 that counts carried pages, byteSpan :609-620, sendToConnection :624-633,
 *      addContiguous :636-640, addNextFromConn :760-780, closeConnection on End :666-676);
 *   2. then calls FlushWithOptions{T: before_ns, CloseAll: close_all} (:235-266):
 *      `for conn.first != nil && conn.first.Seen < T { skipFlush; if closed break }`, then
 *      `CloseAll && !closed && first == nil && lastSeen < T` -> closeConnection.  Both
 *      comparisons are strict, as time.Before is; T = 0 flushes nothing;
 *   3. then, with flush_all, calls FlushAll (:276-287): `for !conn.closed { skipFlush }`.
 * Steps 2 and 3 apply to every connection the object holds, whether or not it has segments in
 * this run; a run with count == 0 is a pure FlushOlderThan / FlushAll.  The trailing
 * GPD_TCP_UNGROUPED run is not assembled.  MaxBufferedPagesTotal couples all connections through
 * one counter and is not offered.
 *
 * Per stream, the sequence of New / Reassembled / ReassemblyComplete calls over any sequence of
 * runs equals that of one reference Assembler fed the same packets in capture order with the
 * same flush calls made at the run boundaries.
 *
 * Reference interfaces the entry points replace:
 *   gpd_tcp_assembler_create / _destroy  NewAssembler (:351-361) + NewStreamPool (:335-342)
 *   gpd_tcp_assembler_run                AssembleWithTimestamp (:533-607), FlushWithOptions
 *                                        (:235-266), FlushOlderThan (:269-271), FlushAll (:276-287)
 *   gpd_tcp_assembler_reset              a new StreamPool
 *   gpd_tcp_assembler_stats / _conns     StreamPool.connections() (:193-201), read-only
 */
#ifndef GPD_TCPASM_H_
#define GPD_TCPASM_H_
#include "gpd_tcpstream.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpd_tcp_assembler gpd_tcp_assembler;

#define GPD_TCP_CONN_NOSEQ 2u   /* the connection's nextSeq is invalidSequence (no SYN seen, nothing flushed) */
#define GPD_TCP_R_CARRIED 8u    /* the record's bytes come from a page carried from an earlier run */
#define GPD_TCP_NO_PACKET 0xFFFFFFFFu /* gpd_tcp_reasm.packet of such a record */

/* FlushOptions (:203-207) plus FlushAll. */
typedef struct gpd_tcp_flush {
  uint64_t before_ns; /* T; 0: nothing is before it */
  uint32_t close_all; /* CloseAll */
  uint32_t flush_all; /* nonzero: step 3 */
} gpd_tcp_flush;

/* One connection as the object holds it (24 B).  All zero: no connection. */
typedef struct gpd_tcp_conn_info {
  uint32_t next_seq;     /* conn.nextSeq; 0 with GPD_TCP_CONN_NOSEQ */
  uint32_t flags;        /* GPD_TCP_CONN_OPEN | GPD_TCP_CONN_NOSEQ */
  uint32_t pages;        /* conn.pages */
  uint32_t page_bytes;   /* bytes those pages hold */
  uint64_t last_seen_ns; /* conn.lastSeen */
} gpd_tcp_conn_info;

/* The object: connections for flow records [0, id_bound).  Of opts only
 * max_pages_per_connection is read (NULL: no limit).  It owns its carry and scratch, serves one
 * call at a time, and must be destroyed before its context. */
int gpd_tcp_assembler_create(gpd_ctx *ctx, uint32_t id_bound, const gpd_tcp_asm_opts *opts, gpd_tcp_assembler **a);
void gpd_tcp_assembler_destroy(gpd_tcp_assembler *a);

/* One run: steps 1 to 3 above.  `in` is the batch gpd_tcp_segments read, segs[count] and
 * groups[ngroups] the device arrays it filled (flow ids given).  ts_ns: NULL, or a device
 * u64[in->n] of packet timestamps; with NULL every timestamp is now_ns.  fl: NULL means
 * {0, 0, 0}.  With count == 0 or ngroups == 0 no segment is read and `in` may be NULL.
 *
 * Outputs, in the layouts of include/gpd_tcpstream.h:
 *   recs[]     one gpd_tcp_reasm per Reassembly, dense, stream after stream and in delivery order
 *              within a stream.  A record whose bytes come from a carried page has
 *              GPD_TCP_R_CARRIED, packet = GPD_TCP_NO_PACKET and src_off = 0.  GPD_TCP_R_FLUSHED
 *              marks the calls made by steps 2 and 3.
 *   seen_ns[]  NULL, or u64 parallel to recs: Reassembly.Seen, the page's Seen for carried and
 *              buffered data, the segment's timestamp for direct delivery.
 *   streams[]  one gpd_tcp_stream per group except the ungrouped one, in hand-off order; then one
 *              per held connection that had no group in this run and on which step 2 or 3 made a
 *              call or a completion, in ascending flow id.  `open` is GPD_TCP_CONN_OPEN |
 *              GPD_TCP_CONN_NOSEQ as applicable, `reserved` the pages the connection still
 *              buffers afterwards.
 *   bytes[]    each stream's record bytes back to back.
 *   out[8]     {records, streams, bytes, Reassembled calls, connections held after, pages held
 *              after, page bytes held after, 0} (host words).
 * Capacity.  out[] is known before anything is written.  When records > max_recs, streams >
 * max_streams or bytes > max_bytes nothing is written, the object is unchanged (the new carry is
 * built beside the old one and the two are swapped on success only), and the call returns
 * GPD_ERR_INVALID.  recs == NULL with max_recs == 0 is the sizing call: out[] only, nothing
 * changes.  Otherwise recs, streams and bytes are required (there is no records-only mode: a
 * carried record has no packet to read in place); all are 16-byte aligned device memory, seen_ns
 * 8-byte aligned.
 * Limits (GPD_ERR_INVALID otherwise): in->n <= 2^32 - 256, in->data_len < 2^32 - 16,
 * ngroups <= count < 2^31, pages of the call plus pages carried < 2^31, output bytes and carried
 * bytes each < 2^32 - 16, every group's flow_id < id_bound or GPD_TCP_UNGROUPED.
 * Synchronises `stream`. */
int gpd_tcp_assembler_run(gpd_tcp_assembler *a, const gpd_batch *in,
                          const gpd_tcp_seg *segs, uint64_t count,
                          const gpd_tcp_group *groups, uint64_t ngroups,
                          const uint64_t *ts_ns, uint64_t now_ns, const gpd_tcp_flush *fl,
                          gpd_tcp_reasm *recs, uint64_t max_recs, uint64_t *seen_ns,
                          gpd_tcp_stream *streams, uint64_t max_streams,
                          uint8_t *bytes, uint64_t max_bytes,
                          uint64_t out[8], void *stream);

/* Drops every connection (no call is made for them).  Call it with gpd_flow_reset. */
int gpd_tcp_assembler_reset(gpd_tcp_assembler *a, void *stream);

/* out[] = {connections, connections with pages, pages, page bytes} held (host words). */
int gpd_tcp_assembler_stats(gpd_tcp_assembler *a, uint64_t out[4]);

/* One record per flow id into out[id_bound] (device, 8-byte aligned).  Synchronises `stream`. */
int gpd_tcp_assembler_conns(gpd_tcp_assembler *a, gpd_tcp_conn_info *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_TCPASM_H_ */
