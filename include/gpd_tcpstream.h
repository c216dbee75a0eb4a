/*
 * gpd_tcpstream.h — C-ABI of the TCP stream assembly: tcpassembly's Reassembly lists for the
 * connections of a decoded batch, built on the device from the grouped segment hand-off
 * (gpd_tcp_segments, include/gpd_tcpassembly.h).
 *
 * The hand-off groups a batch's segments by connection key, each group in capture order.
 * gpd_tcp_assemble runs, for every group except the trailing GPD_TCP_UNGROUPED one, exactly what
 * the reference runs for that key, in this order (paths relative to google/gopacket):
 *   1. Assembler.AssembleWithTimestamp (tcpassembly/assembly.go:533-607) for each segment of the
 *      group in order, getConnection(end = lookup_only) included (:550-551, 495-511): the
 *      first-SYN start (:569-579), the out-of-order insert into the connection's page list
 *      (insertIntoConn :712-727, pagesFromTCP :734-756 with pageBytes = 1900 :87, traverseConn
 *      :683-690, pushBetween :696-710), the contiguous delivery (byteSpan :609-620,
 *      sendToConnection :624-633, addContiguous :636-640, addNextFromConn :760-780) and the
 *      close on End (closeConnection :666-676);
 *   2. the end-of-batch drain `for conn.first != nil && !conn.closed { skipFlush(conn) }`
 *      (skipFlush :645-657): FlushWithOptions{T: later than every packet, CloseAll: false}
 *      (:235-266) restricted to the batch's connections;
 *   3. with opts->close_all, the close of every connection that is still open: FlushAll
 *      (:276-287), which after the drain is one skipFlush on an empty list, a closeConnection.
 * The ungrouped run mixes keys: it is not assembled and gets no stream record; its segments stay
 * with the caller.
 *
 * A batch is the reordering horizon.  Out-of-order data still buffered when the batch ends is
 * flushed by step 2 with Reassembly.Skip set (the gap, or -1 before any sequence number was
 * known); it does not wait for the next batch.  After the drain an open connection is its
 * nextSeq and nothing else, which is what gpd_tcp_conn carries from batch to batch.
 *
 * Options.  max_pages_per_connection is AssemblerOptions.MaxBufferedPagesPerConnection
 * (:720-726; 0: no limit).  MaxBufferedPagesTotal couples all connections through one page
 * counter (a.pc.used, :721), so connections would no longer be independent: it is not offered.
 * FlushOlderThan by time (:269-271) is not offered either: step 2 is the only flush.  The flush
 * by time, and out-of-order data that waits across batches, are what the stateful assembler of
 * gpd_tcpasm.h (gpd_tcp_assembler_run) offers; this entry point stays as it is.
 *
 * Reference interfaces the entry point replaces:
 *   gpd_tcp_assemble   Assembler.AssembleWithTimestamp (:533-607) over whole connections,
 *                      FlushWithOptions (:235-266) / FlushAll (:276-287) at the batch's end, and
 *                      the Stream interface's inputs (Reassembled / ReassemblyComplete, :170-184)
 *                      as record arrays; Reassembly (:71-85) as gpd_tcp_reasm
 */
#ifndef GPD_TCPSTREAM_H_
#define GPD_TCPSTREAM_H_
#include "gpd_tcpassembly.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPD_TCP_PAGE_BYTES 1900u /* pageBytes (:87) */

/* One connection between batches (8 B).  All zero: no connection in the pool. */
typedef struct gpd_tcp_conn {
  uint32_t next_seq; /* conn.nextSeq (valid whenever the connection is open after a drain) */
  uint32_t flags;    /* GPD_TCP_CONN_OPEN */
} gpd_tcp_conn;
#define GPD_TCP_CONN_OPEN 1u

typedef struct gpd_tcp_asm_opts {
  uint32_t max_pages_per_connection; /* MaxBufferedPagesPerConnection; 0: none */
  uint32_t close_all;                /* nonzero: step 3, FlushAll's close */
} gpd_tcp_asm_opts;

/* One Reassembly handed to Stream.Reassembled (32 B). */
typedef struct gpd_tcp_reasm {
  uint32_t packet;     /* packet the bytes come from (Reassembly.Seen is its timestamp) */
  uint32_t src_off;    /* offset of Bytes[0] in that packet (zero-copy use); 0 when len is 0 */
  uint32_t len;        /* len(Bytes) after byteSpan's trim (:609-620); may be 0 */
  int32_t skip;        /* Reassembly.Skip: 0, a gap (2^31 - 1 for a larger one), or -1 (:761-765) */
  uint64_t stream_off; /* offset of Bytes in `bytes` */
  uint32_t call;       /* index of the Reassembled() call within the group: equal => one []Reassembly */
  uint16_t flags;      /* GPD_TCP_R_* */
  uint16_t reserved;   /* zero */
} gpd_tcp_reasm;
#define GPD_TCP_R_START 1u   /* Reassembly.Start (:576) */
#define GPD_TCP_R_END 2u     /* Reassembly.End (:599, 754) */
#define GPD_TCP_R_FLUSHED 4u /* the call was made by the end-of-batch drain (skipFlush) */

/* One assembled group (48 B). */
typedef struct gpd_tcp_stream {
  uint32_t flow_id, first_rec, nrec, ncalls; /* recs[first_rec, first_rec + nrec), calls 0..ncalls-1 */
  uint64_t byte_off, nbytes;                 /* bytes[byte_off, byte_off + nbytes) */
  uint32_t completed;                        /* ReassemblyComplete calls made for this key in this batch */
  uint32_t open;                             /* connection still in the pool afterwards */
  uint32_t next_seq;                         /* valid when open */
  uint32_t reserved;                         /* zero */
} gpd_tcp_stream;

/* Stream assembly of a grouped hand-off.  `in` is the batch gpd_tcp_segments read; segs[count]
 * and groups[ngroups] are the device arrays that call filled for it (flow_id given).
 *
 * state: NULL, or a device array of id_bound connections indexed by flow record, zeroed by the
 * caller once and again on gpd_flow_reset.  With state == NULL every group starts with no
 * connection; otherwise the group of flow record r starts from state[r] and writes it back
 * (zero when the connection closed or never opened).
 *
 * Records.  recs[] holds one record per Reassembly, dense, in group order and within a group in
 * delivery order; records with the same `call` form one Reassembled([]Reassembly) call.
 * ReassemblyComplete follows exactly those calls whose last record has GPD_TCP_R_END; with
 * close_all there is one more at the end for a connection that was still open (streams[].completed
 * counts both).  streams[] gets one record per assembled group, in group order; bytes[] holds
 * each stream's record bytes back to back (stream_off, byte_off).
 *
 * Capacity, as for gpd_tcp_segments.  out[] = {records, streams, bytes, Reassembled calls} (host
 * words).  When records > max_recs or bytes > max_bytes nothing is written, state included,
 * out[] says what is needed and the call returns GPD_ERR_INVALID.  recs == NULL with
 * max_recs == 0 is the sizing call (out[] only, GPD_OK).  bytes == NULL with max_bytes == 0 and
 * recs != NULL: records only, no gather; the caller reads the payloads in place through `packet`
 * and `src_off`.  streams has room for ngroups records.  recs, streams and bytes are 16-byte
 * aligned device memory.
 * Limits (GPD_ERR_INVALID otherwise): in->n <= 2^32 - 256, in->data_len < 2^32 - 16,
 * ngroups <= count < 2^31, fewer than 2^32 pages in all.
 * Synchronises `stream`.  The context's scratch serves one call at a time. */
int gpd_tcp_assemble(gpd_ctx *ctx, const gpd_batch *in,
                     const gpd_tcp_seg *segs, uint64_t count,
                     const gpd_tcp_group *groups, uint64_t ngroups,
                     gpd_tcp_conn *state, uint32_t id_bound,
                     const gpd_tcp_asm_opts *opts,
                     gpd_tcp_reasm *recs, uint64_t max_recs,
                     gpd_tcp_stream *streams,
                     uint8_t *bytes, uint64_t max_bytes,
                     uint64_t out[4], void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_TCPSTREAM_H_ */
