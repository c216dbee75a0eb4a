/*
 * gpd_tcpassembly.h — C-ABI of the tcpassembly hand-off ("decoded batch ->
 * tcpassembly").
 *
 * The reference's consumer of decoded TCP layers is the stream assembler: for every packet the
 * application calls Assembler.AssembleWithTimestamp(netFlow, &tcp, ts)
 * (tcpassembly/assembly.go:533-607), which
 *   1. ignores the packet when it carries nothing the assembler acts on (:535:
 *      !SYN && !FIN && !RST && len(t.Payload) == 0);
 *   2. builds key{netFlow, t.TransportFlow()} (:543) and finds or creates the connection
 *      (getConnection, :495-511; with end = !SYN && len(t.Payload) == 0 a missing connection
 *      is not created, :550-551);
 *   3. hands Seq, the flags and the payload bytes to the connection's stateful insert
 *      (:567-607).
 * gpd_tcp_segments runs step 1 and reads everything steps 2 and 3 read from the TCP layer for a
 * whole decoded batch in HBM, and hands over exactly the packets for which step 1 does not
 * return early.  The key of step 2 is the flow table's record index (gpd_flow_insert,
 * include/gpd_flow.h): given the flow_id array, the segments are grouped by it, stably, so
 * several assemblers can each take whole connections and still see every connection's packets
 * in capture order, the one rule the assembler has.  The connection state (pages, nextSeq,
 * flushing) stays with the caller's assembler (out of scope).
 *
 * "t" is the DecodingLayerParser's TCP object after the call and netFlow comes from its network
 * object: the pair the flow table keys by.  For VXLAN it is the inner segment.
 *
 * Reference interfaces the entry point replaces (paths relative to google/gopacket):
 *   gpd_tcp_segments   the per-packet reads of AssembleWithTimestamp (tcpassembly/assembly.go:
 *                      535,543,550-551,567-571) for a batch, and the caller's group-by over
 *                      key (:289) that lets assemblers work in parallel
 */
#ifndef GPD_TCPASSEMBLY_H_
#define GPD_TCPASSEMBLY_H_
#include "gpd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One handed-over packet (32 B, host order). */
typedef struct gpd_tcp_seg {
  uint32_t packet;       /* index of the packet in the batch */
  uint32_t flow_id;      /* flow_id[packet] as given (GPD_FLOW_NONE when flow_id == NULL) */
  uint32_t seq;          /* t.Seq                                   (assembly.go:567) */
  uint32_t ack;          /* t.Ack (reassembly reads it; tcpassembly does not) */
  uint32_t payload_off;  /* offset of t.Payload in the packet */
  uint32_t payload_len;  /* len(t.Payload), after the IPv4/IPv6 length trimming
                            (ip4.go:214-236, ip6.go:245-275, the extension skipper ip6.go:443-461) */
  uint16_t tcp_off;      /* offset of t.Contents in the packet */
  uint16_t flags;        /* header bytes 12..13 & 0x1FF: NS,CWR,ECE,URG,ACK,PSH,RST,SYN,FIN
                            (tcp.go:241-249; SYN/FIN/RST are read at assembly.go:535,569,599) */
  uint8_t  lookup_only;  /* getConnection's `end` argument: !SYN && payload_len == 0 (:550-551) */
  uint8_t  reserved[3];  /* zero */
} gpd_tcp_seg;

#define GPD_TCP_FIN 0x001u
#define GPD_TCP_SYN 0x002u
#define GPD_TCP_RST 0x004u

/* One run of segs[] with the same key (16 B). */
typedef struct gpd_tcp_group {
  uint32_t flow_id;      /* the group's flow record, or GPD_TCP_UNGROUPED for the tail */
  uint32_t start, count; /* segs[start, start+count) */
  uint32_t first_packet; /* segs[start].packet, the group's earliest packet */
} gpd_tcp_group;
#define GPD_TCP_UNGROUPED 0xFFFFFFFFu

/* The hand-off for a decoded device batch: `in` is the batch gpd_decode read and `res` its
 * results on the device (status + layers, or records; hdr_off required).  The context must be
 * the one (same tables, decoders, options, first layer) that decoded the batch.
 * Limits (GPD_ERR_INVALID otherwise): in->n <= 2^32 - 256 and in->data_len < 2^32 - 16, as for
 * gpd_ip4_fragments and gpd_pcap_write; segs and groups 16-byte aligned (the records move as
 * 16-byte stores).
 *
 * A packet is handed over when the flow table would key it (a network and a transport endpoint,
 * both header offsets below 0xFFFF), its transport endpoint type is TCPPort, and
 * SYN || FIN || RST || payload_len > 0.
 *
 * flow_id == NULL: segs[] holds the handed-over packets in packet order; groups may be NULL;
 * *ngroups = *ungrouped = 0.
 * flow_id != NULL (the u32[n] device array gpd_flow_insert filled for this batch; id_bound the
 * table's capacity): segs[] is ordered by ascending flow_id and, within one id, by ascending
 * packet index.  Every segment whose id is >= id_bound (GPD_FLOW_FULL, an id flagged
 * GPD_FLOW_COLLISION, GPD_FLOW_NONE) goes to one trailing run in packet order, counted by
 * *ungrouped; it is the last group, with flow_id GPD_TCP_UNGROUPED.  (A key that got no record
 * got none for any of its packets, so that run assembled serially reorders no key.)
 * groups[0 .. *ngroups) describes the runs in segs[] order.
 *
 * max_out is the capacity of segs[] and of groups[] (ngroups <= count).  When the hand-off has
 * more than max_out segments nothing is written, *count says what is needed and the call returns
 * GPD_ERR_INVALID; segs == NULL with max_out == 0 is the sizing call (*count only, GPD_OK).
 * segs and groups are device memory; count, ngroups and ungrouped are host words.  Synchronises
 * `stream`.  The context's scratch serves one call at a time (as for gpd_pcap_write). */
int gpd_tcp_segments(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res,
                     const uint32_t *flow_id, uint32_t id_bound,
                     gpd_tcp_seg *segs, gpd_tcp_group *groups, uint64_t max_out,
                     uint64_t *count, uint64_t *ngroups, uint64_t *ungrouped, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_TCPASSEMBLY_H_ */
