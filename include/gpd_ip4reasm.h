/*
 * gpd_ip4reasm.h — C-ABI of the IPv4 defragmentation: ip4defrag's datagrams rebuilt on the device
 * from the fragment hand-off (gpd_ip4_fragments, include/gpd_defrag.h).
 *
 * The hand-off gives, in packet order, the packets IPv4Defragmenter.DefragIPv4WithTimestamp
 * (ip4defrag/defrag.go:86-135, paths relative to google/gopacket) does not return untouched, each
 * with its key ipv4{NetworkFlow(), Id} (:331-342), the fields insert and build read and the
 * verdict of securityChecks (:175-198).  A gpd_ip4_defrag object is the stateful rest: it holds
 * the fragment lists of the running datagrams (the ipFlows map, :346-349) in device memory,
 * payload bytes included, and gpd_ip4_defrag_run does for a whole hand-off what that call does
 * per packet, as if it were made for frags[0], frags[1], ... in order:
 *   fragmentList.insert (:216-273) with its uint16 Highest and Current, the ignored duplicate
 *   (:225-240) and the fragment that is counted without being stored (offset below Highest but
 *   above every stored offset, :222-249); build (:278-328) with the overlap's `currentOffset +
 *   FragOffset*8` (:298); the flush of a list that reaches IPv4MaximumFragmentListLen = 8192
 *   (:120-125); the flush after a successful build (:128-133).  After "hole found" or "invalid
 *   fragment" the list stays, as in the reference: only a datagram or the length limit flushes.
 *
 * The one deliberate addition.  build returns a struct with Length = Highest and Checksum = 0
 * (:309-324); gpd_ip4_dgram keeps those values.  The datagram's bytes, however, are written as a
 * packet the parser decodes with first layer IPv4, so that a reassembled datagram can re-enter
 * decode -> flow table -> tcpassembly: 4*ihl header bytes, then the payload.  The header is the
 * completing fragment's header bytes (options included) with three patches: bytes 6-7 zero (Flags,
 * FragOffset); bytes 2-3 = 4*ihl + payload_len when that is <= 65535, else 0, which
 * DecodeFromBytes reads as len(data) (layers/ip4.go:214-218); bytes 10-11 = the header checksum
 * over the result.
 *
 * GPD_IP4_D_SHORT_SLICE.  build appends frag.Payload[startAt:] for an overlapping fragment after
 * checking startAt against Length-20 (:291-297), not against len(Payload).  With IHL > 5 or a
 * truncated capture startAt can pass len(Payload): Go panics there.  Here nothing is appended
 * for that fragment and the datagram carries the flag.
 *
 * Reference interfaces the entry points replace:
 *   gpd_ip4_defrag_create / destroy   NewIPv4Defragmenter (:353-357) and its garbage collection
 *   gpd_ip4_defrag_run                DefragIPv4WithTimestamp (:86-135) per handed-over packet, with
 *                                     fragmentList.insert (:216-273), build (:278-328), flush (:154-158)
 *   gpd_ip4_defrag_discard            DiscardOlderThan (:140-151)
 *   gpd_ip4_defrag_stats              len(ipFlows) and the lists' lengths (no reference call)
 */
#ifndef GPD_IP4REASM_H_
#define GPD_IP4REASM_H_
#include "gpd_defrag.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPD_IP4_MAX_LIST_LEN 8192u /* IPv4MaximumFragmentListLen (:39) */

/* what DefragIPv4WithTimestamp returned for one hand-off record */
#define GPD_IP4_FILED     0u /* (nil, nil): stored, ignored as a duplicate (:225-240), or counted
                                without being stored (:222-249); the caller of the reference
                                cannot tell these apart */
#define GPD_IP4_COMPLETE  1u /* (out, nil); `datagram` indexes dgrams[] */
#define GPD_IP4_REJECTED  2u /* securityChecks (:175-198); the record's verdict has the text */
#define GPD_IP4_UNCHANGED 3u /* (in, nil): verdict GPD_FRAG_WHOLE */
#define GPD_IP4_HOLE      4u /* "defrag: building - hole found" (:303) */
#define GPD_IP4_INVALID   5u /* "defrag: building - invalid fragment" (:295) */
#define GPD_IP4_LIST_FULL 6u /* "defrag: Fragment List hits its maximum size(8192), without
                                success. Flushing the list" (:120-125) */

/* One outcome per hand-off record (8 B). */
typedef struct gpd_ip4_outcome {
  uint32_t what;     /* GPD_IP4_* */
  uint32_t datagram; /* index in dgrams[] when what == GPD_IP4_COMPLETE, else 0 */
} gpd_ip4_outcome;

/* One reassembled datagram (32 B): the layers.IPv4 build returns (:309-326). */
typedef struct gpd_ip4_dgram {
  uint32_t packet;      /* the completing packet: out takes its header fields (:309-324) */
  uint32_t frag;        /* its index in frags[] */
  uint64_t byte_off;    /* the datagram's place in `bytes`: 4*ihl header bytes, then the payload */
  uint32_t payload_len; /* len(out.Payload): the sum of the appended slices, not Highest */
  uint32_t nfrags;      /* the list's length at build */
  uint16_t length;      /* out.Length = Highest: the reference's value, header not counted */
  uint16_t id;          /* out.Id */
  uint8_t  ihl;         /* out.IHL */
  uint8_t  protocol;    /* out.Protocol */
  uint16_t flags;       /* GPD_IP4_D_* */
} gpd_ip4_dgram;
#define GPD_IP4_D_SHORT_SLICE 1u

typedef struct gpd_ip4_defrag gpd_ip4_defrag;

/* NewIPv4Defragmenter (:353-357).  The object owns the carried lists and its scratch (device
 * memory of the context's device, grown on demand); it serves one call at a time and must be
 * destroyed before its context. */
int gpd_ip4_defrag_create(gpd_ctx *ctx, gpd_ip4_defrag **d);
void gpd_ip4_defrag_destroy(gpd_ip4_defrag *d);

/* DefragIPv4WithTimestamp for a whole hand-off.  `in` is the batch gpd_ip4_fragments read and
 * frags[count] (device) what it wrote: in packet order and complete.  A hand-off cut short by
 * its max_out would report holes or never complete its datagrams; it cannot be told from a
 * complete one here, so the caller passes the count gpd_ip4_fragments returned and an array that
 * holds as many (the Python and Go bindings refuse anything else).  Records whose `packet` does
 * not rise strictly, or lies outside the batch, are refused with GPD_ERR_INVALID.
 * ts_ns: NULL, or a device u64[in->n], the array pcap ingest fills; a record's LastSeen is
 * ts_ns[packet], or now_ns with ts_ns == NULL.
 *
 * Outputs, all device memory, 16-byte aligned.  outcomes[count]: one per record.  dgrams[]: one
 * per reassembled datagram, in the order of their completing packets.  {bytes, out[2], offset,
 * caplen, out[0]} is a gpd_batch the parser decodes with first layer IPv4: datagram k is
 * bytes[offset[k], offset[k] + caplen[k]), back to back in datagram order (see above for the
 * header).  Fragments that stay in a list are copied into the object, so the caller may free or
 * reuse the batch afterwards.
 *
 * Capacity, as for gpd_tcp_assemble.  out[] = {datagrams, outcomes written, bytes, lists held
 * afterwards} (host words), known before anything is written.  When datagrams > max_dgrams or
 * bytes > max_bytes nothing is written, the carried lists are unchanged, out[] says what is
 * needed (out[1] = 0, out[3] = what would be held) and the call returns GPD_ERR_INVALID.
 * dgrams == NULL with max_dgrams == 0 is the sizing call (out[] only, GPD_OK, nothing changed).
 * bytes == NULL with max_bytes == 0 and dgrams != NULL: outcomes and records only (offset and
 * caplen may then be NULL too); the lists advance.
 * Limits (GPD_ERR_INVALID otherwise): in->n <= 2^32 - 256, in->data_len < 2^32 - 16, count plus
 * the carried fragments < 2^31, output bytes and carried bytes < 2^32 - 16 each.
 * Synchronises `stream`. */
int gpd_ip4_defrag_run(gpd_ip4_defrag *d, const gpd_batch *in, const gpd_ip4_frag *frags, uint64_t count,
                       const uint64_t *ts_ns, uint64_t now_ns,
                       gpd_ip4_outcome *outcomes, gpd_ip4_dgram *dgrams, uint64_t max_dgrams,
                       uint32_t *offset, uint32_t *caplen, uint8_t *bytes, uint64_t max_bytes,
                       uint64_t out[4], void *stream);

/* DiscardOlderThan (:140-151): drops the lists with LastSeen < t_ns; *n (host) = their count. */
int gpd_ip4_defrag_discard(gpd_ip4_defrag *d, uint64_t t_ns, uint64_t *n);

/* out[3] (host) = {lists, fragments, payload bytes} currently held. */
int gpd_ip4_defrag_stats(gpd_ip4_defrag *d, uint64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* GPD_IP4REASM_H_ */
