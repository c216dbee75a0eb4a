/*
 * gpd_dns.h — C-ABI of the DNS message decode: (*DNS).DecodeFromBytes (layers/dns.go:304-392) for
 * every packet of a decoded device batch whose decode stopped at LayerTypeDNS.
 *
 * layers/ports.go:63,106 send UDP and TCP port 53 to LayerTypeDNS.  The engine carries that type
 * as a stop type (GPD_LT_DNS) and has no decoder for it: `decoded` ends at UDP or TCP and the
 * layers word's stop type is 107.  This hand-off decodes the message that follows, on the device,
 * without making DNS an engine decoder: the decode kernels, include/gpd.h and the ABI version are
 * as they were.  A caller with `&dns` in its DecodingLayerParser composes `decoded + [DNS]` from
 * the verdict.
 *
 * Candidates.  Packet i is a candidate when GPD_LAYERS_STOP(layers[i]) == GPD_LT_DNS and its
 * status class is not GPD_ST_DECODE_ERROR.  The result words were written under the context's
 * dispatch tables, so mutated port tables are honoured; the context must be the one that decoded
 * the batch (its tables locate the message).  `data` is the Payload of the last decoded layer:
 * for UDP udp.go:30-56 (Length trimmed to the captured bytes, Length == 0 the whole rest), for TCP
 * what follows the header inside the IPv4/IPv6 length (this reference version has no length
 * prefix handling for TCP: the two prefix bytes are decoded as the ID).  It is found by running
 * the generic decoder over the packet again, as the fragment and TCP hand-offs do, so any stack
 * the engine decodes is covered.  An empty payload never reaches the stop type: data_len >= 1.
 * A candidate whose header offsets word is saturated (GPD_HDR_TP == 0xFFFF under a TCP/UDP last
 * layer) or whose layer count is saturated gets GPD_DNS_DEFERRED with data_off/data_len filled.
 *
 * Decode.  DecodeFromBytes restated branch by branch: the 12-byte header (SetTruncated and
 * errDNSPacketTooShort below 12 bytes), QDCount questions (dns.go:636-651), ANCount, NSCount and
 * ARCount records (:710-738, rdata :906-993 against data[:end]), decodeName (:538-627) with its
 * per-level 255-byte test, its 255-level recursion limit and its pointer tests, the character
 * strings (:864-875), decodeOPTs (:877-904), the extended RCODE from OPT additionals (:377-379).
 * Every error return ends the call with the entries appended so far kept (:359,366,373).
 *
 * What the device produces is the validation and the decompressed names.  Fields that are plain
 * slices or fixed reads of rr.Data — IP, TXT, TXTs, the OPT list, URI, the MX/SRV numbers and the
 * five SOA words — are built by the caller from the record's offsets.
 *
 * Work budget.  work(message) is, up to the point where the reference returns: +1 per question
 * or record begun, +1 per decodeName call (recursive ones included), +1 per iteration of its
 * loop, +1 per byte appended to d.buffer (dots included), +1 per character string or OPT option
 * visited.  A message whose work exceeds gpd_dns_config.max_work gets GPD_DNS_DEFERRED: no
 * entries, no names, n_* zero, the header fields as read, rcode the header's.  Work only grows,
 * so an error met within the budget is an error verdict, and a budget passed before the error is
 * deferred.  gpd_dns_decode_host with max_work 0 decodes a deferred message in full.
 *
 * The record describes what this call assigned; what a reused DNS object keeps from an earlier
 * packet (d.Questions of a too-short packet, rr fields of a failed record) is not modelled.
 *
 * Reference interfaces the entry points replace (paths relative to google/gopacket):
 *   gpd_dns_decode        (*DNS).DecodeFromBytes, layers/dns.go:304-392, for every packet that
 *                         DecodingLayerParser.DecodeLayers (parser.go:302-316) would hand to a
 *                         registered &dns after UDP/TCP (layers/ports.go:63,106), with
 *                         DNSQuestion.decode :636-651, DNSResourceRecord.decode :710-738,
 *                         decodeRData :906-993, decodeName :538-627
 *   gpd_dns_decode_host   the same call for one message in host memory
 */
#ifndef GPD_DNS_H_
#define GPD_DNS_H_
#include "gpd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gpd_dns_msg.verdict: GPD_DNS_OK, or the error return that ended the call.  (a0, a1) are the
 * record's err_arg0 / err_arg1, the arguments of the error's text. */
#define GPD_DNS_OK 0u
#define GPD_DNS_E_TOO_SHORT 1u          /* dns.go:307-310   "DNS packet too short" (truncated = 1) */
#define GPD_DNS_E_MAX_RECURSION 2u      /* :539-540         "max DNS recursion level hit" */
#define GPD_DNS_E_NAME_OFFSET_HIGH 3u   /* :541-542         "dns name offset too high" */
#define GPD_DNS_E_NAME_OFFSET_NEG 4u    /* :543-544         "dns name offset is negative"; unreachable:
                                           offsets are indices and 14-bit pointers */
#define GPD_DNS_E_NAME_TOO_LONG 5u      /* :564-565         "dns name is too long" */
#define GPD_DNS_E_NAME_INVALID_INDEX 6u /* :566-567         "dns name uncomputable: invalid index"
                                           (index2 > len(data); index2 < index+1 is unreachable) */
#define GPD_DNS_E_POINTER_HIGH 7u       /* :593-594,597-598 "dns offset pointer too high" */
#define GPD_DNS_E_INDEX_RANGE 8u        /* :619-620         "dns index walked out of range" */
#define GPD_DNS_E_NAME_NO_DATA 9u       /* :1098            "no dns data found for name"; never returned */
#define GPD_DNS_E_LABEL_40 10u          /* :611-613         "qname '0x40' - RFC 2673 unsupported yet
                                           (data=%x index=%d)" (a0 = data[index], a1 = index) */
#define GPD_DNS_E_LABEL_80 11u          /* :615-617         "qname '0x80' unsupported yet (data=%x
                                           index=%d)" (a0 = data[index], a1 = index) */
#define GPD_DNS_E_QUESTION_SMALL 12u    /* :642-643         "DNS question too small" */
#define GPD_DNS_E_RECORD_SMALL 13u      /* :716-717         "DNS record too small" */
#define GPD_DNS_E_RECORD_LENGTH 14u     /* :726-727         "resource record length exceeds data" */
#define GPD_DNS_E_CHAR_STRING 15u       /* :869-870         "Insufficient data for a <character-string>" */
#define GPD_DNS_E_SOA_SMALL 16u         /* :947-948         "SOA too small" */
#define GPD_DNS_E_MX_SMALL 17u          /* :957-958         "MX too small" */
#define GPD_DNS_E_URI_SMALL 18u         /* :967-968         "URI too small" */
#define GPD_DNS_E_SRV_SMALL 19u         /* :974-975         "SRV too small" */
#define GPD_DNS_E_OPT_SHORT 20u         /* :885-886         "DNSOPT record is of length %d, it should be
                                           at least length 4" (a0 = end - offset) */
#define GPD_DNS_E_OPT_MALFORMED 21u     /* :891-892         "Malformed DNSOPT record.  Length %d < %d"
                                           (a0 = len(data), a1 = i + 4) */
#define GPD_DNS_E_OPT_LENGTH 22u        /* :896-897         "Malformed DNSOPT record. The length (%d)
                                           field implies a packet larger than the one received" (a0 = l) */
#define GPD_DNS_E_BAD_QDCOUNT 23u       /* :382-389         the four count checks; unreachable: each loop */
#define GPD_DNS_E_BAD_ANCOUNT 24u       /*                  appends exactly its count or returns */
#define GPD_DNS_E_BAD_NSCOUNT 25u
#define GPD_DNS_E_BAD_ARCOUNT 26u
#define GPD_DNS_E_COUNT 27u
#define GPD_DNS_DEFERRED 255u           /* work > max_work (or saturated offsets): decode on the host */

#define GPD_DNS_SEC_QUESTION 0u
#define GPD_DNS_SEC_ANSWER 1u
#define GPD_DNS_SEC_AUTHORITY 2u
#define GPD_DNS_SEC_ADDITIONAL 3u

#define GPD_DNS_MAX_WORK_DEFAULT 4096u
#define GPD_DNS_MAX_WORK_LIMIT 65535u

/* One candidate, in packet order (48 bytes).  For GPD_DNS_E_TOO_SHORT the header fields and the
 * counts are zero. */
typedef struct gpd_dns_msg {
  uint32_t packet;      /* its index in the batch */
  uint32_t data_off;    /* offset of data in the packet */
  uint32_t data_len;    /* len(data) */
  uint16_t id;          /* d.ID */
  uint16_t flags;       /* bytes 2..3 as one big-endian value: QR OpCode AA TC RD RA Z RCODE */
  uint16_t qdcount, ancount, nscount, arcount; /* as on the wire */
  uint16_t n_q, n_an, n_ns, n_ar; /* len(d.Questions) .. len(d.Additionals) as the call leaves them */
  uint8_t rcode;        /* d.ResponseCode after the OPT extension (:377-379) */
  uint8_t verdict;      /* GPD_DNS_OK, GPD_DNS_E_*, GPD_DNS_DEFERRED */
  uint8_t truncated;    /* the call set Truncated */
  uint8_t reserved;     /* zero */
  uint32_t err_arg0, err_arg1;
  uint32_t first_entry; /* its entries: entries[first_entry .. first_entry + n_q + n_an + n_ns + n_ar) */
} gpd_dns_msg;

/* One question or resource record (32 bytes), in the order questions, answers, authorities,
 * additionals.  Its names lie back to back in names[]: Name at name_off, then the rdata's first
 * name, then its second, each as the reference returns it (labels joined by '.', no leading dot). */
typedef struct gpd_dns_entry {
  uint32_t name_off;    /* into names[] */
  uint16_t name_len;    /* Name */
  uint16_t rname1_len;  /* NS / CNAME / PTR / MX.Name / SRV.Name / SOA.MName */
  uint16_t rname2_len;  /* SOA.RName */
  uint16_t type;
  uint16_t klass;
  uint16_t rdlength;    /* DataLength (questions: 0) */
  uint32_t ttl;
  uint32_t rdata_off;   /* offset of rr.Data in data (questions: 0) */
  uint32_t fixed_off;   /* offset in data of SOA's Serial; 0 otherwise */
  uint8_t section;      /* GPD_DNS_SEC_* */
  uint8_t reserved[3];  /* zero */
} gpd_dns_entry;

typedef struct gpd_dns_config {
  uint32_t max_work;    /* 1 .. GPD_DNS_MAX_WORK_LIMIT */
  uint32_t reserved;    /* zero */
} gpd_dns_config;

/* Device arrays of the caller with their capacities in elements (msgs and entries 16-byte
 * aligned).  A pointer may be NULL when its capacity is 0. */
typedef struct gpd_dns_out {
  gpd_dns_msg *msgs;
  uint64_t cap_msgs;
  gpd_dns_entry *entries;
  uint64_t cap_entries;
  uint8_t *names;
  uint64_t cap_names;
} gpd_dns_out;

typedef struct gpd_dns_counts {
  uint64_t msgs;        /* candidates */
  uint64_t entries;
  uint64_t name_bytes;
  uint64_t deferred;    /* messages with verdict GPD_DNS_DEFERRED */
  uint64_t work;        /* gpd_dns_decode_host: the message's work as far as it was counted; else 0 */
} gpd_dns_counts;

/* Every candidate of the batch `in` that ctx decoded into `res` (hdr_off required; status +
 * layers, or records), in packet order.  cfg NULL: max_work = GPD_DNS_MAX_WORK_DEFAULT; a max_work
 * outside 1..65535 is GPD_ERR_INVALID.  On GPD_OK `counts` holds the three totals and the number
 * deferred, and out's arrays hold that many elements.  When a capacity is short the call returns
 * GPD_ERR_INVALID (as the writers do for out_cap) with `counts` holding the exact needs and the
 * contents of out unspecified: allocate and call again (all capacities 0 is the sizing call).
 * Limits (GPD_ERR_INVALID otherwise): in->n < 2^32 - 256, entries and name bytes below 2^32.
 * Synchronises `stream` and restores the caller's current device. */
int gpd_dns_decode(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res, const gpd_dns_config *cfg,
                   const gpd_dns_out *out, gpd_dns_counts *counts, void *stream);

/* One message in host memory, no device: the same walk.  max_work 0: no budget.  msg->packet,
 * data_off and first_entry are 0, data_len is len.  `counts` as above (msgs = 1); a short
 * cap_entries / cap_names returns GPD_ERR_INVALID with the needs in counts and *msg filled.
 * It serves deferred messages and DNS over a reassembled TCP stream. */
int gpd_dns_decode_host(const uint8_t *data, uint32_t len, uint32_t max_work, gpd_dns_msg *msg,
                        gpd_dns_entry *entries, uint64_t cap_entries, uint8_t *names, uint64_t cap_names,
                        gpd_dns_counts *counts);

#ifdef __cplusplus
}
#endif
#endif /* GPD_DNS_H_ */
