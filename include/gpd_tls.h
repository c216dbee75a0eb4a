/*
 * gpd_tls.h — C-ABI of the TLS record decode: (*TLS).DecodeFromBytes (layers/tls.go:118-194) for
 * every packet of a decoded device batch whose decode stopped at LayerTypeTLS, and for byte ranges
 * of a device buffer (reassembled TCP streams).
 *
 * layers/ports.go:64-73 send TCP 443, 636, 989, 990, 992-995 and 5061 to LayerTypeTLS.  The engine
 * carries that type as a stop type (GPD_LT_TLS) and has no decoder for it: `decoded` ends at TCP
 * and the layers word's stop type is 140.  This hand-off decodes the records that follow, on the
 * device, without making TLS an engine decoder: the decode kernels, include/gpd.h and the ABI
 * version are as they were.  A caller with `&tls` in its DecodingLayerParser composes
 * `decoded + [TLS]` from the verdict.
 *
 * Candidates (gpd_tls_decode).  Packet i is a candidate when GPD_LAYERS_STOP(layers[i]) ==
 * GPD_LT_TLS and its status class is not GPD_ST_DECODE_ERROR.  The result words were written under
 * the context's dispatch tables, so mutated port tables are honoured (a UDP port registered to
 * LayerTypeTLS counts too); the context must be the one that decoded the batch.  `data` is the
 * Payload of the last decoded layer, found as gpd_dns_decode finds it: the generic decoder runs
 * over the packet again.  TCP's payload is what follows the header inside the IPv4/IPv6 length, so
 * Ethernet padding is not part of `data`; the capture length bounds it.  An empty payload never
 * reaches the stop type: data_len >= 1.  A candidate whose header offsets word is saturated
 * (GPD_HDR_TP == 0xFFFF under a TCP/UDP last layer) or whose layer count is saturated gets
 * GPD_TLS_DEFERRED with data_off/data_len filled.
 *
 * Decode.  decodeTLSRecords (tls.go:130-194) restated branch by branch, its tail recursion as a
 * loop, in the reference's order of tests: fewer than 5 bytes (SetTruncated, "TLS record too
 * short"), the content type, 5 + Length against len(data) (SetTruncated), then the per-type rule
 * (tls_cipherspec.go:37-54, tls_alert.go:74-95, tls_appdata.go:22-34, tls_handshake.go:19-28).
 * Every error return ends the call with the records appended so far kept: DecodeFromBytes does
 * not clear its four lists on an error.  Handshake records carry their header only
 * (tls_handshake.go:26 is a TODO), Payload and EncryptedMsg are slices of `data` the caller takes
 * from the record's off and length.
 *
 * Contents.  tls.go:119 sets t.BaseLayer.Contents to data, and :139 sets it again in every
 * invocation that got past the `len(data) < 5` test, to the data that invocation was given.  So
 * after the call Contents begins at the last record whose header was read (contents_off) and runs
 * to the end of data.
 *
 * Work budget.  work(message) is the number of decodeTLSRecords invocations up to the reference's
 * return, the failing one included.  A message whose work exceeds gpd_tls_config.max_records gets
 * GPD_TLS_DEFERRED: no record entries, n_* zero, contents_off and err_off zero.  Work only grows,
 * so an error met within the budget is an error verdict.  A wire-size packet holds at most 292
 * records (all of Length 0); at the default only a crafted jumbo payload or stream defers.
 * gpd_tls_decode_host with max_records 0 decodes a deferred message in full.
 *
 * The record describes what this call assigned.  DecodeFromBytes truncates its four lists at
 * entry (:122-125), so a reused TLS object keeps nothing from an earlier packet: nothing is left
 * that is not modelled here.
 *
 * Reference interfaces the entry points replace (paths relative to google/gopacket):
 *   gpd_tls_decode         (*TLS).DecodeFromBytes, layers/tls.go:118-194, for every packet that
 *                          DecodingLayerParser.DecodeLayers (parser.go:302-316) would hand to a
 *                          registered &tls after TCP (layers/ports.go:64-73)
 *   gpd_tls_decode_ranges  the same call on the bytes tcpassembly hands a Stream
 *                          (Stream.Reassembled, tcpassembly/assembly.go:178), one call per byte range
 *   gpd_tls_decode_host    the same call for one message in host memory
 */
#ifndef GPD_TLS_H_
#define GPD_TLS_H_
#include "gpd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gpd_tls_msg.verdict: GPD_TLS_OK, or the error return that ended the call. */
#define GPD_TLS_OK 0u
#define GPD_TLS_E_TOO_SHORT 1u       /* tls.go:131-134  "TLS record too short" (truncated = 1) */
#define GPD_TLS_E_UNKNOWN_TYPE 2u    /* :146-148        "Unknown TLS record type"; :158-159 is the same
                                        test again and unreachable */
#define GPD_TLS_E_LENGTH_MISMATCH 3u /* :152-155        "TLS packet length mismatch" (truncated = 1) */
#define GPD_TLS_E_CCS_LENGTH 4u      /* tls_cipherspec.go:43-46 "TLS Change Cipher Spec record incorrect
                                        length" (truncated = 1) */
#define GPD_TLS_E_ALERT_SHORT 5u     /* tls_alert.go:80-83 "TLS Alert packet too short" (truncated = 1) */
#define GPD_TLS_E_APPDATA_LENGTH 6u  /* tls_appdata.go:28-30 "TLS Application Data length mismatch";
                                        unreachable: data[hl:tl] always has Length bytes */
#define GPD_TLS_E_COUNT 7u
#define GPD_TLS_DEFERRED 255u        /* work > max_records (or saturated offsets): decode on the host */

/* TLSType (tls.go:20-26) */
#define GPD_TLS_CHANGE_CIPHER_SPEC 20u
#define GPD_TLS_ALERT 21u
#define GPD_TLS_HANDSHAKE 22u
#define GPD_TLS_APPLICATION_DATA 23u

#define GPD_TLS_REC_ENCRYPTED 1u     /* gpd_tls_rec.flags bit 0: EncryptedMsg is set */

#define GPD_TLS_MAX_RECORDS_DEFAULT 1024u
#define GPD_TLS_MAX_RECORDS_LIMIT 1048576u

/* One message, in packet (or range) order (48 bytes, stored 16-byte aligned). */
typedef struct gpd_tls_msg {
  uint32_t packet;       /* its index in the batch; gpd_tls_decode_ranges: the range's index */
  uint32_t data_off;     /* offset of data in the packet; ranges: 0 */
  uint32_t data_len;     /* len(data) */
  uint32_t first_record; /* its entries: recs[first_record .. first_record + the four n_*) */
  uint32_t n_ccs;        /* len(t.ChangeCipherSpec) as the call leaves it */
  uint32_t n_handshake;  /* len(t.Handshake) */
  uint32_t n_appdata;    /* len(t.AppData) */
  uint32_t n_alert;      /* len(t.Alert) */
  uint32_t contents_off; /* t.BaseLayer.Contents = data[contents_off:] */
  uint32_t err_off;      /* GPD_TLS_OK: data_len; else the offset of the record, or short tail, at
                            which the reference returned: a stream consumer carries data[err_off:] */
  uint8_t verdict;       /* GPD_TLS_OK, GPD_TLS_E_*, GPD_TLS_DEFERRED */
  uint8_t truncated;     /* the call called SetTruncated */
  uint8_t reserved[6];   /* zero */
} gpd_tls_msg;

/* One appended record (16 bytes), in wire order.  A record whose own decodeFromBytes fails is not
 * appended and has no entry.  Payload (AppData) and EncryptedMsg (Alert with flags bit 0) are
 * data[off + 5 : off + 5 + length]. */
typedef struct gpd_tls_rec {
  uint32_t off;           /* offset of the record's header in data */
  uint16_t version;       /* TLSVersion */
  uint16_t length;        /* Length */
  uint32_t index_in_kind; /* its position in its own list */
  uint8_t content_type;   /* 20..23 */
  uint8_t a;              /* ChangeCipherSpec: Message after tls_cipherspec.go:48-51 (1 or 255);
                             Alert: Level (tls_alert.go:85-92; 255 when Length != 2); else 0 */
  uint8_t b;              /* Alert: Description (255 when Length != 2); else 0 */
  uint8_t flags;          /* GPD_TLS_REC_ENCRYPTED */
} gpd_tls_rec;

typedef struct gpd_tls_config {
  uint32_t max_records;   /* 1 .. GPD_TLS_MAX_RECORDS_LIMIT */
  uint32_t reserved;      /* zero */
} gpd_tls_config;

/* Device arrays of the caller with their capacities in elements (both 16-byte aligned).  A
 * pointer may be NULL when its capacity is 0. */
typedef struct gpd_tls_out {
  gpd_tls_msg *msgs;
  uint64_t cap_msgs;
  gpd_tls_rec *recs;
  uint64_t cap_recs;
} gpd_tls_out;

typedef struct gpd_tls_counts {
  uint64_t msgs;          /* candidates (ranges: n) */
  uint64_t records;
  uint64_t deferred;      /* messages with verdict GPD_TLS_DEFERRED */
  uint64_t work;          /* gpd_tls_decode_host: the message's work as far as it was counted; else 0 */
} gpd_tls_counts;

/* n byte ranges of one device buffer: range k is bytes[off[k] .. off[k] + len[k]).  off and len
 * are device arrays of n elements. */
typedef struct gpd_tls_ranges {
  const uint8_t *bytes;
  uint64_t nbytes;
  const uint64_t *off;
  const uint32_t *len;
  uint64_t n;
} gpd_tls_ranges;

/* Every candidate of the batch `in` that ctx decoded into `res` (hdr_off required; status +
 * layers, or records), in packet order.  cfg NULL: max_records = GPD_TLS_MAX_RECORDS_DEFAULT; a
 * max_records outside 1..2^20 is GPD_ERR_INVALID.  On GPD_OK `counts` holds the totals and the
 * number deferred, and out's arrays hold that many elements.  When a capacity is short the call
 * returns GPD_ERR_INVALID with `counts` holding the exact needs and the contents of out
 * unspecified: allocate and call again (all capacities 0 is the sizing call).  Limits
 * (GPD_ERR_INVALID otherwise): in->n < 2^32 - 256, records below 2^32.  Synchronises `stream` and
 * restores the caller's current device. */
int gpd_tls_decode(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res, const gpd_tls_config *cfg,
                   const gpd_tls_out *out, gpd_tls_counts *counts, void *stream);

/* The same walk over every range: each is one message (no candidate step), packet is the range's
 * index and data_off 0; len 0 decodes as too short.  No byte outside a range is read.  A range
 * that passes nbytes is detected on the device in the sizing pass: the call returns
 * GPD_ERR_INVALID with the number of such ranges in the error text and writes nothing to out.
 * Contract otherwise as gpd_tls_decode (ranges->n < 2^32 - 256). */
int gpd_tls_decode_ranges(gpd_ctx *ctx, const gpd_tls_ranges *ranges, const gpd_tls_config *cfg,
                          const gpd_tls_out *out, gpd_tls_counts *counts, void *stream);

/* One message in host memory, no device: the same walk.  max_records 0: no budget.  msg->packet,
 * data_off and first_record are 0, data_len is len.  `counts` as above (msgs = 1); a short
 * cap_recs returns GPD_ERR_INVALID with the need in counts and *msg filled.  It serves deferred
 * messages. */
int gpd_tls_decode_host(const uint8_t *data, uint32_t len, uint32_t max_records, gpd_tls_msg *msg,
                        gpd_tls_rec *recs, uint64_t cap_recs, gpd_tls_counts *counts);

#ifdef __cplusplus
}
#endif
#endif /* GPD_TLS_H_ */
