/*
 * gpd_dhcp.h — C-ABI of the DHCP message decode: (*DHCPv4).DecodeFromBytes (layers/dhcpv4.go:126-179,
 * option decode :558-578) and (*DHCPv6).DecodeFromBytes (layers/dhcpv6.go:89-124, option decode
 * dhcpv6_options.go:610-621) for every packet of a decoded device batch whose decode stopped at
 * LayerTypeDHCPv4 or LayerTypeDHCPv6.
 *
 * layers/ports.go:109-112 send UDP 67 and 68 to LayerTypeDHCPv4 and UDP 546 and 547 to
 * LayerTypeDHCPv6.  The engine carries both as stop types (GPD_LT_DHCPV4, GPD_LT_DHCPV6) and has no
 * decoder for either: `decoded` ends at UDP and the layers word's stop type is 118 or 134.  This
 * hand-off decodes the message that follows, on the device, without making DHCP an engine decoder:
 * the decode kernels, include/gpd.h and the ABI version are as they were.  A caller with `&dhcp4` or
 * `&dhcp6` in its DecodingLayerParser composes `decoded + [DHCPv4]` or `decoded + [DHCPv6]` from
 * the verdict.  No Payload follows: both layers leave Payload nil.
 *
 * Candidates.  Packet i is a candidate when GPD_LAYERS_STOP(layers[i]) is GPD_LT_DHCPV4 or
 * GPD_LT_DHCPV6 and its status class is not GPD_ST_DECODE_ERROR.  The result words were written
 * under the context's dispatch tables, so mutated port tables are honoured; the context must be the
 * one that decoded the batch.  `data` is the Payload of the last decoded layer, found as
 * gpd_dns_decode finds it: the generic decoder runs over the packet again.  UDP's payload is
 * trimmed to its Length field, so Ethernet padding is not part of `data`; the capture length
 * bounds it.  A candidate whose header offsets word is saturated (GPD_HDR_TP == 0xFFFF under a
 * TCP/UDP last layer) or whose layer count is saturated gets GPD_DHCP_DEFERRED with data_off,
 * data_len and version filled.  One compaction serves both versions; gpd_dhcp_msg.version says
 * which decode ran.
 *
 * DHCPv4 (dhcpv4.go:126-179), branch by branch in the reference's order:
 *   len(data) < 240      SetTruncated, "DHCPv4 length %d too short" (err_arg = len).  d.Options is
 *                        not cleared on this path, so a reused object keeps the options of an
 *                        earlier packet; that is not modelled: n_opts is 0 and the header fields 0.
 *   the header fields    assigned at :131-145 (ClientHWAddr at :143: see below), Options emptied at
 *                        :131; then the magic cookie
 *                        (:146-148): "Bad DHCP header", with the header fields filled.
 *   len(data) == 240     nil, Contents not set (:150-153).
 *   the option loop      (:157-174) Pad is appended with Length 0 and nil Data and advances one
 *                        byte; End stops the loop and is not appended; bytes after End are ignored;
 *                        a list that runs to the end of data without End is OK.  A lone non-Pad,
 *                        non-End type byte at the tail is DecOptionNotEnoughData (:568-570); the
 *                        `len(data) < 1` form (:559-562) cannot happen inside `start < stop`.  A
 *                        Length that passes the tail is DecOptionMalformed (:572-574).  Every
 *                        error keeps the options appended so far and returns without Contents.
 *   Contents = data      only when the loop completes (:176).
 * ClientHWAddr is data[28 : 28+d.HardwareLen] (:143).  HardwareLen is a uint8 (:89), so the sum
 * is uint8 arithmetic and wraps, as 4+o.Length wraps in uint16 in the DHCPv6 option decode.
 *   HardwareLen >= 228   the high bound is HardwareLen - 228 (0..27), below the low bound 28: the
 *                        slice expression panics for every message, whatever the buffer, with
 *                        "runtime error: slice bounds out of range [28:N]" (N in err_arg).  That
 *                        is a property of the message: GPD_DHCP_E_V4_HW_PANIC.  DecodeLayers
 *                        (parser.go:304-306,328-332) returns it as the error "panic: " + that
 *                        text unless IgnorePanic is set, in which case the panic reaches the
 *                        caller.  Operation .. RelayAgentIP were assigned and Options emptied;
 *                        ClientHWAddr, ServerName, File and the cookie test were not reached.
 *   213 <= HardwareLen <= 227 with 28 + HardwareLen > data_len
 *                        the reference slices by capacity: depending on the caller's buffer it
 *                        panics or returns bytes beyond the message.  Neither is a property of
 *                        the message.  The walk sets GPD_DHCP_HW_PAST_DATA and goes on as the
 *                        reference does when the capacity allows; it never reads past data_len,
 *                        and the bindings return the address clipped to `data`.  This is the one
 *                        place where the result is not the reference's.
 *
 * DHCPv6 (dhcpv6.go:89-124):
 *   len(data) < 4        SetTruncated, "DHCPv6 length %d too short" (err_arg = len).
 *   Contents = data      from :94 on, also when a later test fails.
 *   types 12 and 13      relay-forward and relay-reply need 34 bytes; below that SetTruncated and
 *                        "DHCPv6 length %d too short for message type %d" (err_arg = len, the type
 *                        in `op`).  They carry HopCount, LinkAddr = data[2:18], PeerAddr =
 *                        data[18:34]; the others TransactionID = data[1:4] (in `xid`, 24 bits).
 *   the option loop      16-bit code, 16-bit length.  A tail of 1 to 3 bytes is "not enough data to
 *                        decode" (dhcpv6_options.go:611-613).  4 + Length past the tail (tested in
 *                        int, :616) is "dhcpv6 option size < length %d", whose argument is
 *                        4 + o.Length in uint16 arithmetic and wraps: err_arg carries the wrapped
 *                        value.  The failing option is not appended.
 * (:619 slices data[4 : 4+o.Length] in uint16 too: an option of Length >= 0xFFFC that fits panics
 * in the reference.  It needs 65,536 bytes of data, more than a UDP datagram holds; the walk
 * appends such an option like any other.)
 *
 * Work budget.  work(message) is the number of option decodes begun, the failing one and End
 * included.  A message whose work exceeds gpd_dhcp_config.max_options gets GPD_DHCP_DEFERRED: no
 * option entries, every field but packet, data_off, data_len, first_opt and version zero.  A 1472-byte UDP
 * payload holds at most 1232 DHCPv4 options (all Pad) or 367 DHCPv6 options, so at the default
 * only a jumbo or reassembled crafted datagram defers.  gpd_dhcp_decode_host with max_options 0
 * decodes a deferred message in full.
 *
 * Reference interfaces the entry points replace (paths relative to google/gopacket):
 *   gpd_dhcp_decode       (*DHCPv4).DecodeFromBytes, layers/dhcpv4.go:126-179, and
 *                         (*DHCPv6).DecodeFromBytes, layers/dhcpv6.go:89-124, for every packet that
 *                         DecodingLayerParser.DecodeLayers (parser.go:302-316) would hand to a
 *                         registered &dhcp4 / &dhcp6 after UDP (layers/ports.go:109-112)
 *   gpd_dhcp_decode_host  the same calls for one message in host memory
 */
#ifndef GPD_DHCP_H_
#define GPD_DHCP_H_
#include "gpd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two stop types (layers/layertypes.go: LayerTypeDHCPv4 = 118, LayerTypeDHCPv6 = 134). */
#define GPD_LT_DHCPV4 118u
#define GPD_LT_DHCPV6 134u

/* gpd_dhcp_msg.verdict: GPD_DHCP_OK, or the error return (or the panic) that ended the call. */
#define GPD_DHCP_OK 0u
#define GPD_DHCP_E_V4_TOO_SHORT 1u      /* dhcpv4.go:127-130 "DHCPv4 length %d too short" (truncated = 1) */
#define GPD_DHCP_E_V4_BAD_MAGIC 2u      /* :146-148 InvalidMagicCookie "Bad DHCP header" */
#define GPD_DHCP_E_V4_OPT_NO_DATA 3u    /* :568-570 DecOptionNotEnoughData "Not enough data to decode" */
#define GPD_DHCP_E_V4_OPT_MALFORMED 4u  /* :572-574 DecOptionMalformed "Option is malformed" */
#define GPD_DHCP_E_V6_TOO_SHORT 5u      /* dhcpv6.go:90-93 "DHCPv6 length %d too short" (truncated = 1) */
#define GPD_DHCP_E_V6_RELAY_SHORT 6u    /* :100-103 "DHCPv6 length %d too short for message type %d"
                                           (truncated = 1) */
#define GPD_DHCP_E_V6_OPT_NO_DATA 7u    /* dhcpv6_options.go:611-613 "not enough data to decode" */
#define GPD_DHCP_E_V6_OPT_SIZE 8u       /* :616-618 "dhcpv6 option size < length %d" */
#define GPD_DHCP_E_V4_OPT_EMPTY 9u      /* dhcpv4.go:559-562 "Not enough data to decode"; unreachable:
                                           the loop hands decode at least one byte */
#define GPD_DHCP_E_V4_HW_PANIC 10u      /* dhcpv4.go:143 HardwareLen >= 228: the reference panics; DecodeLayers
                                           returns (parser.go:328-332)
                                           "panic: runtime error: slice bounds out of range [28:%d]" */
#define GPD_DHCP_E_COUNT 11u
#define GPD_DHCP_DEFERRED 255u          /* work > max_options (or saturated offsets): decode on the host */

/* gpd_dhcp_msg.mflags */
#define GPD_DHCP_CONTENTS 1u            /* BaseLayer.Contents was set to data */
#define GPD_DHCP_RELAY 2u               /* DHCPv6 relay form: HopCount, LinkAddr, PeerAddr */
#define GPD_DHCP_HW_PAST_DATA 4u        /* DHCPv4: HardwareLen < 228 and 28 + HardwareLen > data_len (see
                                           above) */

#define GPD_DHCP_V4_END 255u            /* DHCPOptEnd */
#define GPD_DHCP_V4_PAD 0u              /* DHCPOptPad */
#define GPD_DHCP_V6_RELAY_FORWARD 12u   /* DHCPv6MsgTypeRelayForward */
#define GPD_DHCP_V6_RELAY_REPLY 13u     /* DHCPv6MsgTypeRelayReply */

#define GPD_DHCP_MAX_OPTIONS_DEFAULT 2048u
#define GPD_DHCP_MAX_OPTIONS_LIMIT 65536u

/* One message, in packet order (48 bytes, stored 16-byte aligned).  The four IPs (data[12:28]),
 * ClientHWAddr (data[28:28+hlen], clipped to data), ServerName (data[44:108]), File
 * (data[108:236]), LinkAddr, PeerAddr and every option's Data are read from the message bytes at
 * these fixed offsets; they are not copied. */
typedef struct gpd_dhcp_msg {
  uint32_t packet;    /* its index in the batch */
  uint32_t data_off;  /* offset of data in the packet */
  uint32_t data_len;  /* len(data) */
  uint32_t first_opt; /* its entries: opts[first_opt .. first_opt + n_opts) */
  uint32_t n_opts;    /* len(d.Options) as the call leaves it */
  uint32_t xid;       /* v4: Xid; v6 non-relay: TransactionID as a 24-bit big-endian number */
  uint32_t err_off;   /* the offset in data where the reference returned: 0 for the length tests, 28
                         for the ClientHWAddr panic, 236 for the cookie, the failing option's first byte; GPD_DHCP_OK: data_len */
  uint32_t err_arg;   /* the error text's %d (the second, the message type, is `op`); else 0 */
  uint16_t secs;      /* v4: Secs */
  uint16_t flags;     /* v4: Flags */
  uint8_t verdict;    /* GPD_DHCP_OK, GPD_DHCP_E_*, GPD_DHCP_DEFERRED */
  uint8_t truncated;  /* the call called SetTruncated */
  uint8_t version;    /* 4 or 6: which decode ran */
  uint8_t op;         /* v4: Operation; v6: MsgType */
  uint8_t htype;      /* v4: HardwareType */
  uint8_t hlen;       /* v4: HardwareLen */
  uint8_t hops;       /* v4: HardwareOpts; v6 relay: HopCount */
  uint8_t mflags;     /* GPD_DHCP_CONTENTS | GPD_DHCP_RELAY | GPD_DHCP_HW_PAST_DATA */
  uint8_t reserved[4]; /* zero */
} gpd_dhcp_msg;

/* One appended option (8 bytes), in wire order.  v4: Data = data[off+2 : off+2+length] (Pad: nil);
 * v6: Data = data[off+4 : off+4+length]. */
typedef struct gpd_dhcp_opt {
  uint32_t off;       /* the option's first byte in data */
  uint16_t code;      /* v4: Type (8 bits); v6: Code */
  uint16_t length;    /* Length */
} gpd_dhcp_opt;

typedef struct gpd_dhcp_config {
  uint32_t max_options; /* 1 .. GPD_DHCP_MAX_OPTIONS_LIMIT */
  uint32_t reserved;    /* zero */
} gpd_dhcp_config;

/* Device arrays of the caller with their capacities in elements (both 16-byte aligned).  A
 * pointer may be NULL when its capacity is 0. */
typedef struct gpd_dhcp_out {
  gpd_dhcp_msg *msgs;
  uint64_t cap_msgs;
  gpd_dhcp_opt *opts;
  uint64_t cap_opts;
} gpd_dhcp_out;

typedef struct gpd_dhcp_counts {
  uint64_t msgs;      /* candidates */
  uint64_t options;
  uint64_t deferred;  /* messages with verdict GPD_DHCP_DEFERRED */
  uint64_t work;      /* gpd_dhcp_decode_host: the message's work as far as it was counted; else 0 */
} gpd_dhcp_counts;

/* Every candidate of the batch `in` that ctx decoded into `res` (hdr_off required; status +
 * layers, or records), in packet order.  cfg NULL: max_options = GPD_DHCP_MAX_OPTIONS_DEFAULT; a
 * max_options outside 1..65536 is GPD_ERR_INVALID.  On GPD_OK `counts` holds the totals and the
 * number deferred, and out's arrays hold that many elements.  When a capacity is short the call
 * returns GPD_ERR_INVALID with `counts` holding the exact needs and the contents of out
 * unspecified: allocate and call again (all capacities 0 is the sizing call).  Limits
 * (GPD_ERR_INVALID otherwise): in->n < 2^32 - 256, options below 2^32.  Synchronises `stream` and
 * restores the caller's current device. */
int gpd_dhcp_decode(gpd_ctx *ctx, const gpd_batch *in, const gpd_result *res, const gpd_dhcp_config *cfg,
                    const gpd_dhcp_out *out, gpd_dhcp_counts *counts, void *stream);

/* One message in host memory, no device: the same walk.  version is 4 or 6 (anything else is
 * GPD_ERR_INVALID); max_options 0: no budget.  msg->packet, data_off and first_opt are 0, data_len
 * is len.  `counts` as above (msgs = 1); a short cap_opts returns GPD_ERR_INVALID with the need in
 * counts and *msg filled.  It serves deferred messages. */
int gpd_dhcp_decode_host(uint32_t version, const uint8_t *data, uint32_t len, uint32_t max_options,
                         gpd_dhcp_msg *msg, gpd_dhcp_opt *opts, uint64_t cap_opts, gpd_dhcp_counts *counts);

#ifdef __cplusplus
}
#endif
#endif /* GPD_DHCP_H_ */
