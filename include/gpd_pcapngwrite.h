/*
 * gpd_pcapngwrite.h — C-ABI of the pcapng way out: the blocks of a pcapng stream built on the
 * host, and the kept packets of a device batch as enhanced packet blocks built on the device
 * (the writers).
 *
 * The reference writes a pcapng capture one block at a time: pcapgo.NgWriter puts a section
 * header, one interface description per AddInterface and one enhanced packet block per
 * WritePacket on an io.Writer (pcapgo/ngwrite.go).  Here the section, interface and statistics
 * blocks are small and built on the host into a caller's buffer; the packets are a batch in HBM
 * and a mask says which to keep: their blocks are built on the device by the stream compaction
 * gpd_pcap_write uses (include/gpd_pcapwrite.h), with the host-built blocks in front as a prefix.
 *
 * Reference interfaces each entry point replaces (paths relative to google/gopacket):
 *   gpd_pcapng_section_block    NgWriter.writeSectionHeader            pcapgo/ngwrite.go:187-234
 *   gpd_pcapng_interface_block  NgWriter.AddInterface                  pcapgo/ngwrite.go:237-298
 *   gpd_pcapng_stats_block      NgWriter.WriteInterfaceStats           pcapgo/ngwrite.go:301-353
 *                               (the options of all three: prepareNgOptions :102-115,
 *                                writeOptions :118-184)
 *   gpd_pcapng_write            the loop `for i in kept: w.WritePacket(ci[i], data[i])`
 *                               (WritePacket :356-392)
 *
 * Where this differs from the reference, and why:
 *  - The reference writes little-endian only; so does this.  A section info whose big_endian
 *    flag is set (as a reader of a big-endian capture returns it) is refused, not converted.
 *  - An option's length field has 16 bits and the reference truncates a longer string's length
 *    silently (:106), which leaves a stream no reader can follow.  A string of more than 65,535
 *    bytes (65,534 for the filter, which gains a byte) is refused with GPD_ERR_INVALID.
 *  - ngwrite.go:360-362 (`CaptureLength != len(data)`) cannot arise from a batch: both are
 *    caplen[i].
 *  - ngwrite.go:363-365's error text prints the CaptureInfo with %+v, which embeds a time.Time
 *    rendered in the process's local zone; the text is the one gpd_pcap_write gives:
 *      invalid capture info (packet %llu: capture length %u, length %u):  capture length > length
 *  - WritePacket takes ci.Timestamp.UnixNano() as it is (:371): no time.Now() for the zero time,
 *    and the interface's TimestampOffset is NOT subtracted, so a reader adds it again and a
 *    packet on an interface with offset 100 reads back 100 s later (ngwrite_test.go:208-210).
 *    ts_ns is written raw, as that bit pattern.
 *  - A descriptor that reaches past data_len is read as gpd_decode reads it: offset and caplen
 *    clamped to the buffer; the clamped caplen is the block's CaptureLength.
 *  - The block's total length is computed in 32 bits, as the reference computes it (:367-369).
 */
#ifndef GPD_PCAPNGWRITE_H_
#define GPD_PCAPNGWRITE_H_
#include "gpd.h"
#include "gpd_pcapng.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gpd_pcapng_write: the most bytes `prefix` may hold. */
#define GPD_PCAPNGW_MAX_PREFIX 65536u

/* NgNoValue64 (pcapng.go:120-121): a statistics counter that is not written. */
#define GPD_PCAPNG_NO_VALUE64 0xFFFFFFFFFFFFFFFFull

/* gpd_pcapng_write *bad_reason: which of WritePacket's checks stopped the loop. */
#define GPD_PCAPNGW_BAD_NONE   0u
#define GPD_PCAPNGW_BAD_IFACE  1u /* InterfaceIndex >= the interfaces added (ngwrite.go:357-359) */
#define GPD_PCAPNGW_BAD_LENGTH 2u /* CaptureLength > Length (ngwrite.go:363-365) */

/* NgInterfaceStatistics (pcapng.go:123-136).  A time is time.Time.UnixNano() as a bit pattern;
 * Go's zero time, which Unix nanoseconds cannot express, is has_* = 0. */
typedef struct gpd_pcapng_stats {
  uint64_t last_update;      /* LastUpdate; without has_last_update the block's timestamp is 0 (:332-335) */
  uint64_t start_time;       /* StartTime; written only with has_start_time (:308-312) */
  uint64_t end_time;         /* EndTime; written only with has_end_time (:313-317) */
  uint64_t packets_received; /* PacketsReceived; GPD_PCAPNG_NO_VALUE64: not written */
  uint64_t packets_dropped;  /* PacketsDropped; GPD_PCAPNG_NO_VALUE64: not written */
  uint32_t has_last_update, has_start_time, has_end_time;
  uint32_t reserved;
} gpd_pcapng_stats;

/* The three host-only block builders need no device and no context.  Each writes its block to
 * out[0, *len) and returns GPD_OK; out = NULL is a sizing call (*len alone); a block that does
 * not fit out_cap is GPD_ERR_INVALID with *len what it takes and nothing written.  Every block
 * is little-endian and a multiple of 4 bytes long.
 *
 * The strings of a gpd_pcapng_section_info / gpd_pcapng_iface are bytes [off, off + len) of
 * `strs` (strs_len bytes), as a reader returns them over its capture buffer; len = 0 is Go's
 * empty string (not written); off = UINT64_MAX with len > 0 is len zero bytes. */

/* writeSectionHeader (ngwrite.go:187-234): options in the order application, comment, hardware,
 * OS, then an end-of-options entry when there was at least one; version 1.0; the section length
 * field is 0xFFFFFFFFFFFFFFFF.  info->big_endian != 0 is GPD_ERR_INVALID. */
int gpd_pcapng_section_block(const gpd_pcapng_section_info *info, const uint8_t *strs, uint64_t strs_len,
                             uint8_t *out, uint64_t out_cap, uint64_t *len);

/* AddInterface (ngwrite.go:237-298): options in the order name, comment, description, filter
 * (one zero byte, then the string: :258-261), OS, if_tsoffset (only when nonzero), if_tsresol.
 * if_tsresol is always 9, whatever intf->ts_resolution says (:273-274), a 1-byte value stored in
 * 4 bytes (:168-173).  The scale fields of the struct are not looked at. */
int gpd_pcapng_interface_block(const gpd_pcapng_iface *intf, const uint8_t *strs, uint64_t strs_len,
                               uint8_t *out, uint64_t out_cap, uint64_t *len);

/* WriteInterfaceStats (ngwrite.go:301-353): options in the order start time, end time, dropped,
 * received; a time is the 64-bit value, high word first (:151-157).  intf outside [0, n_ifaces)
 * is GPD_ERR_PCAP with the reference's text (:302-304):
 *   Can't send statistics for non existent interface %d; have only %d interfaces */
int gpd_pcapng_stats_block(int64_t intf, uint32_t n_ifaces, const gpd_pcapng_stats *stats,
                           uint8_t *out, uint64_t out_cap, uint64_t *len);

/* The loop `for i in kept packets, ascending: w.WritePacket(ci[i], data[i])` (ngwrite.go:356-392)
 * over a device batch.
 *   in         the batch (device pointers, the usual batch contract: any layout)
 *   ts_ns      u64[n] device, the bit pattern of CaptureInfo.Timestamp.UnixNano(), written raw
 *   wirelen    u32[n] device, CaptureInfo.Length; NULL means Length = CaptureLength
 *   ifindex    u32[n] device, CaptureInfo.InterfaceIndex; NULL means interface 0 for every packet
 *   n_ifaces   the interfaces added so far (w.intf), which the indices are checked against
 *   keep       u8[n] device, nonzero = write this packet; NULL = every packet
 *   prefix     HOST bytes that stand in front of the first record: the section and interface
 *              blocks the builders made.  prefix_len is a multiple of 4 and at most
 *              GPD_PCAPNGW_MAX_PREFIX; NULL with 0 is a stream of records only, which is how a
 *              second batch is appended to a file.  The bytes are consumed before the call
 *              returns.
 *   out        device buffer, 16-byte aligned, out_cap bytes
 * Each kept packet becomes, little-endian, the 28 bytes {6, total, ifindex, uint32(ts >> 32),
 * uint32(ts), caplen, Length}, its caplen bytes, (4 - caplen & 3) & 3 zero bytes and `total`
 * again, where total = 32 + caplen + padding; back to back in ascending packet index.
 *
 * Returns through host pointers: *n_written (records), *bytes (stream length, prefix included),
 * *bad_index, *bad_reason.  The checks run per kept packet in the reference's order:
 * ifindex[i] >= n_ifaces (:357-359), then caplen > Length (:363-365).  The loop stops at the
 * lowest kept index that fails either: the records before it are written and counted, *bad_index
 * is its packet index (UINT64_MAX: none), *bad_reason the GPD_PCAPNGW_BAD_* check it failed, and
 * the call returns GPD_ERR_PCAP; gpd_last_error_string() gives the reference's interface text
 * (above, with the packet's index and n_ifaces) or the length text.  An unkept packet of that
 * kind is no error.
 *
 * Capacity as for gpd_pcap_write: when the stream does not fit out_cap, nothing is written to
 * `out`, *bytes and *n_written say what is needed and the call returns GPD_ERR_INVALID; out = NULL
 * with out_cap = 0 is a sizing call: the same counts, GPD_OK (or GPD_ERR_PCAP).  No byte of `out`
 * at or beyond *bytes is ever written.  Limits: n <= 2^32 - 256, data_len < 2^32 - 16.
 *
 * The sizes are computed first and read back (the call synchronises `stream` there); the copy is
 * then queued on `stream`.  The context's scratch, shared with gpd_pcap_write and
 * gpd_batch_select, serves one call at a time. */
int gpd_pcapng_write(gpd_ctx *ctx, const gpd_batch *in, const uint64_t *ts_ns, const uint32_t *wirelen,
                     const uint32_t *ifindex, uint32_t n_ifaces, const uint8_t *keep,
                     const uint8_t *prefix, uint32_t prefix_len, uint8_t *out, uint64_t out_cap,
                     uint64_t *n_written, uint64_t *bytes, uint64_t *bad_index, uint32_t *bad_reason,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_PCAPNGWRITE_H_ */
