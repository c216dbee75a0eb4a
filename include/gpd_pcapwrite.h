/*
 * gpd_pcapwrite.h — C-ABI of the way back out: selected packets of a device batch as a pcap
 * stream, or as a new dense batch (the writers).
 *
 * The reference writes a capture one packet at a time: pcapgo.Writer.WritePacket puts a 16-byte
 * record header and the packet's bytes on an io.Writer (pcapgo/write.go).  Here the packets are
 * a batch in HBM and a mask says which to keep: the stream is built on the device by a stream
 * compaction over variable-length records (a prefix sum of the record sizes, then one copy pass),
 * and stays there until the caller copies it where it wants it.
 *
 * Reference interfaces each entry point replaces (paths relative to google/gopacket):
 *   gpd_pcap_file_header   Writer.WriteFileHeader                        pcapgo/write.go:80-96
 *                          (NewWriter / NewWriterNanos :53-76 choose the magic; :98-99 the scaler)
 *   gpd_pcap_write         the loop `for i in kept: w.WritePacket(ci[i], data[i])`
 *                          (writePacketHeader :101-114, WritePacket :117-129)
 *   gpd_batch_select       (no reference counterpart: the kept packets copied out, as
 *                           `append(kept, data[i])` over a slice of packets would)
 *
 * Where this differs from the reference, and why:
 *  - write.go:118-120 (`CaptureLength != len(data)`) cannot arise from a batch: both are caplen[i].
 *  - write.go:103-105 substitutes time.Now() for the zero Timestamp.  Unix nanoseconds cannot
 *    express Go's zero time, so that substitution is the caller's: ts_ns is required.
 *  - write.go:121-123's error text prints the CaptureInfo with %+v, which embeds a time.Time
 *    rendered in the process's local zone and is not reproducible.  gpd_last_error_string() gives
 *      invalid capture info (packet %llu: capture length %u, length %u):  capture length > length
 *  - WritePacket never compares the capture length with the snap length; neither does this.
 *  - A descriptor that reaches past data_len is read as gpd_decode reads it: offset and caplen
 *    clamped to the buffer; the clamped caplen is the record's CaptureLength.
 */
#ifndef GPD_PCAPWRITE_H_
#define GPD_PCAPWRITE_H_
#include "gpd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPD_PCAPW_NANOS        1u /* NewWriterNanos: sub-second field in ns; otherwise µs (write.go:53-76,98-99) */
#define GPD_PCAPW_FILE_HEADER  2u /* the stream starts with WriteFileHeader's 24 bytes */

/* WriteFileHeader (write.go:80-96), host only, no device: always little-endian, version 2.4,
 * bytes 8..15 zero; the magic follows GPD_PCAPW_NANOS. */
int gpd_pcap_file_header(uint32_t flags, uint32_t snaplen, uint32_t linktype, uint8_t out[24]);

/* The loop `for i in kept packets, ascending: w.WritePacket(ci[i], data[i])` over a device batch.
 *   in       the batch (device pointers, the usual batch contract: any layout)
 *   ts_ns    u64[n] device, CaptureInfo.Timestamp as Unix ns (what gpd_pcap_index returns)
 *   wirelen  u32[n] device, CaptureInfo.Length; NULL means Length = CaptureLength
 *   keep     u8[n] device, nonzero = write this packet; NULL = every packet
 *   out      device buffer, 16-byte aligned, out_cap bytes
 * Each kept packet becomes the 16 little-endian bytes {uint32(ts / 1e9), uint32(ts % 1e9 / scaler),
 * caplen, Length} (scaler 1000, or 1 with GPD_PCAPW_NANOS) and its caplen bytes, back to back in
 * ascending packet index; snaplen and linktype are used by the file header only.
 *
 * Returns through host pointers: *n_written (records), *bytes (stream length, file header
 * included when asked for), *bad_index.  The loop stops at the first kept packet with
 * caplen > Length (write.go:121-123): the records before it are written and counted, *bad_index
 * is its packet index (UINT64_MAX: none) and the call returns GPD_ERR_PCAP.  An unkept packet of
 * that kind is no error.
 *
 * When the stream does not fit out_cap, nothing is written to `out`, *bytes and *n_written say
 * what is needed and the call returns GPD_ERR_INVALID (the text names both sizes).  out = NULL
 * with out_cap = 0 is a sizing call: the same counts, GPD_OK (or GPD_ERR_PCAP).  No byte of
 * `out` at or beyond *bytes is ever written.
 *
 * The sizes are computed first and read back (the call synchronises `stream` there, as
 * gpd_flow_keys does: they size the caller's next step); the copy is then queued on `stream`.
 * The context's scratch serves one call at a time. */
int gpd_pcap_write(gpd_ctx *ctx, const gpd_batch *in, const uint64_t *ts_ns, const uint32_t *wirelen,
                   const uint8_t *keep, uint32_t flags, uint32_t snaplen, uint32_t linktype,
                   uint8_t *out, uint64_t out_cap,
                   uint64_t *n_written, uint64_t *bytes, uint64_t *bad_index, void *stream);

/* The kept packets as a new dense batch: packet j of the output is the j-th kept packet, at
 * out_offset[j] = 16-byte-aligned running position, out_caplen[j] its caplen, out_index[j]
 * (may be NULL) its index in `in`; the three arrays hold max_out entries (more kept packets:
 * GPD_ERR_INVALID, nothing written).  *bytes is the new batch's data_len: the end of the last
 * packet's 16-byte slot.  It must stay < 2^32 - 16 (refused otherwise).  out_data (16-byte
 * aligned) holds out_cap >= *bytes bytes; the call writes whole slots, zero-filling a slot's
 * padding, and nothing at or beyond *bytes, so the result obeys the batch contract.  Capacity
 * and the sizing call (out_data = NULL, out_cap = 0) as for gpd_pcap_write. */
int gpd_batch_select(gpd_ctx *ctx, const gpd_batch *in, const uint8_t *keep,
                     uint8_t *out_data, uint64_t out_cap, uint32_t *out_offset, uint32_t *out_caplen,
                     uint32_t *out_index, uint64_t max_out, uint64_t *n_out, uint64_t *bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPD_PCAPWRITE_H_ */
