/*
 * gpd_pcapng.h — C-ABI of the pcapng ingest in front of the batched decoder.
 *
 * The reference reads a pcapng capture one block at a time: pcapgo.NewNgReader parses the first
 * section header (and, by default, the section's first interface), and every ReadPacketData
 * call skips to the next packet block and copies its bytes out (pcapgo/ngread.go).  Here a
 * capture that is already in memory is read through an opaque reader over the caller's buffer:
 * gpd_pcapng_index returns where each packet's bytes lie in the buffer, so the capture itself is
 * the decoder's batch buffer and nothing is repacked.
 *
 * The reader restates pcapgo's NgReader, not the pcapng standard: the trailing block length is
 * never looked at, `total_len - 8` wraps as uint32, any short read is io.EOF (text "EOF"), and so
 * on — see the stop codes below.  Where the reference would panic the reader stops with
 * GPD_PCAPNG_STOP_PANIC; it never faults on any input.
 *
 * Reference interfaces each entry point replaces (paths relative to google/gopacket):
 *   gpd_pcapng_open          pcapgo.NewNgReader                    pcapgo/ngread.go:61-83
 *                            (readBlock :127-152, readSectionHeader :197-269,
 *                             firstInterface :295-322, readInterfaceDescriptor :325-386)
 *   gpd_pcapng_index         the loop `for { data, ci, err := r.ReadPacketData() ... }`
 *                            (readPacketHeader :443-525, ReadPacketData :529-545,
 *                             convertTime :389-392, readInterfaceStatistics :395-438)
 *   gpd_pcapng_linktype      NgReader.LinkType()                   pcapgo/ngread.go:578-580
 *   gpd_pcapng_section       NgReader.SectionInfo()                pcapgo/ngread.go:583-585
 *   gpd_pcapng_interface     NgReader.Interface(i)                 pcapgo/ngread.go:588-593
 *   gpd_pcapng_ninterfaces   NgReader.NInterfaces()                pcapgo/ngread.go:596-598
 *   gpd_pcapng_resolution    NgReader.Resolution()                 pcapgo/ngread.go:601-606
 *   gpd_pcapng_skip_section  NgReader.SkipSection()                pcapgo/ngread.go:286-292
 *   gpd_pcapng_pos, gpd_pcapng_close, gpd_pcapng_last_error   (no reference counterpart)
 *   gpd_decode_pcapng        that loop feeding DecodingLayerParser.DecodeLayers
 *
 * The SectionEndCallback / StatisticsCallback options (ngread.go:31-35) have no counterpart:
 * statistics blocks are parsed (they can stop the reader) and their values dropped.
 */
#ifndef GPD_PCAPNG_H_
#define GPD_PCAPNG_H_
#include "gpd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Block types and magics (pcapgo/pcapng.go:24-41) */
#define GPD_PCAPNG_BLOCK_SECTION   0x0A0D0D0Au
#define GPD_PCAPNG_BLOCK_INTERFACE 1u
#define GPD_PCAPNG_BLOCK_PACKET    2u
#define GPD_PCAPNG_BLOCK_SIMPLE    3u
#define GPD_PCAPNG_BLOCK_STATS     5u
#define GPD_PCAPNG_BLOCK_ENHANCED  6u
#define GPD_PCAPNG_BYTE_ORDER      0x1A2B3C4Du

/* Returned when the reader stops with one of the reference's errors (or where it panics); the
 * text is in gpd_pcapng_last_error() and gpd_last_error_string(). */
#define GPD_ERR_PCAPNG (-6)

/* Why a walk ended (gpd_pcapng_index *stop).  Every stop but LIMIT is final: later calls on the
 * reader return the same stop and no packets. */
#define GPD_PCAPNG_STOP_LIMIT      0  /* max_n packets were returned; more may follow */
#define GPD_PCAPNG_STOP_EOF        1  /* "EOF" with no byte left where a block header would start */
#define GPD_PCAPNG_STOP_EOF_BLOCK  2  /* "EOF" inside a block (the reference cannot tell these apart) */
#define GPD_PCAPNG_STOP_NEGATIVE   3  /* "bufio: negative count": capture length beyond the block */
#define GPD_PCAPNG_STOP_IFACE_ID   4  /* "Interface id %d not present in section (have only %d interfaces)" */
#define GPD_PCAPNG_STOP_NO_IFACE   5  /* "At least one Interface is needed for a packet" */
#define GPD_PCAPNG_STOP_NO_FIRST   6  /* "A section must have an interface before a packet block" */
#define GPD_PCAPNG_STOP_BYTE_ORDER 7  /* "Wrong byte order value in Section Header" */
#define GPD_PCAPNG_STOP_OPT_END    8  /* "End of Options must be zero length" */
#define GPD_PCAPNG_STOP_VERSION    9  /* "Unknown pcapng Version in Section Header" */
#define GPD_PCAPNG_STOP_LINKTYPE   10 /* "Link type of current interface is different from first one" */
#define GPD_PCAPNG_STOP_PANIC      11 /* the reference panics here (text says where) */
#define GPD_PCAPNG_STOP_MAGIC      12 /* "Unknown magic %x" (gpd_pcapng_open only) */

/* NgReaderOptions (ngread.go:22-36) and this library's knobs. */
typedef struct gpd_pcapng_opts {
  uint32_t want_mixed_linktype;           /* WantMixedLinkType */
  uint32_t error_on_mismatching_linktype; /* ErrorOnMismatchingLinkType */
  uint32_t skip_unknown_version;          /* SkipUnknownVersion */
  int32_t device_walk;                    /* gpd_decode_pcapng: -1 automatic (on), 0 host walk only */
  uint64_t chunk_bytes;                   /* gpd_decode_pcapng: bytes per H2D chunk, a multiple of 2048
                                             in [4096, 64 MiB]; 0 = 64 MiB */
} gpd_pcapng_opts;

/* A string of the capture: bytes [off, off + len) of the reader's buffer.  off = UINT64_MAX
 * with len > 0 stands for len zero bytes (a zero-length option read before any other keeps the
 * reference's initial 1024-byte option buffer, ngread.go:64-66,173-191). */
typedef struct gpd_pcapng_str {
  uint64_t off;
  uint32_t len;
  uint32_t reserved;
} gpd_pcapng_str;

/* NgSectionInfo (pcapng.go:178-187) */
typedef struct gpd_pcapng_section_info {
  gpd_pcapng_str hardware, os, application, comment;
  uint32_t big_endian; /* the section's byte order */
  uint32_t reserved;
} gpd_pcapng_section_info;

/* NgInterface (pcapng.go:145-170) without its statistics */
typedef struct gpd_pcapng_iface {
  gpd_pcapng_str name, comment, description, filter, os;
  uint64_t ts_offset;     /* TimestampOffset */
  uint64_t second_mask;   /* secondMask, scaleUp, scaleDown of readInterfaceDescriptor */
  uint64_t scale_up;
  uint64_t scale_down;
  uint32_t linktype;      /* LinkType */
  uint32_t snaplen;       /* SnapLength, 0 = unlimited */
  uint32_t ts_resolution; /* TimestampResolution (0 in the file reads as 6) */
  uint32_t reserved;
} gpd_pcapng_iface;

typedef struct gpd_pcapng_reader gpd_pcapng_reader;

/* NewNgReader on buf[0:len) (kept by reference: it must outlive the reader).  opts may be NULL
 * (all zero, device walk automatic).  On a stop the call returns GPD_ERR_PCAPNG, *out is NULL and
 * *stop (may be NULL) is the GPD_PCAPNG_STOP_* code. */
int gpd_pcapng_open(const uint8_t *buf, uint64_t len, const gpd_pcapng_opts *opts,
                    gpd_pcapng_reader **out, int *stop);

/* The next max_n ReadPacketData results.  Packet i is returned as
 *   offset[i]   where its bytes start in buf (< 2^32: a packet beyond is GPD_ERR_INVALID)
 *   caplen[i]   CaptureInfo.CaptureLength      wirelen[i]  CaptureInfo.Length
 *   ts_sec[i], ts_nsec[i]  CaptureInfo.Timestamp as time.Unix(convertTime()) normalises it
 *               (0, 0 for a simple packet block, whose Timestamp is time.Time{})
 *   ifindex[i]  CaptureInfo.InterfaceIndex    linktype[i]  that interface's link type
 * (any array after caplen may be NULL).  Packets dropped for their link type are not counted.
 * At a stop, *n_out counts the packets before it and the call returns GPD_ERR_PCAPNG with the
 * reference's text, except for LIMIT and EOF (GPD_OK). */
int gpd_pcapng_index(gpd_pcapng_reader *r, uint64_t max_n, uint32_t *offset, uint32_t *caplen,
                     uint32_t *wirelen, int64_t *ts_sec, uint32_t *ts_nsec, uint32_t *ifindex,
                     uint32_t *linktype, uint64_t *n_out, int *stop);

uint32_t gpd_pcapng_linktype(const gpd_pcapng_reader *r);
uint32_t gpd_pcapng_ninterfaces(const gpd_pcapng_reader *r);
/* GPD_ERR_INVALID with "Interface %d invalid. There are only %d interfaces" when i is out of range */
int gpd_pcapng_interface(const gpd_pcapng_reader *r, int64_t i, gpd_pcapng_iface *out);
int gpd_pcapng_section(const gpd_pcapng_reader *r, gpd_pcapng_section_info *out);
/* Resolution(): *base 2 or 10 and *exponent <= 0 of interface 0; 0, 0 with want_mixed_linktype.
 * GPD_ERR_INVALID when there is no interface (the reference panics). */
int gpd_pcapng_resolution(const gpd_pcapng_reader *r, int *base, int *exponent);
/* SkipSection(): returns like gpd_pcapng_index, *stop (may be NULL) as there. */
int gpd_pcapng_skip_section(gpd_pcapng_reader *r, int *stop);
/* Where the reader stands: the next block header, or at a final stop the header of the block it
 * stopped in (len after a clean EOF). */
uint64_t gpd_pcapng_pos(const gpd_pcapng_reader *r);
void gpd_pcapng_close(gpd_pcapng_reader *r);
/* The calling thread's last stop text of this header's functions ("" when none). */
const char *gpd_pcapng_last_error(void);

/* The ReadPacketData loop feeding DecodeLayers: the next max_n packets of the reader are decoded
 * with the context's parser into `out` (host arrays of max_n entries; status and layers
 * required, ext and records not supported), as gpd_decode_pcap_at does for pcap.  Returns like
 * gpd_pcapng_index.  GPD_ERR_INVALID for a reader opened with want_mixed_linktype: a context
 * has one first layer.  The reader's buffer is the decoder's batch buffer here, so gpd.h's batch
 * contract holds for it: readable to round_up(len, 16) (packets the host walk finds travel
 * through gpd_decode_host). */
int gpd_decode_pcapng(gpd_ctx *ctx, gpd_pcapng_reader *r, uint64_t max_n, const gpd_result *out,
                      uint64_t *n_out, int *stop, int nthreads);

/* Diagnostics of this thread's last gpd_decode_pcapng call: [0] chunks walked on the device,
 * [1] whole chunks handed to the host walk, [2] tails of chunks handed to the host at a
 * state-changing block (section header, interface description, statistics), and why a chunk or
 * tail went: [3] a speculation the stitch could not correct, [4] a block the device does not
 * vouch for, [5] a block header no segment covered, [6] a walk ending short of the chunk;
 * [7] segments the stitch re-walked. */
void gpd_decode_pcapng_last_walk_counts(uint32_t *c8);

#ifdef __cplusplus
}
#endif
#endif /* GPD_PCAPNG_H_ */
