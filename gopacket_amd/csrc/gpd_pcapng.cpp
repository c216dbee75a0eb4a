// gpd_pcapng.cpp — the pcapng block walk on the host, host side of include/gpd_pcapng.h.
//
// A sequential restatement of pcapgo's NgReader on an in-memory capture (paths relative to
// google/gopacket), function by function:
//   readBytes / Discard ........ pcapgo/ngread.go:89-99   (any short read is io.EOF)
//   readBlock .................. pcapgo/ngread.go:127-152
//   readOption ................. pcapgo/ngread.go:155-193
//   readSectionHeader .......... pcapgo/ngread.go:197-269
//   skipSection / SkipSection .. pcapgo/ngread.go:272-292
//   firstInterface ............. pcapgo/ngread.go:295-322
//   readInterfaceDescriptor .... pcapgo/ngread.go:325-386
//   convertTime ................ pcapgo/ngread.go:389-392  (+ time.Unix's normalisation)
//   readInterfaceStatistics .... pcapgo/ngread.go:395-438
//   readPacketHeader ........... pcapgo/ngread.go:443-525
//   ReadPacketData ............. pcapgo/ngread.go:529-545
// The stream is the buffer and a position; instead of copying a packet out, the walk returns
// where its bytes lie.  All block arithmetic is the reference's wrapping uint32 / uint16 /
// uint64 arithmetic.  Two things differ by decision (include/gpd_pcapng.h): where the reference
// panics, and where an option value is shorter than the reference indexes it (it then reads
// stale bytes of its reused option buffer, or panics), the reader stops with STOP_PANIC.
//
// This file includes no HIP header: tests/c/ng_walk_host.c links it alone under
// -fsanitize=address,undefined (-DGPD_PCAPNG_STANDALONE drops the call into the runtime's
// gpd_last_error_string text).
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "gpd_pcapng_internal.h"

#ifndef GPD_PCAPNG_STANDALONE
namespace gpd {
int set_error(int code, const char *fmt, ...);
}
#endif

namespace {

using Reader = gpd_pcapng_reader;

thread_local std::string g_ng_err;

int publish(int code, const std::string &text) {
  g_ng_err = text;
#ifndef GPD_PCAPNG_STANDALONE
  return gpd::set_error(code, "%s", text.c_str());
#else
  return code;
#endif
}

int fail(Reader &r, int stop, const char *fmt, ...) {
  char b[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  r.stop = stop;
  r.err = b;
  return stop;
}

inline uint32_t get32(const Reader &r, uint64_t at) {
  uint32_t v;
  std::memcpy(&v, r.buf + at, 4);
  return r.big_endian ? __builtin_bswap32(v) : v;
}
inline uint16_t get16(const Reader &r, uint64_t at) {
  uint16_t v;
  std::memcpy(&v, r.buf + at, 2);
  return r.big_endian ? (uint16_t)__builtin_bswap16(v) : v;
}
inline uint64_t get64(const Reader &r, uint64_t at) {
  uint64_t v;
  std::memcpy(&v, r.buf + at, 8);
  return r.big_endian ? __builtin_bswap64(v) : v;
}

// readBytes (ngread.go:89-99): n bytes at *at, or io.EOF with the stream drained.
int rd(Reader &r, uint64_t n, uint64_t *at) {
  if (r.len - r.pos < n) {
    r.pos = r.len;
    return fail(r, GPD_PCAPNG_STOP_EOF_BLOCK, "EOF");
  }
  *at = r.pos;
  r.pos += n;
  return 0;
}

// bufio.Reader.Discard: ErrNegativeCount, nothing for 0, io.EOF when short.
int discard(Reader &r, int64_t n) {
  if (n < 0) return fail(r, GPD_PCAPNG_STOP_NEGATIVE, "bufio: negative count");
  uint64_t at;
  return n ? rd(r, (uint64_t)n, &at) : 0;
}

int read_block(Reader &r) {  // ngread.go:127-152
  r.blk_pos = r.pos;
  if (r.pos == r.len) return fail(r, GPD_PCAPNG_STOP_EOF, "EOF");
  uint64_t at, bo;
  if (rd(r, 8, &at)) return r.stop;
  r.blk_type = get32(r, at);
  if (r.blk_type == GPD_PCAPNG_BLOCK_SECTION) {
    if (rd(r, 4, &bo)) return r.stop;
    uint32_t v;
    std::memcpy(&v, r.buf + bo, 4);
    if (__builtin_bswap32(v) == GPD_PCAPNG_BYTE_ORDER)  // (little-endian host: bswap = big-endian read)
      r.big_endian = true;
    else if (v == GPD_PCAPNG_BYTE_ORDER)
      r.big_endian = false;
    else
      return fail(r, GPD_PCAPNG_STOP_BYTE_ORDER, "Wrong byte order value in Section Header");
    r.blk_len = get32(r, at + 4) - 8u - 4u;
    return 0;
  }
  r.blk_len = get32(r, at + 4) - 8u;
  return 0;
}

// readOption (ngread.go:155-193).  *olen: the option's own length field (0 keeps the previous
// option's value in opt_val, as the reference's reused buffer does).
int read_option(Reader &r, uint16_t *olen) {
  *olen = 0;
  if (r.blk_len == 4) {
    r.opt_code = 0;
    return 0;
  }
  uint64_t at;
  if (rd(r, 4, &at)) return r.stop;
  r.blk_len -= 4;
  r.opt_code = get16(r, at);
  const uint16_t length = get16(r, at + 2);
  *olen = length;
  if (r.opt_code == 0) {
    if (length != 0) return fail(r, GPD_PCAPNG_STOP_OPT_END, "End of Options must be zero length");
    return 0;
  }
  if (length != 0) {
    uint64_t v;
    if (rd(r, length, &v)) return r.stop;
    r.opt_val = gpd_pcapng_str{v, length, 0};
    uint16_t padding = length % 4;
    if (padding > 0) {
      padding = 4 - padding;
      if (discard(r, padding)) return r.stop;
    }
    r.blk_len -= (uint32_t)(uint16_t)(length + padding);  // uint16 sum: 65535 + 1 wraps to 0
  }
  return 0;
}

int panic_short(Reader &r, const char *what, unsigned need, unsigned have) {
  return fail(r, GPD_PCAPNG_STOP_PANIC, "the reference panics here: %s option of %u bytes read as %u", what, have,
              need);
}

int read_interface(Reader &r) {  // readInterfaceDescriptor, ngread.go:325-386
  uint64_t at;
  if (rd(r, 8, &at)) return r.stop;
  r.blk_len -= 8;
  gpd_pcapng_iface f{};
  f.linktype = get16(r, at);
  f.snaplen = get32(r, at + 4);
  for (;;) {
    uint16_t ol;
    if (read_option(r, &ol)) return r.stop;
    const gpd_pcapng_str &v = r.opt_val;
    if (r.opt_code == 0) break;
    switch (r.opt_code) {
      case 2: f.name = v; break;
      case 1: f.comment = v; break;
      case 3: f.description = v; break;
      case 11:  // value[1:]: the filter type byte is dropped
        if (ol < 1) return panic_short(r, "if_filter", 1, ol);
        f.filter = gpd_pcapng_str{v.off + 1, v.len - 1, 0};
        break;
      case 12: f.os = v; break;
      case 14:
        if (ol < 8) return panic_short(r, "if_tsoffset", 8, ol);
        f.ts_offset = get64(r, v.off);
        break;
      case 9:
        if (ol < 1) return panic_short(r, "if_tsresol", 1, ol);
        f.ts_resolution = r.buf[v.off];
        break;
    }
  }
  if (discard(r, (int64_t)r.blk_len)) return r.stop;
  if (f.ts_resolution == 0) f.ts_resolution = 6;
  const uint32_t e = f.ts_resolution & 0x7f;
  if (f.ts_resolution & 0x80) {
    f.second_mask = e >= 64 ? 0 : 1ull << e;  // Go: a shift by 64 or more gives 0
  } else {
    f.second_mask = 1;
    for (uint32_t j = 0; j < e; j++) f.second_mask *= 10;  // wraps
  }
  f.scale_up = f.scale_down = 1;
  if (f.second_mask < 1000000000ull) {
    if (f.second_mask == 0)
      return fail(r, GPD_PCAPNG_STOP_PANIC,
                  "the reference panics here: integer divide by zero (timestamp resolution %u)", f.ts_resolution);
    f.scale_up = 1000000000ull / f.second_mask;
  } else {
    f.scale_down = f.second_mask / 1000000000ull;
  }
  r.ifaces.push_back(f);
  return 0;
}

// convertTime (ngread.go:389-392) and time.Unix's normalisation of the nanoseconds.
void convert_time(const gpd_pcapng_iface &f, uint64_t ts, int64_t *sec, uint32_t *nsec) {
  uint64_t s = ts / f.second_mask + f.ts_offset;  // second_mask != 0 (read_interface)
  int64_t n = (int64_t)(ts % f.second_mask * f.scale_up / f.scale_down);
  if (n < 0 || n >= 1000000000ll) {
    const int64_t q = n / 1000000000ll;
    s += (uint64_t)q;
    n -= q * 1000000000ll;
    if (n < 0) {
      n += 1000000000ll;
      s--;
    }
  }
  *sec = (int64_t)s;
  *nsec = (uint32_t)n;
}

int read_statistics(Reader &r) {  // readInterfaceStatistics, ngread.go:395-438 (values dropped)
  uint64_t at;
  if (rd(r, 12, &at)) return r.stop;
  r.blk_len -= 12;
  const uint32_t id = get32(r, at);
  if (id >= r.ifaces.size())
    return fail(r, GPD_PCAPNG_STOP_IFACE_ID, "Interface id %u not present in section (have only %u interfaces)", id,
                (unsigned)r.ifaces.size());
  for (;;) {
    uint16_t ol;
    if (read_option(r, &ol)) return r.stop;
    if (r.opt_code == 0) break;
    if (r.opt_code >= 2 && r.opt_code <= 5 && ol < 8) return panic_short(r, "statistics", 8, ol);
  }
  return discard(r, (int64_t)r.blk_len);
}

int skip_blocks(Reader &r) {  // skipSection, ngread.go:272-284
  for (;;) {
    if (read_block(r)) return r.stop;
    if (r.blk_type == GPD_PCAPNG_BLOCK_SECTION) return 0;
    if (discard(r, (int64_t)r.blk_len)) return r.stop;
  }
}

int first_interface(Reader &r) {  // ngread.go:295-322
  for (;;) {
    if (read_block(r)) return r.stop;
    switch (r.blk_type) {
      case GPD_PCAPNG_BLOCK_INTERFACE:
        if (read_interface(r)) return r.stop;
        if (!r.first_found) {
          r.linktype = r.ifaces[0].linktype;
          r.first_found = true;
        } else if (r.linktype != r.ifaces[0].linktype) {
          if (r.opts.error_on_mismatching_linktype)
            return fail(r, GPD_PCAPNG_STOP_LINKTYPE, "Link type of current interface is different from first one");
          continue;
        }
        return 0;
      case GPD_PCAPNG_BLOCK_PACKET:
      case GPD_PCAPNG_BLOCK_ENHANCED:
      case GPD_PCAPNG_BLOCK_SIMPLE:
      case GPD_PCAPNG_BLOCK_STATS:
        return fail(r, GPD_PCAPNG_STOP_NO_FIRST, "A section must have an interface before a packet block");
    }
    if (discard(r, (int64_t)r.blk_len)) return r.stop;
  }
}

int read_section(Reader &r) {  // readSectionHeader, ngread.go:197-269
  r.ifaces.clear();
  uint64_t at;
  for (;;) {
    if (rd(r, 12, &at)) return r.stop;
    r.blk_len -= 12;
    if (get16(r, at) == 1 && get16(r, at + 2) == 0) break;
    if (!r.opts.skip_unknown_version)
      return fail(r, GPD_PCAPNG_STOP_VERSION, "Unknown pcapng Version in Section Header");
    if (discard(r, (int64_t)r.blk_len)) return r.stop;
    if (skip_blocks(r)) return r.stop;
  }
  gpd_pcapng_section_info s{};
  for (;;) {
    uint16_t ol;
    if (read_option(r, &ol)) return r.stop;
    if (r.opt_code == 0) break;
    switch (r.opt_code) {
      case 1: s.comment = r.opt_val; break;
      case 2: s.hardware = r.opt_val; break;
      case 3: s.os = r.opt_val; break;
      case 4: s.application = r.opt_val; break;
    }
  }
  if (discard(r, (int64_t)r.blk_len)) return r.stop;
  s.big_endian = r.big_endian;
  r.section = s;
  if (!r.opts.want_mixed_linktype) return first_interface(r);
  return 0;
}

int iface_missing(Reader &r, uint32_t id) {
  return fail(r, GPD_PCAPNG_STOP_IFACE_ID, "Interface id %u not present in section (have only %u interfaces)", id,
              (unsigned)r.ifaces.size());
}

}  // namespace

int gpd_pcapng_reader::open() {
  Reader &r = *this;
  if (read_block(r)) return r.stop;
  if (r.blk_type != GPD_PCAPNG_BLOCK_SECTION) return fail(r, GPD_PCAPNG_STOP_MAGIC, "Unknown magic %x", r.blk_type);
  return read_section(r);
}

int gpd_pcapng_reader::skip_section() {
  Reader &r = *this;
  if (r.stop) return r.stop;
  if (skip_blocks(r)) return r.stop;
  return read_section(r);
}

int gpd_pcapng_reader::absorb_state_blocks() {
  Reader &r = *this;
  while (!r.stop) {
    if (r.len - r.pos < 8) break;
    const uint32_t type = get32(r, r.pos);
    if (type != GPD_PCAPNG_BLOCK_SECTION && type != GPD_PCAPNG_BLOCK_INTERFACE && type != GPD_PCAPNG_BLOCK_STATS)
      break;
    if (read_block(r)) break;
    if (r.blk_type == GPD_PCAPNG_BLOCK_INTERFACE)
      read_interface(r);
    else if (r.blk_type == GPD_PCAPNG_BLOCK_STATS)
      read_statistics(r);
    else
      read_section(r);
  }
  return r.stop;
}

int gpd_pcapng_reader::result(int stop_code) const {
  if (stop_code == GPD_PCAPNG_STOP_LIMIT || stop_code == GPD_PCAPNG_STOP_EOF) {
    g_ng_err.clear();
    return GPD_OK;
  }
  return publish(GPD_ERR_PCAPNG, err);
}

int gpd_pcapng_reader::next_packet(gpd::NgPacket *p) {  // readPacketHeader + ReadPacketData
  Reader &r = *this;
  if (r.stop) return r.stop;
  for (;;) {
    uint64_t at;
    bool found = false;
    while (!found) {
      if (read_block(r)) return r.stop;
      switch (r.blk_type) {
        case GPD_PCAPNG_BLOCK_ENHANCED:
        case GPD_PCAPNG_BLOCK_PACKET: {
          if (rd(r, 20, &at)) return r.stop;
          r.blk_len -= 20;
          p->ifindex = r.blk_type == GPD_PCAPNG_BLOCK_ENHANCED ? get32(r, at) : get16(r, at);
          if (p->ifindex >= r.ifaces.size()) return iface_missing(r, p->ifindex);
          convert_time(r.ifaces[p->ifindex], (uint64_t)get32(r, at + 4) << 32 | get32(r, at + 8), &p->ts_sec,
                       &p->ts_nsec);
          p->caplen = get32(r, at + 12);
          p->wirelen = get32(r, at + 16);
          found = true;
          break;
        }
        case GPD_PCAPNG_BLOCK_SIMPLE:
          if (rd(r, 4, &at)) return r.stop;
          r.blk_len -= 4;
          p->ts_sec = 0;
          p->ts_nsec = 0;
          p->ifindex = 0;
          p->wirelen = p->caplen = get32(r, at);
          if (r.ifaces.empty())
            return fail(r, GPD_PCAPNG_STOP_NO_IFACE, "At least one Interface is needed for a packet");
          if (r.ifaces[0].snaplen != 0 && p->caplen > r.ifaces[0].snaplen) p->caplen = r.ifaces[0].snaplen;
          found = true;
          break;
        case GPD_PCAPNG_BLOCK_INTERFACE:
          if (read_interface(r)) return r.stop;
          break;
        case GPD_PCAPNG_BLOCK_STATS:
          if (read_statistics(r)) return r.stop;
          break;
        case GPD_PCAPNG_BLOCK_SECTION:
          if (read_section(r)) return r.stop;
          break;
        default:
          if (discard(r, (int64_t)r.blk_len)) return r.stop;
      }
    }
    p->linktype = r.ifaces[p->ifindex].linktype;
    if (!r.opts.want_mixed_linktype && p->linktype != r.linktype) {
      if (discard(r, (int64_t)r.blk_len)) return r.stop;
      if (r.opts.error_on_mismatching_linktype)
        return fail(r, GPD_PCAPNG_STOP_LINKTYPE, "Link type of current interface is different from first one");
      continue;
    }
    break;
  }
  if (rd(r, p->caplen, &p->off)) return r.stop;
  return discard(r, (int64_t)r.blk_len - (int64_t)p->caplen);
}

extern "C" {

const char *gpd_pcapng_last_error(void) { return g_ng_err.c_str(); }

int gpd_pcapng_open(const uint8_t *buf, uint64_t len, const gpd_pcapng_opts *opts, gpd_pcapng_reader **out,
                    int *stop) {
  if (stop) *stop = 0;
  if (!out || (!buf && len)) return publish(GPD_ERR_INVALID, "gpd_pcapng_open: null argument");
  *out = nullptr;
  gpd_pcapng_opts o{};
  o.device_walk = -1;
  if (opts) o = *opts;
  if (o.chunk_bytes && (o.chunk_bytes % 2048 || o.chunk_bytes < 4096 || o.chunk_bytes > (64ull << 20)))
    return publish(GPD_ERR_INVALID, "gpd_pcapng_open: chunk_bytes must be a multiple of 2048 in [4096, 64 MiB]");
  gpd_pcapng_reader *r = new gpd_pcapng_reader;
  r->buf = buf;
  r->len = len;
  r->opts = o;
  if (r->open()) {
    if (stop) *stop = r->stop;
    const std::string text = r->err;
    delete r;
    return publish(GPD_ERR_PCAPNG, text);
  }
  g_ng_err.clear();
  *out = r;
  return GPD_OK;
}

int gpd_pcapng_index(gpd_pcapng_reader *r, uint64_t max_n, uint32_t *offset, uint32_t *caplen, uint32_t *wirelen,
                     int64_t *ts_sec, uint32_t *ts_nsec, uint32_t *ifindex, uint32_t *linktype, uint64_t *n_out,
                     int *stop) {
  if (!r || !n_out || (max_n && (!offset || !caplen))) return publish(GPD_ERR_INVALID, "gpd_pcapng_index: null argument");
  uint64_t n = 0;
  int s = GPD_PCAPNG_STOP_LIMIT;
  while (n < max_n) {
    gpd::NgPacket p;
    if ((s = r->next_packet(&p))) break;
    if (p.off >= (1ull << 32)) {
      r->stop = GPD_PCAPNG_STOP_PANIC;
      r->err = "gpd_pcapng_index: packet offsets beyond 4 GiB";
      *n_out = n;
      if (stop) *stop = r->stop;
      return publish(GPD_ERR_INVALID, r->err);
    }
    offset[n] = (uint32_t)p.off;
    caplen[n] = p.caplen;
    if (wirelen) wirelen[n] = p.wirelen;
    if (ts_sec) ts_sec[n] = p.ts_sec;
    if (ts_nsec) ts_nsec[n] = p.ts_nsec;
    if (ifindex) ifindex[n] = p.ifindex;
    if (linktype) linktype[n] = p.linktype;
    n++;
  }
  *n_out = n;
  if (stop) *stop = s;
  return r->result(s);
}

uint32_t gpd_pcapng_linktype(const gpd_pcapng_reader *r) { return r ? r->linktype : 0; }
uint32_t gpd_pcapng_ninterfaces(const gpd_pcapng_reader *r) { return r ? (uint32_t)r->ifaces.size() : 0; }

int gpd_pcapng_interface(const gpd_pcapng_reader *r, int64_t i, gpd_pcapng_iface *out) {
  if (!r || !out) return publish(GPD_ERR_INVALID, "gpd_pcapng_interface: null argument");
  if (i < 0 || (uint64_t)i >= r->ifaces.size()) {
    char b[96];
    snprintf(b, sizeof b, "Interface %lld invalid. There are only %u interfaces", (long long)i,
             (unsigned)r->ifaces.size());
    return publish(GPD_ERR_INVALID, b);
  }
  *out = r->ifaces[(size_t)i];
  return GPD_OK;
}

int gpd_pcapng_section(const gpd_pcapng_reader *r, gpd_pcapng_section_info *out) {
  if (!r || !out) return publish(GPD_ERR_INVALID, "gpd_pcapng_section: null argument");
  *out = r->section;
  return GPD_OK;
}

int gpd_pcapng_resolution(const gpd_pcapng_reader *r, int *base, int *exponent) {
  if (!r || !base || !exponent) return publish(GPD_ERR_INVALID, "gpd_pcapng_resolution: null argument");
  *base = *exponent = 0;
  if (r->opts.want_mixed_linktype) return GPD_OK;
  if (r->ifaces.empty()) return publish(GPD_ERR_INVALID, "gpd_pcapng_resolution: no interface (the reference panics)");
  *base = r->ifaces[0].ts_resolution & 0x80 ? 2 : 10;
  *exponent = -(int)(r->ifaces[0].ts_resolution & 0x7f);
  return GPD_OK;
}

int gpd_pcapng_skip_section(gpd_pcapng_reader *r, int *stop) {
  if (!r) return publish(GPD_ERR_INVALID, "gpd_pcapng_skip_section: null argument");
  const int s = r->skip_section();
  if (stop) *stop = s;
  if (s == 0) {
    g_ng_err.clear();
    return GPD_OK;
  }
  return publish(GPD_ERR_PCAPNG, r->err);
}

uint64_t gpd_pcapng_pos(const gpd_pcapng_reader *r) { return !r ? 0 : r->stop ? r->blk_pos : r->pos; }

void gpd_pcapng_close(gpd_pcapng_reader *r) { delete r; }

}  // extern "C"
