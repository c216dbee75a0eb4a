// gpd_dns_walk.h — (*DNS).DecodeFromBytes (layers/dns.go:304-392) as one walker over a message's
// bytes, plain C++17 shared by the device kernels (gpd_dns.hip), the host entry point
// gpd_dns_decode_host and the stand-alone test program (tests/c/dns_walk_host.cpp).
//
// The walker is templated on a sink.  It tells the sink every name byte and every finished
// entry; the sizing sink ignores them (the walk's counts are the result), the storing sink puts
// them into arrays whose capacities are the sizing walk's counts.  A record that fails after some
// of its name bytes were told is not committed: its bytes lie past the committed count, and the
// storing sink's bound keeps them inside the message's own share.
//
// decodeName (:538-627) recurses only as a tail: after the inner call returns, the outer one
// does `index++`, leaves its loop and returns buffer[start+1:] — and every outer level's result
// but the first's is dropped (:604).  So the walk is a loop over levels with three words of
// state: the level, the current level's start (the 255-byte test is `index2 - offset` of that
// level, :564) and the first level's end offset (index + 2 at its pointer, or index + 1 at its
// zero byte).  No stack, no array: nothing here can make a kernel use scratch memory.
//
// work (include/gpd_dns.h) is counted where the reference does the step, so the count at any
// return equals the model's (tests/dns_ref.py).  max_work 0 means no budget.
#pragma once
#include <stdint.h>

#include "../../include/gpd_dns.h"

#if defined(__HIPCC__)
#define GPD_DNS_HD __host__ __device__ __forceinline__
#else
#define GPD_DNS_HD inline
#endif

namespace gpd {

// dns.go:55-74: the types decodeRData looks at
constexpr uint32_t kDnsA = 1, kDnsNS = 2, kDnsCNAME = 5, kDnsSOA = 6, kDnsPTR = 12, kDnsHINFO = 13, kDnsMX = 15,
                   kDnsTXT = 16, kDnsAAAA = 28, kDnsSRV = 33, kDnsOPT = 41, kDnsURI = 256;

// The sizing sink.
struct DnsCountSink {
  GPD_DNS_HD void name_byte(uint32_t, uint8_t) const {}
  GPD_DNS_HD void entry(uint32_t, const gpd_dns_entry &) const {}
};

// The storing sink: entry k of the message to entries[k], name byte p to names[p], both inside
// the capacities.  name_base is added to every name_off (the message's place in names[]).
struct DnsStoreSink {
  gpd_dns_entry *entries;
  uint32_t cap_entries;
  uint8_t *names;
  uint32_t cap_names;
  uint32_t name_base;
  GPD_DNS_HD void name_byte(uint32_t p, uint8_t b) const {
    if (p < cap_names) names[p] = b;
  }
  GPD_DNS_HD void entry(uint32_t k, const gpd_dns_entry &e) const {
    if (k >= cap_entries) return;
    gpd_dns_entry x = e;
    x.name_off += name_base;
    entries[k] = x;
  }
};

struct DnsWalk {
  uint64_t work = 0, max_work = 0;  // max_work 0: unbounded
  uint32_t a0 = 0, a1 = 0;          // the error's arguments
  uint32_t n_entries = 0;           // committed
  uint32_t name_bytes = 0;          // committed
  GPD_DNS_HD bool spend(uint64_t k) {  // false: the budget is passed
    work += k;
    return max_work == 0 || work <= max_work;
  }
};

GPD_DNS_HD uint32_t dns_be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
GPD_DNS_HD uint32_t dns_be32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// decodeName(data[:len], offset, buffer, 1).  The name's bytes go to the sink from position
// `pos` on (without the leading dot); *nlen is len(name), *endp the returned offset.  Returns
// GPD_DNS_OK, an error code, or GPD_DNS_DEFERRED.
template <class Sink>
GPD_DNS_HD uint32_t dns_name(const uint8_t *d, uint32_t len, uint32_t offset, const Sink &sink, uint32_t pos,
                             DnsWalk &W, uint32_t *nlen, uint32_t *endp) {
  uint32_t level = 1, app = 0, end_first = 0;
  for (;;) {  // one decodeName call per round
    if (!W.spend(1)) return GPD_DNS_DEFERRED;
    if (level > 255u) return GPD_DNS_E_MAX_RECURSION;           // :539
    if (offset >= len) return GPD_DNS_E_NAME_OFFSET_HIGH;       // :541
    uint32_t index = offset;
    bool pointer = false;
    if (d[index] != 0) {                                        // (:548: a zero byte returns at once)
      while (d[index] != 0) {                                   // :552
        if (!W.spend(1)) return GPD_DNS_DEFERRED;
        const uint32_t b = d[index];
        const uint32_t kind = b & 0xC0u;
        if (kind == 0xC0u) {                                    // :573-609
          if (index + 2u > len) return GPD_DNS_E_POINTER_HIGH;  // :593
          const uint32_t offsetp = ((b << 8) | d[index + 1u]) & 0x3FFFu;
          if (offsetp > len) return GPD_DNS_E_POINTER_HIGH;     // :597
          if (level == 1u) end_first = index + 2u;              // index++ (:608), then index + 1 (:624,626)
          offset = offsetp;
          ++level;
          pointer = true;
          break;
        }
        if (kind == 0x40u || kind == 0x80u) {                   // :611-617
          W.a0 = b;
          W.a1 = index;
          return kind == 0x40u ? GPD_DNS_E_LABEL_40 : GPD_DNS_E_LABEL_80;
        }
        const uint32_t index2 = index + b + 1u;                 // :563
        if (index2 - offset > 255u) return GPD_DNS_E_NAME_TOO_LONG;  // :564
        if (index2 > len) return GPD_DNS_E_NAME_INVALID_INDEX;  // :566
        if (!W.spend(1u + b)) return GPD_DNS_DEFERRED;          // :569-570
        if (app) sink.name_byte(pos + app - 1u, (uint8_t)'.');
        ++app;
        for (uint32_t k = index + 1u; k < index2; ++k, ++app) sink.name_byte(pos + app - 1u, d[k]);
        index = index2;
        if (index >= len) return GPD_DNS_E_INDEX_RANGE;         // :619
      }
    }
    if (pointer) continue;  // the inner call
    if (level == 1u) end_first = index + 1u;                    // :549,624,626
    break;                  // every outer level only returns (:604-609)
  }
  *nlen = app ? app - 1u : 0u;                                  // :623-626
  *endp = end_first;
  return GPD_DNS_OK;
}

// decodeRData (:906-993) of a record with DataLength > 0; `end` is len(data[:end]) (:732), `off`
// the rdata's offset.  Names go behind the record's Name at pos.
template <class Sink>
GPD_DNS_HD uint32_t dns_rdata(const uint8_t *d, uint32_t end, uint32_t off, const Sink &sink, uint32_t pos,
                              DnsWalk &W, gpd_dns_entry &e) {
  const uint32_t type = e.type, dl = e.rdlength;
  uint32_t n1 = 0, n2 = 0, endq = 0, v;
  if (type == kDnsTXT || type == kDnsHINFO) {                   // :912-918, :864-875
    for (uint32_t index = 0; index != dl;) {
      if (!W.spend(1)) return GPD_DNS_DEFERRED;
      const uint32_t index2 = index + 1u + d[off + index];
      if (index2 > dl) return GPD_DNS_E_CHAR_STRING;
      index = index2;
    }
  } else if (type == kDnsNS || type == kDnsCNAME || type == kDnsPTR) {  // :919-936
    if ((v = dns_name(d, end, off, sink, pos, W, &n1, &endq)) != GPD_DNS_OK) return v;
  } else if (type == kDnsSOA) {                                 // :937-955
    if ((v = dns_name(d, end, off, sink, pos, W, &n1, &endq)) != GPD_DNS_OK) return v;
    if ((v = dns_name(d, end, endq, sink, pos + n1, W, &n2, &endq)) != GPD_DNS_OK) return v;
    if (end < endq + 20u) return GPD_DNS_E_SOA_SMALL;
    e.fixed_off = endq;
  } else if (type == kDnsMX) {                                  // :956-965
    if (end < off + 2u) return GPD_DNS_E_MX_SMALL;
    if ((v = dns_name(d, end, off + 2u, sink, pos, W, &n1, &endq)) != GPD_DNS_OK) return v;
  } else if (type == kDnsURI) {                                 // :966-972
    if (dl < 4u) return GPD_DNS_E_URI_SMALL;
  } else if (type == kDnsSRV) {                                 // :973-984
    if (end < off + 6u) return GPD_DNS_E_SRV_SMALL;
    if ((v = dns_name(d, end, off + 6u, sink, pos, W, &n1, &endq)) != GPD_DNS_OK) return v;
  } else if (type == kDnsOPT) {                                 // :985-990, :877-904 (offset < end here)
    if (off + 4u > end) {
      W.a0 = end - off;
      return GPD_DNS_E_OPT_SHORT;
    }
    for (uint32_t i = off; i < end;) {
      if (!W.spend(1)) return GPD_DNS_DEFERRED;
      if (end < i + 4u) {
        W.a0 = end;
        W.a1 = i + 4u;
        return GPD_DNS_E_OPT_MALFORMED;
      }
      const uint32_t l = dns_be16(d + i + 2u);
      if (i + 4u + l > end) {
        W.a0 = l;
        return GPD_DNS_E_OPT_LENGTH;
      }
      i += l + 4u;
    }
  }
  e.rname1_len = (uint16_t)n1;
  e.rname2_len = (uint16_t)n2;
  return GPD_DNS_OK;
}

// DecodeFromBytes(data[:len]).  m's packet, data_off and first_entry are the caller's; every
// other field is written.  W.n_entries / W.name_bytes are what the sink was told to keep.
template <class Sink>
GPD_DNS_HD void dns_walk(const uint8_t *d, uint32_t len, const Sink &sink, DnsWalk &W, gpd_dns_msg &m) {
  m.data_len = len;
  m.id = m.flags = m.qdcount = m.ancount = m.nscount = m.arcount = 0;
  m.n_q = m.n_an = m.n_ns = m.n_ar = 0;
  m.rcode = m.truncated = m.reserved = 0;
  m.verdict = GPD_DNS_OK;
  m.err_arg0 = m.err_arg1 = 0;
  if (len < 12u) {                                              // :307-310
    m.truncated = 1;
    m.verdict = GPD_DNS_E_TOO_SHORT;
    return;
  }
  m.id = (uint16_t)dns_be16(d);                                 // :315-327
  m.flags = (uint16_t)dns_be16(d + 2);
  m.qdcount = (uint16_t)dns_be16(d + 4);
  m.ancount = (uint16_t)dns_be16(d + 6);
  m.nscount = (uint16_t)dns_be16(d + 8);
  m.arcount = (uint16_t)dns_be16(d + 10);
  uint32_t rcode = d[3] & 0x0Fu;
  uint32_t offset = 12, verdict = GPD_DNS_OK;
  for (uint32_t sec = 0; sec < 4u; ++sec) {
    const uint32_t want = sec == 0 ? m.qdcount : sec == 1 ? m.ancount : sec == 2 ? m.nscount : m.arcount;
    uint32_t got = 0;
    for (; verdict == GPD_DNS_OK && got < want; ++got) {
      if (!W.spend(1)) {
        verdict = GPD_DNS_DEFERRED;
        break;
      }
      gpd_dns_entry e{};
      e.name_off = W.name_bytes;
      e.section = (uint8_t)sec;
      uint32_t nlen = 0, endq = 0;
      if ((verdict = dns_name(d, len, offset, sink, W.name_bytes, W, &nlen, &endq)) != GPD_DNS_OK) break;
      e.name_len = (uint16_t)nlen;
      if (sec == 0) {                                           // :636-651
        if (len < endq + 4u) {
          verdict = GPD_DNS_E_QUESTION_SMALL;
          break;
        }
        e.type = (uint16_t)dns_be16(d + endq);
        e.klass = (uint16_t)dns_be16(d + endq + 2u);
        offset = endq + 4u;
      } else {                                                  // :710-738
        if (len < endq + 10u) {
          verdict = GPD_DNS_E_RECORD_SMALL;
          break;
        }
        e.type = (uint16_t)dns_be16(d + endq);
        e.klass = (uint16_t)dns_be16(d + endq + 2u);
        e.ttl = dns_be32(d + endq + 4u);
        e.rdlength = (uint16_t)dns_be16(d + endq + 8u);
        const uint32_t end = endq + 10u + e.rdlength;
        if (end > len) {
          verdict = GPD_DNS_E_RECORD_LENGTH;
          break;
        }
        e.rdata_off = endq + 10u;
        if (e.rdlength > 0 &&
            (verdict = dns_rdata(d, end, endq + 10u, sink, W.name_bytes + nlen, W, e)) != GPD_DNS_OK)
          break;
        offset = end;
        if (sec == 3 && e.type == kDnsOPT) rcode = (rcode | ((e.ttl >> 20) & 0xF0u)) & 0xFFu;  // :377-379
      }
      sink.entry(W.n_entries, e);
      ++W.n_entries;
      W.name_bytes += (uint32_t)e.name_len + e.rname1_len + e.rname2_len;
    }
    if (sec == 0) m.n_q = (uint16_t)got;
    else if (sec == 1) m.n_an = (uint16_t)got;
    else if (sec == 2) m.n_ns = (uint16_t)got;
    else m.n_ar = (uint16_t)got;
  }
  m.verdict = (uint8_t)verdict;
  m.rcode = (uint8_t)rcode;
  if (verdict == GPD_DNS_DEFERRED) {  // no entries, no names; the header as read
    m.rcode = (uint8_t)(d[3] & 0x0Fu);
    m.n_q = m.n_an = m.n_ns = m.n_ar = 0;
    W.n_entries = W.name_bytes = 0;
    return;
  }
  m.err_arg0 = W.a0;
  m.err_arg1 = W.a1;
}

}  // namespace gpd
