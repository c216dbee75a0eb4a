// gpd_tls_walk.h — (*TLS).DecodeFromBytes (layers/tls.go:118-194) as one walker over a message's
// bytes, plain C++17 shared by the device kernels (gpd_tls.hip), the host entry point
// gpd_tls_decode_host and the stand-alone test program (tests/c/tls_walk_host.cpp).
//
// decodeTLSRecords (:130-194) calls itself only as its last statement (:193), on data[tl:], so the
// walk is a loop over record headers with one offset as its state.  One round is one invocation:
// the tests come in the reference's order (too short, the content type, the length, the per-type
// rule), and `work` (include/gpd_tls.h) is the number of rounds begun.
//
// The walker is templated on a sink that is told every appended record; the sizing sink ignores
// them (the walk's count is the result), the storing sink puts them into an array whose capacity
// is the sizing walk's count.  The four list lengths are four words, not an array: nothing here
// can make a kernel use scratch memory.  Every byte is read as a byte, at an offset below len.
#pragma once
#include <stdint.h>

#include "../../include/gpd_tls.h"

#if defined(__HIPCC__)
#define GPD_TLS_HD __host__ __device__ __forceinline__
#else
#define GPD_TLS_HD inline
#endif

namespace gpd {

// The sizing sink.
struct TlsCountSink {
  GPD_TLS_HD void rec(uint32_t, const gpd_tls_rec &) const {}
};

// The storing sink: record k of the message to recs[k], inside the capacity, as one 16-byte store
// (recs is 16-byte aligned).
struct TlsStoreSink {
  gpd_tls_rec *recs;
  uint32_t cap;
  GPD_TLS_HD void rec(uint32_t k, const gpd_tls_rec &r) const {
    if (k >= cap) return;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    v4 x;
    __builtin_memcpy(&x, &r, 16);
    *reinterpret_cast<v4 *>(recs + k) = x;
#else
    recs[k] = r;
#endif
  }
};

struct TlsWalk {
  uint64_t work = 0, max_records = 0;  // max_records 0: unbounded
  uint32_t n_records = 0;              // appended
};

// The record of a message that is the host's: no entries, n_* zero, contents_off and err_off zero.
GPD_TLS_HD void tls_deferred(uint32_t len, TlsWalk &W, gpd_tls_msg &m) {
  m = gpd_tls_msg{};
  m.data_len = len;
  m.verdict = (uint8_t)GPD_TLS_DEFERRED;
  W.n_records = 0;
}

// t.DecodeFromBytes(data[:len]).  m.packet, data_off and first_record are left zero.
template <class Sink>
GPD_TLS_HD void tls_walk(const uint8_t *d, uint32_t len, const Sink &sink, TlsWalk &W, gpd_tls_msg &m) {
  m = gpd_tls_msg{};
  m.data_len = len;
  uint32_t off = 0, contents = 0;                                // :119 Contents = data
  uint32_t n_ccs = 0, n_hs = 0, n_app = 0, n_alert = 0;          // :122-125
  uint32_t verdict = GPD_TLS_OK, truncated = 0;
  for (;;) {  // one decodeTLSRecords(data[off:]) per round
    if (++W.work > W.max_records && W.max_records != 0) {
      tls_deferred(len, W, m);
      return;
    }
    const uint32_t rem = len - off;
    if (rem < 5u) {                                              // :131-134
      truncated = 1;
      verdict = GPD_TLS_E_TOO_SHORT;
      break;
    }
    contents = off;                                              // :139
    const uint8_t *h = d + off;
    const uint32_t ct = h[0];                                    // :142-144
    const uint32_t version = ((uint32_t)h[1] << 8) | h[2];
    const uint32_t length = ((uint32_t)h[3] << 8) | h[4];
    if (ct < GPD_TLS_CHANGE_CIPHER_SPEC || ct > GPD_TLS_APPLICATION_DATA) {  // :146-148
      verdict = GPD_TLS_E_UNKNOWN_TYPE;
      break;
    }
    const uint32_t tl = 5u + length;                             // :150-155
    if (rem < tl) {
      truncated = 1;
      verdict = GPD_TLS_E_LENGTH_MISMATCH;
      break;
    }
    gpd_tls_rec r{};
    r.off = off;
    r.version = (uint16_t)version;
    r.length = (uint16_t)length;
    r.content_type = (uint8_t)ct;
    if (ct == GPD_TLS_CHANGE_CIPHER_SPEC) {                      // tls_cipherspec.go:43-51
      if (length != 1u) {
        truncated = 1;
        verdict = GPD_TLS_E_CCS_LENGTH;
        break;
      }
      r.a = h[5] == 1u ? (uint8_t)1 : (uint8_t)255;
      r.index_in_kind = n_ccs++;
    } else if (ct == GPD_TLS_ALERT) {                            // tls_alert.go:80-92
      if (length < 2u) {
        truncated = 1;
        verdict = GPD_TLS_E_ALERT_SHORT;
        break;
      }
      if (length == 2u) {
        r.a = h[5];
        r.b = h[6];
      } else {
        r.a = r.b = 255;
        r.flags = (uint8_t)GPD_TLS_REC_ENCRYPTED;
      }
      r.index_in_kind = n_alert++;
    } else if (ct == GPD_TLS_HANDSHAKE) {                        // tls_handshake.go:19-28: the header only
      r.index_in_kind = n_hs++;
    } else {                                                     // tls_appdata.go:28-30 cannot fail:
      r.index_in_kind = n_app++;                                 // data[hl:tl] has Length bytes
    }
    sink.rec(W.n_records, r);
    ++W.n_records;
    off += tl;
    if (rem == tl) break;                                        // :190-192
  }
  m.n_ccs = n_ccs;
  m.n_handshake = n_hs;
  m.n_appdata = n_app;
  m.n_alert = n_alert;
  m.contents_off = contents;
  m.err_off = off;  // GPD_TLS_OK: len
  m.verdict = (uint8_t)verdict;
  m.truncated = (uint8_t)truncated;
}

}  // namespace gpd
