// gpd_tcpasm_walk.h — the stateful assembler's state machine for one connection
// (include/gpd_tcpasm.h), as __host__ __device__ code: gpd_tcpasm.hip runs it on lane 0 of an
// item's wave, and a host program (tests/c/tcpasm_walk_host.cpp) runs the same code over
// generated connections cut into several runs, under the sanitizers.
//
// It is gpd_tcpstream_walk.h's machine (whose Sequence.Difference and page count it calls) with
// what outliving a batch needs: a page carries its Seen and where its bytes lie (the batch, or
// the object's byte store for a page carried from an earlier run), the connection carries
// lastSeen (tcpassembly/assembly.go:564-566) and the bytes it buffers, and the end of a run is
// FlushWithOptions (:235-266) and FlushAll (:276-287) instead of a drain.
#pragma once
#include <stdint.h>

#include "../../include/gpd_tcpasm.h"
#include "gpd_tcpstream_walk.h"

namespace gpd {

// One page of the out-of-order list while a run walks it (48 B).  Node ids are local to the
// item's region: the carried pages first, in list order, then the pages of the run's segments.
struct TamNode {
  uint32_t prev, next;  // kTsmNil
  uint32_t seq;
  uint32_t packet;      // the packet its bytes lie in; GPD_TCP_NO_PACKET: the old byte store
  uint32_t off, len;    // packet bytes [off, off + len), or old store bytes [off, off + len)
  uint32_t end;         // page.End (:754)
  uint32_t pad;
  uint64_t seen;        // page.Seen (:741)
  uint64_t pad2;
};

// One page between runs (32 B), a connection's pages consecutive and in list order.
struct TamCarried {
  uint32_t seq, len;
  uint32_t end;
  uint32_t off;   // its bytes: store[off, off + len)
  uint64_t seen;
  uint64_t pad;
};

struct TamConn {
  uint32_t exists;      // in the pool
  uint32_t valid;       // nextSeq != invalidSequence
  uint32_t next_seq;
  uint32_t first, last; // the page list, kTsmNil when empty
  uint32_t pages;       // conn.pages
  uint32_t page_bytes;  // bytes the list holds
  uint64_t last_seen;   // conn.lastSeen
  uint32_t nrec, ncalls, completed;
  uint32_t nbytes;      // bytes delivered by this run so far
  uint32_t cur_flags;   // GPD_TCP_R_FLUSHED while steps 2 and 3 run
  uint32_t last_end;    // End of the last record appended to the call under construction
};

struct TamIo {
  TamNode *nodes;         // the item's node region
  gpd_tcp_reasm *recs;    // the item's private records
  uint64_t *seen;         // ... their Seen
  uint32_t *src;          // ... where their bytes start, in the batch's data or in the old store
  uint32_t cap;           // the region's size: carried pages plus the pages of the run's segments
  uint32_t max_pages;     // MaxBufferedPagesPerConnection
  const uint32_t *offset; // the batch's packet offsets
  uint32_t n;             // ... and how many there are
};

// Where packet `packet` starts in the batch's data (a packet outside the batch: nowhere, its
// bytes read as zeros).
GPD_TSM_HD uint32_t tam_packet_base(const TamIo &io, uint32_t packet) {
  return packet < io.n ? io.offset[packet] : 0xFFFFFFF0u;
}

GPD_TSM_HD void tam_conn_init(TamConn &c) {
  c.exists = c.valid = 0;
  c.next_seq = 0;
  c.first = c.last = kTsmNil;
  c.pages = c.page_bytes = 0;
  c.last_seen = 0;
  c.nrec = c.ncalls = c.completed = 0;
  c.nbytes = 0;
  c.cur_flags = 0;
  c.last_end = 0;
}

// The carried connection; its cp carried pages are nodes 0 .. cp - 1 of the region.
GPD_TSM_HD void tam_conn_load(TamConn &c, const gpd_tcp_conn_info &ci) {
  tam_conn_init(c);
  if (!(ci.flags & GPD_TCP_CONN_OPEN)) return;
  c.exists = 1;
  c.valid = (ci.flags & GPD_TCP_CONN_NOSEQ) ? 0u : 1u;
  c.next_seq = c.valid ? ci.next_seq : 0u;
  c.pages = ci.pages;
  c.page_bytes = ci.page_bytes;
  c.last_seen = ci.last_seen_ns;
  if (ci.pages) {
    c.first = 0;
    c.last = ci.pages - 1u;
  }
}

GPD_TSM_HD TamNode tam_node_of(const TamCarried &p, uint32_t j, uint32_t cp) {
  TamNode n;
  n.prev = j ? j - 1u : kTsmNil;
  n.next = j + 1u < cp ? j + 1u : kTsmNil;
  n.seq = p.seq;
  n.packet = GPD_TCP_NO_PACKET;
  n.off = p.off;
  n.len = p.len;
  n.end = p.end;
  n.pad = 0;
  n.seen = p.seen;
  n.pad2 = 0;
  return n;
}

GPD_TSM_HD gpd_tcp_conn_info tam_conn_info(const TamConn &c) {
  gpd_tcp_conn_info ci;
  ci.next_seq = (c.exists && c.valid) ? c.next_seq : 0u;
  ci.flags = c.exists ? (GPD_TCP_CONN_OPEN | (c.valid ? 0u : GPD_TCP_CONN_NOSEQ)) : 0u;
  ci.pages = c.exists ? c.pages : 0u;
  ci.page_bytes = c.exists ? c.page_bytes : 0u;
  ci.last_seen_ns = c.exists ? c.last_seen : 0ull;
  return ci;
}

// One record appended to the call under construction; src: where Bytes[0] lies.
GPD_TSM_HD void tam_emit(TamConn &c, const TamIo &io, uint32_t packet, uint32_t src_off, uint32_t src, uint32_t len,
                         int32_t skip, uint32_t flags, uint64_t seen) {
  c.last_end = (flags & GPD_TCP_R_END) ? 1u : 0u;
  if (c.nrec >= io.cap) return;  // (cannot happen: a page or a segment gives one record at most)
  gpd_tcp_reasm r;
  r.packet = packet;
  r.src_off = (len && packet != GPD_TCP_NO_PACKET) ? src_off : 0u;  // (no Bytes[0]: zero)
  r.len = len;
  r.skip = skip;
  r.stream_off = c.nbytes;
  r.call = c.ncalls;
  r.flags = (uint16_t)(flags | c.cur_flags | (packet == GPD_TCP_NO_PACKET ? GPD_TCP_R_CARRIED : 0u));
  r.reserved = 0;
  io.recs[c.nrec] = r;
  io.seen[c.nrec] = seen;
  io.src[c.nrec] = len ? src : 0u;
  c.nrec += 1;
  c.nbytes += len;
}

// byteSpan (:609-620), as tsm_byte_span.
GPD_TSM_HD uint32_t tam_byte_span(TamConn &c, uint32_t seq, uint32_t len) {
  if (!c.valid) {
    c.next_seq = seq + len;
    c.valid = 1;
    return 0;
  }
  const int64_t span = tsm_diff(seq, c.next_seq);
  if (span <= 0) {
    c.next_seq = seq + len;
    return 0;
  }
  if ((int64_t)len < span) return len;  // nextSeq stays
  c.next_seq = c.next_seq + (len - (uint32_t)span);
  return (uint32_t)span;
}

// closeConnection (:666-676).
GPD_TSM_HD void tam_close(TamConn &c) {
  c.completed += 1;
  c.exists = c.valid = 0;
  c.next_seq = 0;
  c.first = c.last = kTsmNil;
  c.pages = c.page_bytes = 0;
  c.last_seen = 0;
}

// addNextFromConn (:760-780).
GPD_TSM_HD void tam_add_next(TamConn &c, const TamIo &io) {
  const TamNode f = io.nodes[c.first];
  int32_t skip = 0;
  if (!c.valid) {
    skip = -1;
  } else {
    const int64_t d = tsm_diff(c.next_seq, f.seq);
    if (d > 0) skip = d > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)d;  // (Skip is an int: saturated to 32 bits)
  }
  const uint32_t trim = tam_byte_span(c, f.seq, f.len);
  const uint32_t base = f.packet == GPD_TCP_NO_PACKET ? 0u : tam_packet_base(io, f.packet);
  tam_emit(c, io, f.packet, f.off + trim, base + f.off + trim, f.len - trim, skip, f.end ? GPD_TCP_R_END : 0u, f.seen);
  if (c.first == c.last || f.next == kTsmNil) {
    c.first = c.last = kTsmNil;
  } else {
    c.first = f.next;
    io.nodes[c.first].prev = kTsmNil;
  }
  c.pages -= 1;
  c.page_bytes -= f.len;
}

// sendToConnection (:624-633) for the records appended since the call began.
GPD_TSM_HD void tam_send(TamConn &c, const TamIo &io) {
  while (c.first != kTsmNil && tsm_diff(c.next_seq, io.nodes[c.first].seq) <= 0) tam_add_next(c, io);  // :636-640
  c.ncalls += 1;
  if (c.last_end) tam_close(c);
}

// insertIntoConn (:712-727): the segment cut into the nodes [page0, page0 + tsm_pages(len)).
GPD_TSM_HD void tam_insert(TamConn &c, const TamIo &io, const gpd_tcp_seg &s, uint32_t page0, bool end, uint64_t ts) {
  const uint32_t k = tsm_pages(s.payload_len);
  uint32_t left = s.payload_len, seq = s.seq, off = s.payload_off;
  for (uint32_t j = 0; j < k; ++j) {  // pagesFromTCP (:734-756)
    const uint32_t len = left < GPD_TCP_PAGE_BYTES ? left : GPD_TCP_PAGE_BYTES;
    TamNode n;
    n.prev = j ? page0 + j - 1u : kTsmNil;
    n.next = j + 1u < k ? page0 + j + 1u : kTsmNil;
    n.seq = seq;
    n.packet = s.packet;
    n.off = off;
    n.len = len;
    n.end = (j + 1u == k && end) ? 1u : 0u;
    n.pad = 0;
    n.seen = ts;
    n.pad2 = 0;
    io.nodes[page0 + j] = n;
    seq += len;
    off += len;
    left -= len;
  }
  const uint32_t p = page0, p2 = page0 + k - 1u;
  uint32_t prev = c.last, cur = kTsmNil;  // traverseConn (:683-690)
  while (prev != kTsmNil && tsm_diff(io.nodes[prev].seq, s.seq) < 0) {
    cur = prev;
    prev = io.nodes[cur].prev;
  }
  if (cur == kTsmNil || c.last == kTsmNil) {  // pushBetween (:696-710)
    c.last = p2;
  } else {
    io.nodes[p2].next = cur;
    io.nodes[cur].prev = p2;
  }
  if (prev == kTsmNil || c.first == kTsmNil) {
    c.first = p;
  } else {
    io.nodes[p].prev = prev;
    io.nodes[prev].next = p;
  }
  c.pages += k;
  c.page_bytes += s.payload_len;
  if (io.max_pages > 0 && c.pages >= io.max_pages) tam_add_next(c, io);  // :720-726
}

// AssembleWithTimestamp (:533-607) for one segment; page0: the first node of its pages.
GPD_TSM_HD void tam_step(TamConn &c, const TamIo &io, const gpd_tcp_seg &s, uint32_t page0, uint64_t ts) {
  const bool syn = s.flags & GPD_TCP_SYN, fin = s.flags & GPD_TCP_FIN, rst = s.flags & GPD_TCP_RST;
  if (!syn && !fin && !rst && s.payload_len == 0) return;  // :535
  if (!c.exists) {  // getConnection (:495-511)
    if (!syn && s.payload_len == 0) return;  // end: looked up, not created (:550-556)
    c.exists = 1;
    c.valid = 0;
    c.next_seq = 0;
    c.first = c.last = kTsmNil;
    c.pages = c.page_bytes = 0;
    c.last_seen = 0;
  }
  if (c.last_seen < ts) c.last_seen = ts;  // :564-566
  const uint32_t rec0 = c.nrec;
  c.last_end = 0;
  const uint32_t src = tam_packet_base(io, s.packet) + s.payload_off;
  if (!c.valid) {
    if (syn) {  // :569-579
      tam_emit(c, io, s.packet, s.payload_off, src, s.payload_len, 0, GPD_TCP_R_START, ts);
      c.next_seq = s.seq + s.payload_len + 1u;
      c.valid = 1;
    } else {
      tam_insert(c, io, s, page0, fin || rst, ts);
    }
  } else if (tsm_diff(c.next_seq, s.seq) > 0) {  // :586-590
    tam_insert(c, io, s, page0, fin || rst, ts);
  } else {  // :591-602
    const uint32_t trim = tam_byte_span(c, s.seq, s.payload_len);
    tam_emit(c, io, s.packet, s.payload_off + trim, src + trim, s.payload_len - trim, 0,
             (rst || fin) ? GPD_TCP_R_END : 0u, ts);
  }
  if (c.nrec != rec0) tam_send(c, io);  // :603-605
}

// skipFlush (:645-657).
GPD_TSM_HD void tam_skip_flush(TamConn &c, const TamIo &io) {
  if (c.first == kTsmNil) {
    tam_close(c);
    return;
  }
  c.last_end = 0;
  tam_add_next(c, io);
  tam_send(c, io);
}

// The end of a run: FlushWithOptions{T: fl.before_ns, CloseAll: fl.close_all} (:235-266), then
// with fl.flush_all FlushAll (:276-287).  A closed connection is out of the pool (c.exists == 0).
GPD_TSM_HD void tam_flush(TamConn &c, const TamIo &io, const gpd_tcp_flush &fl) {
  if (!c.exists) return;
  c.cur_flags = GPD_TCP_R_FLUSHED;
  while (c.exists && c.first != kTsmNil && io.nodes[c.first].seen < fl.before_ns) tam_skip_flush(c, io);  // :247-254
  if (fl.close_all && c.exists && c.first == kTsmNil && c.last_seen < fl.before_ns) tam_close(c);         // :255-259
  if (fl.flush_all)
    while (c.exists) tam_skip_flush(c, io);  // :281-283
  c.cur_flags = 0;
}

// Whether steps 2 and 3 touch a held connection that has no segment in the run (its first page's
// Seen given when it has pages).
GPD_TSM_HD bool tam_flush_touches(const gpd_tcp_conn_info &ci, uint64_t first_seen, const gpd_tcp_flush &fl) {
  if (!(ci.flags & GPD_TCP_CONN_OPEN)) return false;
  if (fl.flush_all) return true;
  if (ci.pages) return first_seen < fl.before_ns;
  return fl.close_all && ci.last_seen_ns < fl.before_ns;
}

}  // namespace gpd
