// gpd_tcpstream_walk.h — the assembler's state machine for one connection (include/gpd_tcpstream.h),
// as __host__ __device__ code: gpd_tcpstream.hip runs it on lane 0 of a group's wave, and a host
// program (tests/c/tcpstream_walk_host.cpp) runs the same code over generated groups under the
// sanitizers, as gpd_bpf_vm.h shares the BPF interpreter.
//
// Restated from tcpassembly/assembly.go: Sequence.Difference (:54-61), AssembleWithTimestamp
// (:533-607) with getConnection (:495-511), byteSpan (:609-620), sendToConnection (:624-633),
// addContiguous (:636-640), skipFlush (:645-657), closeConnection (:666-676), traverseConn
// (:683-690), pushBetween (:696-710), insertIntoConn (:712-727), pagesFromTCP (:734-756) and
// addNextFromConn (:760-780).  The out-of-order list's nodes are pages, not segments: a later
// segment may land between two pages of an earlier one (traverseConn walks page by page).
#pragma once
#include <stdint.h>

#include "../../include/gpd_tcpstream.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_TSM_HD __host__ __device__ inline
#else
#define GPD_TSM_HD inline
#endif

namespace gpd {

constexpr uint32_t kTsmNil = 0xFFFFFFFFu;

// Pages a segment is cut into when it is buffered (pagesFromTCP: at least one, :735-737).
GPD_TSM_HD uint32_t tsm_pages(uint32_t payload_len) {
  return payload_len == 0 ? 1u : (payload_len + GPD_TCP_PAGE_BYTES - 1u) / GPD_TCP_PAGE_BYTES;
}

// One page of the out-of-order list (32 B).
struct TsmNode {
  uint32_t prev, next;  // node ids, kTsmNil
  uint32_t seq;
  uint32_t packet;      // the packet its bytes lie in
  uint32_t off, len;    // the page's bytes: packet bytes [off, off + len)
  uint32_t end;         // page.End (:754)
  uint32_t pad;
};

// One key's connection and the group's running output.
struct TsmConn {
  uint32_t exists;    // in the pool
  uint32_t valid;     // nextSeq != invalidSequence
  uint32_t next_seq;
  uint32_t first, last;  // the page list, kTsmNil when empty
  uint32_t pages;        // conn.pages
  uint32_t nrec, ncalls, completed;
  uint32_t nbytes;    // bytes delivered so far (< 2^32: every byte is a byte of the batch)
  uint32_t cur_flags; // GPD_TCP_R_FLUSHED while the drain runs
  uint32_t last_end;  // End of the last record appended to the call under construction
};

struct TsmIo {
  TsmNode *nodes;       // the batch's page nodes, by page id
  gpd_tcp_reasm *recs;  // the group's private record region
  uint32_t cap;         // its capacity: the group's pages (a page or a segment gives one record at most)
  uint32_t max_pages;   // MaxBufferedPagesPerConnection
};

GPD_TSM_HD void tsm_conn_init(TsmConn &c, uint32_t open, uint32_t next_seq) {
  c.exists = open;
  c.valid = open;
  c.next_seq = next_seq;
  c.first = c.last = kTsmNil;
  c.pages = 0;
  c.nrec = c.ncalls = c.completed = 0;
  c.nbytes = 0;
  c.cur_flags = 0;
  c.last_end = 0;
}

// Sequence.Difference (:54-61): t - s, roll-over safe between the outer quarters only.
GPD_TSM_HD int64_t tsm_diff(uint32_t s32, uint32_t t32) {
  int64_t s = s32, t = t32;
  const int64_t U = 1ll << 32, Q = U / 4;
  if (s > U - Q && t < Q) t += U;
  else if (t > U - Q && s < Q) s += U;
  return t - s;
}

// One record appended to the call under construction.
GPD_TSM_HD void tsm_emit(TsmConn &c, const TsmIo &io, uint32_t packet, uint32_t src_off, uint32_t len, int32_t skip,
                         uint32_t flags) {
  c.last_end = (flags & GPD_TCP_R_END) ? 1u : 0u;
  if (c.nrec >= io.cap) return;  // (cannot happen: see TsmIo::cap)
  gpd_tcp_reasm r;
  r.packet = packet;
  r.src_off = len ? src_off : 0u;  // (no Bytes[0]: zero)
  r.len = len;
  r.skip = skip;
  r.stream_off = c.nbytes;
  r.call = c.ncalls;
  r.flags = (uint16_t)(flags | c.cur_flags);
  r.reserved = 0;
  io.recs[c.nrec] = r;
  c.nrec += 1;
  c.nbytes += len;
}

// byteSpan (:609-620) on a span of `len` bytes received at `seq`: the bytes trimmed from its
// front (all of them when it ends before nextSeq: Bytes == nil) and the new nextSeq.
GPD_TSM_HD uint32_t tsm_byte_span(TsmConn &c, uint32_t seq, uint32_t len) {
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

// closeConnection (:666-676): ReassemblyComplete, out of the pool, its pages dropped.
GPD_TSM_HD void tsm_close(TsmConn &c) {
  c.completed += 1;
  c.exists = c.valid = 0;
  c.next_seq = 0;
  c.first = c.last = kTsmNil;
  c.pages = 0;
}

// addNextFromConn (:760-780).
GPD_TSM_HD void tsm_add_next(TsmConn &c, const TsmIo &io) {
  const TsmNode f = io.nodes[c.first];
  int32_t skip = 0;
  if (!c.valid) {
    skip = -1;
  } else {
    const int64_t d = tsm_diff(c.next_seq, f.seq);
    if (d > 0) skip = d > 0x7FFFFFFFll ? 0x7FFFFFFF : (int32_t)d;  // (Skip is an int: saturated to 32 bits)
  }
  const uint32_t trim = tsm_byte_span(c, f.seq, f.len);
  tsm_emit(c, io, f.packet, f.off + trim, f.len - trim, skip, f.end ? GPD_TCP_R_END : 0u);
  if (c.first == c.last || f.next == kTsmNil) {  // (the second cannot differ: pushBetween keeps the list whole)
    c.first = c.last = kTsmNil;
  } else {
    c.first = f.next;
    io.nodes[c.first].prev = kTsmNil;
  }
  c.pages -= 1;
}

// sendToConnection (:624-633) for the records appended since the call began.
GPD_TSM_HD void tsm_send(TsmConn &c, const TsmIo &io) {
  while (c.first != kTsmNil && tsm_diff(c.next_seq, io.nodes[c.first].seq) <= 0) tsm_add_next(c, io);  // :636-640
  c.ncalls += 1;
  if (c.last_end) tsm_close(c);
}

// insertIntoConn (:712-727): the segment cut into pages [page0, page0 + tsm_pages(len)).
GPD_TSM_HD void tsm_insert(TsmConn &c, const TsmIo &io, const gpd_tcp_seg &s, uint32_t page0, bool end) {
  const uint32_t k = tsm_pages(s.payload_len);
  uint32_t left = s.payload_len, seq = s.seq, off = s.payload_off;
  for (uint32_t j = 0; j < k; ++j) {  // pagesFromTCP (:734-756)
    const uint32_t len = left < GPD_TCP_PAGE_BYTES ? left : GPD_TCP_PAGE_BYTES;
    TsmNode n;
    n.prev = j ? page0 + j - 1u : kTsmNil;
    n.next = j + 1u < k ? page0 + j + 1u : kTsmNil;
    n.seq = seq;
    n.packet = s.packet;
    n.off = off;
    n.len = len;
    n.end = (j + 1u == k && end) ? 1u : 0u;
    n.pad = 0;
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
  if (io.max_pages > 0 && c.pages >= io.max_pages) tsm_add_next(c, io);  // :720-726
}

// AssembleWithTimestamp (:533-607) for one segment of the group; page0: its first page id.
GPD_TSM_HD void tsm_step(TsmConn &c, const TsmIo &io, const gpd_tcp_seg &s, uint32_t page0) {
  const bool syn = s.flags & GPD_TCP_SYN, fin = s.flags & GPD_TCP_FIN, rst = s.flags & GPD_TCP_RST;
  if (!syn && !fin && !rst && s.payload_len == 0) return;  // :535
  if (!c.exists) {  // getConnection (:495-511)
    if (!syn && s.payload_len == 0) return;  // end: looked up, not created (:550-556)
    c.exists = 1;
    c.valid = 0;
    c.next_seq = 0;
    c.first = c.last = kTsmNil;
    c.pages = 0;
  }
  const uint32_t rec0 = c.nrec;
  c.last_end = 0;
  if (!c.valid) {
    if (syn) {  // :569-579
      tsm_emit(c, io, s.packet, s.payload_off, s.payload_len, 0, GPD_TCP_R_START);
      c.next_seq = s.seq + s.payload_len + 1u;
      c.valid = 1;
    } else {
      tsm_insert(c, io, s, page0, fin || rst);
    }
  } else if (tsm_diff(c.next_seq, s.seq) > 0) {  // :586-590
    tsm_insert(c, io, s, page0, fin || rst);
  } else {  // :591-602
    const uint32_t trim = tsm_byte_span(c, s.seq, s.payload_len);
    tsm_emit(c, io, s.packet, s.payload_off + trim, s.payload_len - trim, 0, (rst || fin) ? GPD_TCP_R_END : 0u);
  }
  if (c.nrec != rec0) tsm_send(c, io);  // :603-605
}

// The end of the batch: the drain (`for conn.first != nil && !conn.closed { skipFlush }`, :247-254
// with T later than every packet) and, with close_all, FlushAll's close (:281-283).
GPD_TSM_HD void tsm_finish(TsmConn &c, const TsmIo &io, bool close_all) {
  c.cur_flags = GPD_TCP_R_FLUSHED;
  while (c.exists && c.first != kTsmNil) {  // skipFlush (:645-657)
    c.last_end = 0;
    tsm_add_next(c, io);
    tsm_send(c, io);
  }
  c.cur_flags = 0;
  if (close_all && c.exists) tsm_close(c);  // skipFlush on an empty list (:649-651)
}

}  // namespace gpd
