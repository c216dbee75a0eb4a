// gpd_ip4reasm_walk.h — ip4defrag's state machine for one key (include/gpd_ip4reasm.h), as
// __host__ __device__ code: gpd_ip4reasm.hip runs it on lane 0 of a group's wave, and a host
// program (tests/c/ip4reasm_walk_host.cpp) runs the same code over generated groups under the
// sanitizers, as gpd_tcpstream_walk.h shares the assembler.
//
// Restated from ip4defrag/defrag.go: fragmentList.insert (:216-273), build (:278-328) and the
// part of DefragIPv4WithTimestamp that follows the insert (:115-134).  The list is an array of
// nodes in list order (container/list's order), so PushBack is a store at the end and
// InsertBefore a shift.  Highest and Current are uint16 and wrap as the reference's do.
#pragma once
#include <stdint.h>

#include "../../include/gpd_ip4reasm.h"
#include "gpd_gather.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_IPR_HD __host__ __device__ inline
#else
#define GPD_IPR_HD inline
#endif

namespace gpd {

// One fragment in a list (16 B): what insert and build read of the layer, and where its
// payload lies.
struct IprNode {
  uint32_t src;          // byte offset of Payload[0] in its base
  uint32_t payload_len;  // len(Payload)
  uint16_t frag_offset;  // FragOffset (units of 8 bytes)
  uint16_t length;       // Length
  uint32_t where;        // kIprStore: the object's byte store; kIprBatch: the current batch's data
};
constexpr uint32_t kIprStore = 0, kIprBatch = 1;

// One slice build appends: bytes [src, src + len) of base `where` to the datagram's payload at
// `pos` (the shared gather's piece, gpd_gather.h).
using IprPiece = GatherPiece;

// One key's fragmentList (:204-210); the nodes are the caller's array.
struct IprList {
  uint32_t nn;       // List.Len()
  uint32_t highest;  // uint16
  uint32_t current;  // uint16
  uint32_t final_received;
  uint64_t last_seen;
};

struct IprBuilt {  // a successful build
  uint32_t payload_len, npieces, nfrags, length, flags;
};

GPD_IPR_HD void ipr_list_init(IprList &L) {
  L.nn = 0;
  L.highest = L.current = 0;
  L.final_received = 0;
  L.last_seen = 0;
}

GPD_IPR_HD uint32_t ipr_frag_length(uint32_t length) { return (length - 20u) & 0xFFFFu; }  // in.Length - 20 (:253)

// build (:278-328): the pieces of the list in order into pieces[0 ...] (room for L.nn).  Returns
// GPD_IP4_COMPLETE, GPD_IP4_HOLE or GPD_IP4_INVALID; a failed build leaves B.npieces 0.
GPD_IPR_HD uint32_t ipr_build(const IprList &L, const IprNode *nodes, IprPiece *pieces, IprBuilt &B) {
  uint32_t cur = 0, pos = 0, np = 0, flags = 0;
  B.payload_len = B.npieces = B.flags = 0;
  B.nfrags = L.nn;
  B.length = L.highest;
  for (uint32_t k = 0; k < L.nn; ++k) {
    const IprNode e = nodes[k];
    const uint32_t off8 = ((uint32_t)e.frag_offset * 8u) & 0xFFFFu;
    uint32_t start = 0, len = 0;
    if (off8 == cur) {
      len = e.payload_len;
      cur = (cur + e.length - 20u) & 0xFFFFu;
    } else if (off8 < cur) {
      start = (cur - off8) & 0xFFFFu;
      if (start > ipr_frag_length(e.length)) return GPD_IP4_INVALID;
      if (start > e.payload_len) flags |= GPD_IP4_D_SHORT_SLICE;  // (Go panics: Payload[startAt:])
      else len = e.payload_len - start;
      cur = (cur + off8) & 0xFFFFu;  // (sic, :298)
    } else {
      return GPD_IP4_HOLE;
    }
    pieces[np++] = IprPiece{e.src + (len ? start : 0u), len, pos, e.where};
    pos += len;
  }
  B.payload_len = pos;
  B.npieces = np;
  B.flags = flags;
  return GPD_IP4_COMPLETE;
}

// One DefragIPv4WithTimestamp call from the insert on (:115-134) for fragment f (more: its
// MoreFragments bit) at time t.  nodes has room for every fragment the key can hold (the
// carried ones plus the group's records); pieces for as many.  Returns the outcome; with
// GPD_IP4_COMPLETE, B and pieces[0, B.npieces) describe the datagram.  The list is flushed
// (ipr_list_init) after a datagram and at the length limit, as d.flush does.
GPD_IPR_HD uint32_t ipr_step(IprList &L, IprNode *nodes, const IprNode &f, bool more, uint64_t t, IprPiece *pieces,
                             IprBuilt &B) {
  const uint32_t off8 = ((uint32_t)f.frag_offset * 8u) & 0xFFFFu;
  uint32_t what = GPD_IP4_FILED;
  bool dup = false;
  B.npieces = 0;
  if (off8 >= L.highest) {
    nodes[L.nn++] = f;  // PushBack
  } else {
    for (uint32_t k = 0; k < L.nn; ++k) {
      const uint32_t eo = nodes[k].frag_offset;
      if (f.frag_offset == eo) {
        dup = true;  // ignored, nothing counted (:225-240)
        break;
      }
      if (f.frag_offset < eo) {  // InsertBefore
        for (uint32_t j = L.nn; j > k; --j) nodes[j] = nodes[j - 1u];
        nodes[k] = f;
        ++L.nn;
        break;
      }
    }  // (no larger offset stored: counted below without being stored)
  }
  if (!dup) {
    L.last_seen = t;
    const uint32_t fl = ipr_frag_length(f.length);
    const uint32_t end = (off8 + fl) & 0xFFFFu;
    if (L.highest < end) L.highest = end;
    L.current = (L.current + fl) & 0xFFFFu;
    if (!more) L.final_received = 1;
    if (L.final_received && L.highest == L.current) what = ipr_build(L, nodes, pieces, B);
  }
  if (what != GPD_IP4_COMPLETE && L.nn + 1u > GPD_IP4_MAX_LIST_LEN) {  // :120-125
    ipr_list_init(L);
    return GPD_IP4_LIST_FULL;
  }
  if (what == GPD_IP4_COMPLETE) ipr_list_init(L);  // :128-133
  return what;
}

}  // namespace gpd
