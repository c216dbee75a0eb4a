// gpd_flow_slots.h — the flow table's slot rules since records can leave it
// (include/gpd_flow_expire.h): what a slot's fingerprint word says, the probe of a table that
// holds tombstones as a step function, and the sweep that turns tombstones back into empty
// slots.  Plain C++17 for host and device: the kernels of gpd_flow.hip run these functions with
// their loads, compare-and-swaps and stores around them, and tests/c/flow_slots_host.cpp runs
// them sequentially against a std::unordered_map.
//
// A slot's word is 0 (empty: never used since the last reset, or swept), a fingerprint (56 bits,
// never 0, with the claiming launch's epoch in the top byte), or the tombstone: a record that
// StreamPool.remove took out (tcpassembly/assembly.go:659-676) while later slots of its chain may
// hold keys that probed past it.  A probe therefore walks past tombstones and only an empty slot
// ends a chain.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPD_SLOT_HD __host__ __device__ __forceinline__
#else
#define GPD_SLOT_HD inline
#endif

namespace gpd {

constexpr uint64_t kSlotFpBits = (1ull << 56) - 1ull;  // the fingerprint in a slot's word
constexpr uint64_t kSlotTomb = 1ull << 56;             // non-zero, fingerprint bits zero
constexpr uint64_t kNoSlot = ~0ull;

enum SlotKind : uint32_t { SLOT_EMPTY = 0, SLOT_TOMB = 1, SLOT_USED = 2 };

GPD_SLOT_HD constexpr SlotKind slot_kind(uint64_t word) {
  return word == 0ull ? SLOT_EMPTY : (word & kSlotFpBits) == 0ull ? SLOT_TOMB : SLOT_USED;
}

// A find-or-claim in progress for fingerprint fp in a table of mask + 1 slots.
struct SlotProbe {
  uint64_t s;     // the slot to look at next
  uint64_t left;  // slots of the circle not looked at yet, s included
  uint64_t tomb;  // the first tombstone met, or kNoSlot
};

enum SlotStep : uint32_t {
  STEP_NEXT = 0,     // walked on: read slot p.s and step again
  STEP_MATCH,        // slot p.s holds the fingerprint
  STEP_CLAIM_EMPTY,  // no record: claim the empty slot p.s (0 -> fingerprint)
  STEP_CLAIM_TOMB,   // no record: claim the remembered tombstone p.tomb (tombstone -> fingerprint)
  STEP_FULL          // the whole circle holds other fingerprints
};

GPD_SLOT_HD SlotProbe slot_probe_begin(uint64_t fp, uint64_t mask) {
  return SlotProbe{fp & mask, mask + 1ull, kNoSlot};
}

// One step, given the word read at p.s.  The first tombstone of the chain is remembered and
// claimed once the chain has ended without the fingerprint: at an empty slot, or after the whole
// circle.  Without one the empty slot is claimed, as in a table that never had a removal.
GPD_SLOT_HD SlotStep slot_probe_step(SlotProbe &p, uint64_t word, uint64_t fp, uint64_t mask) {
  if (p.left == 0ull) return p.tomb != kNoSlot ? STEP_CLAIM_TOMB : STEP_FULL;
  const SlotKind kind = slot_kind(word);
  if (kind == SLOT_EMPTY) return p.tomb != kNoSlot ? STEP_CLAIM_TOMB : STEP_CLAIM_EMPTY;
  if (kind == SLOT_USED && (word & kSlotFpBits) == fp) return STEP_MATCH;
  if (kind == SLOT_TOMB && p.tomb == kNoSlot) p.tomb = p.s;
  p.s = (p.s + 1ull) & mask;
  p.left -= 1ull;
  return STEP_NEXT;
}

// The claim of p.tomb lost its compare-and-swap (concurrent probers only): the slot holds a
// fingerprint now, perhaps this one, so the probe resumes there with nothing remembered.
GPD_SLOT_HD void slot_probe_lost_tomb(SlotProbe &p, uint64_t fp, uint64_t mask) {
  p.left = mask + 1ull - ((p.tomb - (fp & mask)) & mask);
  p.s = p.tomb;
  p.tomb = kNoSlot;
}

// The sweep's rule for slot s, one caller per slot in any order or all at once: an empty slot
// whose predecessor is a tombstone clears the run of tombstones that ends at it, walking
// backwards (indices wrap) until a slot that is not a tombstone.  A chain that reached such a
// tombstone went on to the empty slot and ended there; ending one slot earlier loses no key.  A
// run that ends at a record stays: keys behind it may have probed through.  word_at(i) reads slot
// i's word, clear(i) stores 0 there; callers that meet on one run store the same zeros.  Returns
// the slots cleared.
template <class WordAt, class Clear>
GPD_SLOT_HD uint64_t slot_sweep_at(WordAt word_at, Clear clear, uint64_t mask, uint64_t s) {
  if (slot_kind(word_at(s)) != SLOT_EMPTY) return 0ull;
  uint64_t n = 0ull, t = (s - 1ull) & mask;
  while (n <= mask && slot_kind(word_at(t)) == SLOT_TOMB) {
    clear(t);
    t = (t - 1ull) & mask;
    n += 1ull;
  }
  return n;
}

}  // namespace gpd
