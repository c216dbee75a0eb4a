// flow_slots_host.cpp — the flow table's slot rules (gopacket_amd/csrc/gpd_flow_slots.h) run
// sequentially on the host against a std::unordered_map: find-or-claim with tombstones, remove,
// and the sweep, on tables of 8, 64 and 1024 slots over random insert, remove and expire-all
// sequences.  A stand-alone program for a host sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/c/flow_slots_host.cpp -o flow_slots_host
//   flow_slots_host <seed> <steps per table>
//
// After every step: no key is stored twice, every live key is found where the map says, inserts
// succeed exactly while live keys < capacity, no tombstone run ends at an empty slot, and after
// removing everything every slot is empty.  Prints "ok <steps run> ..." with what the sequences
// reached, and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_flow_slots.h"

using namespace gpd;

static int fails;
static long n_full, n_tomb_claims, n_wrapped;  // what the sequences reached (printed)
#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      if (++fails < 20) std::printf("line %d: %s\n", __LINE__, #cond); \
    }                                                         \
  } while (0)

struct Table {
  uint64_t mask;
  std::vector<uint64_t> word;  // the slots' fingerprint words
  std::vector<uint64_t> key;   // the stored key (0 where none)
  explicit Table(uint64_t cap) : mask(cap - 1), word(cap, 0), key(cap, 0) {}

  // The key's fingerprint: 20 hashed bits below (the home slot), the key itself above, so that
  // keys share home slots and chains, and no two keys a fingerprint; never 0, as the kernels'.
  static uint64_t fp_of(uint64_t k) { return ((k << 20) | ((k * 0x9E3779B97F4A7C15ull) >> 44)) & kSlotFpBits; }

  // find-or-claim: the slot, or kNoSlot when the table is full; *made says whether it was claimed
  uint64_t insert(uint64_t k, bool *made) {
    const uint64_t fp = fp_of(k);
    SlotProbe p = slot_probe_begin(fp, mask);
    *made = false;
    for (;;) {
      const SlotStep st = slot_probe_step(p, word[p.s], fp, mask);
      if (st == STEP_NEXT) continue;
      if (st == STEP_MATCH) {
        if (key[p.s] == k) return p.s;
        // another key under the fingerprint: a collision, which the kernels flag; the test's
        // fingerprints are injective on its keys, so this is a failure
        EXPECT(!"fingerprint collision");
        return kNoSlot;
      }
      if (st == STEP_FULL) return ++n_full, kNoSlot;
      if (st == STEP_CLAIM_TOMB) ++n_tomb_claims;
      if (st == STEP_CLAIM_TOMB && p.left == 0) ++n_wrapped;  // claimed after the whole circle: no empty slot
      const uint64_t s = st == STEP_CLAIM_TOMB ? p.tomb : p.s;
      EXPECT(slot_kind(word[s]) == (st == STEP_CLAIM_TOMB ? SLOT_TOMB : SLOT_EMPTY));
      word[s] = fp | (3ull << 56);
      key[s] = k;
      *made = true;
      return s;
    }
  }
  void remove(uint64_t s) {
    if (slot_kind(word[s]) != SLOT_USED) return;
    word[s] = kSlotTomb;
    key[s] = 0;
  }
  void sweep(uint64_t live) {
    if (live == 0) {  // the kernel's rule when no record is left
      for (auto &w : word)
        if (slot_kind(w) == SLOT_TOMB) w = 0;
      return;
    }
    for (uint64_t s = 0; s <= mask; s++)
      slot_sweep_at([&](uint64_t i) { return word[i]; }, [&](uint64_t i) { word[i] = 0; }, mask, s);
  }
};

static uint64_t rng_state;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static void check(const Table &t, const std::unordered_map<uint64_t, uint64_t> &live) {
  uint64_t used = 0;
  for (uint64_t s = 0; s <= t.mask; s++) {
    const SlotKind kind = slot_kind(t.word[s]);
    if (kind == SLOT_USED) {
      used++;
      auto it = live.find(t.key[s]);
      EXPECT(it != live.end() && it->second == s);  // stored once, where the map says
    }
    if (kind == SLOT_TOMB) EXPECT(slot_kind(t.word[(s + 1) & t.mask]) != SLOT_EMPTY || live.empty());
  }
  EXPECT(used == live.size());
  if (live.empty())
    for (uint64_t s = 0; s <= t.mask; s++) EXPECT(t.word[s] == 0);
  // every live key is found by the probe (read-only: a copy takes the claim, if one came)
  for (const auto &kv : live) {
    const uint64_t fp = Table::fp_of(kv.first);
    SlotProbe p = slot_probe_begin(fp, t.mask);
    SlotStep st;
    while ((st = slot_probe_step(p, t.word[p.s], fp, t.mask)) == STEP_NEXT) {
    }
    EXPECT(st == STEP_MATCH && p.s == kv.second);
  }
}

int main(int argc, char **argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
  const long steps = argc > 2 ? std::strtol(argv[2], nullptr, 10) : 2000;
  long run = 0;
  static_assert(slot_kind(0) == SLOT_EMPTY && slot_kind(kSlotTomb) == SLOT_TOMB && slot_kind(1) == SLOT_USED &&
                    slot_kind(0xFFull << 56) == SLOT_TOMB && slot_kind((1ull << 56) | 1ull) == SLOT_USED,
                "slot classification");
  for (uint64_t cap : {8ull, 64ull, 1024ull}) {
    rng_state = seed * 0x2545F4914F6CDD1Dull + cap;
    Table t(cap);
    std::unordered_map<uint64_t, uint64_t> live;  // key -> slot
    const uint64_t universe = cap * 2;            // keys 1..universe: the table fills up and overflows
    for (long step = 0; step < steps; step++, run++) {
      const uint64_t r = rnd() % 100;
      // phases of growth and of shrinking, so that the table is full at times and empty at others
      const bool grow = ((step / (long)(cap * 3)) & 1) == 0;
      if (r < (grow ? 70u : 25u)) {
        const uint64_t k = 1 + rnd() % universe;
        bool made = false;
        const uint64_t s = t.insert(k, &made);
        auto it = live.find(k);
        if (it != live.end()) {
          EXPECT(s == it->second && !made);
        } else if (live.size() < cap) {
          EXPECT(s != kNoSlot && made);  // a slot is free: the insert finds it
          if (s != kNoSlot) live[k] = s;
        } else {
          EXPECT(s == kNoSlot && !made);
        }
      } else if (r < 99 || rnd() % (cap / 8) != 0) {
        // remove a few records, duplicates and empty slots among them, then sweep
        const int m = 1 + (int)(rnd() % 4);
        for (int j = 0; j < m; j++) {
          const uint64_t s = rnd() & t.mask;
          if (slot_kind(t.word[s]) == SLOT_USED) live.erase(t.key[s]);
          t.remove(s);
          t.remove(s);
        }
        t.sweep(live.size());
      } else {
        for (uint64_t s = 0; s <= t.mask; s++) t.remove(s);  // expire everything
        live.clear();
        t.sweep(0);
      }
      if (cap <= 64 || step % 16 == 0 || live.empty()) check(t, live);
    }
    for (uint64_t s = 0; s <= t.mask; s++) t.remove(s);
    live.clear();
    t.sweep(0);
    check(t, live);
  }
  if (fails) return 1;
  std::printf("ok %ld full %ld tombstones claimed %ld after the whole circle %ld\n", run, n_full, n_tomb_claims,
              n_wrapped);
  return 0;
}
