// tcptrack_fsm_host.cpp — the connection tracker's step function and map algebra
// (gopacket_amd/csrc/gpd_tcptrack_fsm.h) on the host.  A stand-alone program for a sanitizer
// build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/c/tcptrack_fsm_host.cpp -o tcptrack_fsm_host
//
//   tcptrack_fsm_host table         prints `option state t.dir code state' t.dir' accept` for all
//                                   2 x 12 x 32 inputs (compared with tests/tcptrack_ref.py)
//   tcptrack_fsm_host scan SEED N   N random packet sequences of length 1..300 per option: the
//                                   verdicts from composed prefix maps equal the sequential
//                                   ones — composed as a left fold, as a balanced tree, and in
//                                   pieces cut at arbitrary points, each piece seeded with the
//                                   state the one before carried out.  Prints "ok <sequences>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../gopacket_amd/csrc/gpd_tcptrack_fsm.h"

using namespace gpd::fsm;

static constexpr GenTable kGen = make_gen_table();
static_assert(kGen.g[0][0] == generator(0, false) && kGen.g[1][31] == generator(31, true), "compile-time table");

static int fails;
#define EXPECT(cond)                                      \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("line %d: %s\n", __LINE__, #cond);      \
      if (++fails > 20) std::exit(1);                     \
    }                                                     \
  } while (0)

// The verdict bytes of `codes` from element e0, one CheckState after another; *e_out: the element after.
static std::vector<uint8_t> sequential(const std::vector<uint32_t> &codes, bool opt, uint32_t e0, uint32_t *e_out) {
  std::vector<uint8_t> v;
  uint32_t e = e0;
  for (uint32_t c : codes) {
    const Step s = step(e % 6u, e / 6u, c, opt);
    v.push_back((uint8_t)verdict(s, c));
    e = elem(s.state, s.tdir);
  }
  *e_out = e;
  return v;
}

// The verdicts from inclusive prefix maps `inc` (inc[k] = codes 0..k composed) and the element e0.
static std::vector<uint8_t> from_prefixes(const std::vector<uint32_t> &codes, const std::vector<Map> &inc, bool opt,
                                          uint32_t e0, uint32_t *e_out) {
  std::vector<uint8_t> v;
  for (size_t k = 0; k < codes.size(); ++k) {
    const uint32_t before = apply(k ? inc[k - 1] : kIdentity, e0);
    const Step s = step(before % 6u, before / 6u, codes[k], opt);
    v.push_back((uint8_t)verdict(s, codes[k]));
    EXPECT(elem(s.state, s.tdir) == apply(inc[k], e0));
  }
  *e_out = apply(inc.back(), e0);
  return v;
}

static std::vector<Map> left_fold(const std::vector<Map> &g) {
  std::vector<Map> inc(g.size());
  Map m = kIdentity;
  for (size_t k = 0; k < g.size(); ++k) inc[k] = m = compose(m, g[k]);
  return inc;
}

// Inclusive prefixes of g[lo, hi) by halves: the right half's prefixes get the left half's total in front.
static void tree(const std::vector<Map> &g, size_t lo, size_t hi, std::vector<Map> &inc) {
  if (hi - lo == 1) {
    inc[lo] = g[lo];
    return;
  }
  const size_t mid = lo + (hi - lo) / 2;
  tree(g, lo, mid, inc);
  tree(g, mid, hi, inc);
  for (size_t k = mid; k < hi; ++k) inc[k] = compose(inc[mid - 1], inc[k]);
}

static int run_table() {
  for (uint32_t o = 0; o < 2; ++o)
    for (uint32_t e = 0; e < kElems; ++e)
      for (uint32_t c = 0; c < kCodes; ++c) {
        const Step s = step(e % 6u, e / 6u, c, o != 0);
        std::printf("%u %u %u %u %u %u %u\n", o, e % 6u, e / 6u, c, s.state, s.tdir, s.accept);
        EXPECT(apply(kGen.g[o][c], e) == elem(s.state, s.tdir));
      }
  return fails ? 1 : 0;
}

static int run_scan(uint64_t seed, int count) {
  std::mt19937_64 rng(seed);
  // codes that reach every state: SYN, SYN+ACK, ACK, FIN+ACK, RST and anything else, either direction
  const uint32_t often[] = {kSyn, kSyn | kAck, kAck, kAck, kAck, kFin | kAck, kFin, kRst, kRst | kAck};
  for (uint32_t e = 0; e < kElems; ++e) {
    EXPECT(elem_of_byte(byte_of_elem(e)) == e && apply(kIdentity, e) == e);
    EXPECT(byte_of_elem(e) == ((e % 6u) | ((e / 6u) << 3)));
  }
  int done = 0;
  for (int opt = 0; opt < 2; ++opt)
    for (int it = 0; it < count; ++it, ++done) {
      const size_t len = 1 + rng() % 300;
      std::vector<uint32_t> codes(len);
      for (auto &c : codes) {
        c = (rng() % 4 == 0) ? (uint32_t)(rng() % kCodes) : often[rng() % (sizeof often / sizeof often[0])];
        if (rng() % 2) c ^= kDir;
      }
      std::vector<Map> g(len);
      for (size_t k = 0; k < len; ++k) g[k] = kGen.g[opt][codes[k]];
      const uint32_t e0 = it % 3 == 0 ? (uint32_t)(rng() % kElems) : 0u;  // (a fresh FSM, or any carried state)
      uint32_t e_seq, e_a, e_b;
      const std::vector<uint8_t> want = sequential(codes, opt != 0, e0, &e_seq);
      const std::vector<Map> fold = left_fold(g);
      std::vector<Map> tr(len);
      tree(g, 0, len, tr);
      EXPECT(from_prefixes(codes, fold, opt != 0, e0, &e_a) == want && e_a == e_seq);
      EXPECT(from_prefixes(codes, tr, opt != 0, e0, &e_b) == want && e_b == e_seq);
      EXPECT(fold == tr);
      // pieces: each scanned from the identity and applied to the element carried into it
      std::vector<uint8_t> got;
      uint32_t e = e0;
      for (size_t lo = 0; lo < len;) {
        const size_t n = 1 + rng() % (len - lo);
        const std::vector<uint32_t> piece(codes.begin() + lo, codes.begin() + lo + n);
        std::vector<Map> pg(g.begin() + lo, g.begin() + lo + n), inc(n);
        tree(pg, 0, n, inc);
        uint32_t e_next;
        const std::vector<uint8_t> v = from_prefixes(piece, inc, opt != 0, e, &e_next);
        got.insert(got.end(), v.begin(), v.end());
        e = e_next;
        lo += n;
      }
      EXPECT(got == want && e == e_seq);
    }
  if (fails) return 1;
  std::printf("ok %d\n", done);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "table")) return run_table();
  if (argc == 4 && !std::strcmp(argv[1], "scan")) return run_scan(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]));
  std::fprintf(stderr, "usage: %s table | scan SEED N\n", argv[0]);
  return 2;
}
