// Host-only check of the balanced pool's choice (csrc/pool_pick.h): the context with the fewest batches outstanding, ties round-robin behind the context used last, -1 when
// every context is at the bound.  No device: tests/test_pool_pick.py builds and runs it, once plain and once under AddressSanitizer + UBSan.  Exit status 0 and "ok" when
// every case holds.
#include <cstdio>
#include <vector>
#include "pool_pick.h"
using namespace nbls;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)
static int pick(const std::vector<int>& o, int K, int after) { return pool_pick(o.data(), (int)o.size(), K, after); }
int main() {
  // the fewest outstanding wins, wherever `after` stands
  for (int after = -1; after < 4; after++) {
    EXPECT(pick({2, 1, 0, 1}, 3, after) == 2);
    EXPECT(pick({1, 2, 2, 2}, 3, after) == 0);
    EXPECT(pick({2, 2, 2, 1}, 3, after) == 3);
  }
  // a context at the bound is never taken: the one below K gets the batch, also when it is the context used last
  EXPECT(pick({2, 1, 2, 2}, 2, 1) == 1);
  EXPECT(pick({2, 2, 2, 1}, 2, 3) == 3);
  // ties go round-robin: the first of the tied contexts behind `after`, wrapping around
  EXPECT(pick({0, 0, 0, 0}, 2, -1) == 0);
  EXPECT(pick({0, 0, 0, 0}, 2, 0) == 1);
  EXPECT(pick({0, 0, 0, 0}, 2, 2) == 3);
  EXPECT(pick({0, 0, 0, 0}, 2, 3) == 0);      // wrap-around
  EXPECT(pick({1, 0, 1, 0}, 2, 1) == 3);
  EXPECT(pick({1, 0, 1, 0}, 2, 3) == 1);      // wraps past context 0, which has more
  EXPECT(pick({0, 1, 1, 0}, 2, 3) == 0);
  EXPECT(pick({1, 1, 1, 1}, 2, 2) == 3);
  EXPECT(pick({1, 1, 1, 1}, 2, 7) == 0);      // `after` is reduced mod depth: 7 = context 3
  EXPECT(pick({1, 1, 1, 1}, 2, -5) == 0);     // -5 = context 3 as well
  // all at K: -1; above K (never produced by the pool) counts as full too
  EXPECT(pick({2, 2, 2, 2}, 2, 0) == -1);
  EXPECT(pick({1, 1, 1}, 1, 2) == -1);
  EXPECT(pick({3, 2, 5}, 2, 1) == -1);
  EXPECT(pick({8, 8}, 8, 0) == -1);
  // K = 1: only idle contexts are taken
  EXPECT(pick({1, 0, 1}, 1, 1) == 1);
  EXPECT(pick({0, 1, 0}, 1, 0) == 2);
  EXPECT(pick({0, 1, 0}, 1, 2) == 0);
  EXPECT(pick({0, 0, 0}, 1, -1) == 0);
  // depth = 1: context 0 until it is full
  for (int after = -1; after < 2; after++) {
    EXPECT(pick({0}, 2, after) == 0);
    EXPECT(pick({1}, 2, after) == 0);
    EXPECT(pick({2}, 2, after) == -1);
    EXPECT(pick({0}, 1, after) == 0);
    EXPECT(pick({1}, 1, after) == -1);
  }
  // degenerate arguments answer "full", they do not read anything
  EXPECT(pool_pick(nullptr, 4, 2, 0) == -1);
  { const int o[1] = {0}; EXPECT(pool_pick(o, 0, 2, 0) == -1); EXPECT(pool_pick(o, -3, 2, 0) == -1); EXPECT(pool_pick(o, 1, 0, 0) == -1); }
  // from all-zero counts, depth consecutive picks visit every context once, in round-robin order, whatever K and wherever the walk starts; with nothing retiring, the next
  // depth picks do it again (K = 2) and then the pool is full
  for (int depth : {1, 2, 3, 4, 12, 64}) for (int K : {1, 2, 8}) for (int first_after : {-1, 0, depth - 1, depth / 2}) {
    std::vector<int> o((size_t)depth, 0), seen((size_t)depth, 0);
    int after = first_after;
    for (int round = 0; round < K; round++) {
      for (int s = 0; s < depth; s++) {
        const int k = pick(o, K, after);
        EXPECT(k >= 0 && k < depth);
        if (k < 0 || k >= depth) break;
        EXPECT(k == ((first_after % depth + depth) % depth + 1 + s) % depth);
        EXPECT(seen[(size_t)k] == round);
        seen[(size_t)k]++; o[(size_t)k]++; after = k;
      }
    }
    EXPECT(pick(o, K, after) == -1);
    // one context retires a batch: it is the only candidate
    o[(size_t)(depth / 2)]--;
    EXPECT(pick(o, K, after) == depth / 2);
  }
  // a fast context (retires between picks) takes more batches than a slow one, and no count ever exceeds K
  {
    std::vector<int> o(3, 0), got(3, 0);
    int after = -1;
    for (int s = 0; s < 30; s++) {
      if (o[1] > 0) o[1]--;      // context 1 completes a batch before every submit
      const int k = pick(o, 2, after);
      if (k < 0) { o[0]--; o[2]--; continue; }      // full: the slow ones retire one each
      o[(size_t)k]++; got[(size_t)k]++; after = k;
      for (int v : o) EXPECT(v >= 0 && v <= 2);
    }
    EXPECT(got[1] > got[0] && got[1] > got[2]);
  }
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
