// Host-only check of the pool's level assignment (csrc/pool_levels.h): which stream priority context i of a pool gets when the pool spreads its streams over the priority
// levels.  No device: tests/test_gpu_pool_priorities.py builds and runs it.  Exit status 0 and "ok" when every case holds.
#include <cstdio>
#include <vector>
#include "pool_levels.h"
using namespace nbls;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)
int main() {
  // the device's three levels: default first, then high, then low; a cap of two keeps default and high
  EXPECT((pool_priority_levels(-1, 1, 0) == std::vector<int>{0, -1, 1}));
  EXPECT((pool_priority_levels(-1, 1, 3) == std::vector<int>{0, -1, 1}));
  EXPECT((pool_priority_levels(-1, 1, 2) == std::vector<int>{0, -1}));
  EXPECT((pool_priority_levels(1, -1, 0) == std::vector<int>{0, -1, 1}));      // the two bounds in either order
  EXPECT((pool_priority_levels(-2, 0, 0) == std::vector<int>{0, -1, -2}));
  // one level: the default priority alone, whatever the cap
  EXPECT((pool_priority_levels(0, 0, 0) == std::vector<int>{0}));
  EXPECT((pool_priority_levels(0, 0, 3) == std::vector<int>{0}));
  EXPECT(pool_priority_levels(2, 5, 0).size() == 1);
  // L == 1: every context on level 0, at any depth
  for (int depth : {1, 4, 5, 12, 64}) for (int i = 0; i < depth; i++) EXPECT(pool_priority_level(i, depth, 4, 1) == 0);
  // the streams fit the queues of one level: nothing is spread
  for (int i = 0; i < 4; i++) EXPECT(pool_priority_level(i, 4, 4, 3) == 0);
  for (int i = 0; i < 12; i++) EXPECT(pool_priority_level(i, 12, 22, 3) == 0);
  // twelve on a cap of four and three levels: i mod 3, four streams a level
  int count[3] = {0, 0, 0};
  for (int i = 0; i < 12; i++) { const int l = pool_priority_level(i, 12, 4, 3); EXPECT(l == i % 3); count[l]++; }
  EXPECT(count[0] == 4 && count[1] == 4 && count[2] == 4);
  // two levels: six streams a level; depth beyond levels x queues still assigns a level (streams share again, no error)
  for (int i = 0; i < 12; i++) EXPECT(pool_priority_level(i, 12, 4, 2) == i % 2);
  for (int i = 0; i < 64; i++) { const int l = pool_priority_level(i, 64, 4, 3); EXPECT(l >= 0 && l < 3 && l == i % 3); }
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
