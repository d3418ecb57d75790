// pool_levels.h -- which stream priority a pool context gets when the pool spreads its streams over the priority levels (nbls_pool_init_ex, NBLS_POOL_SPREAD_PRIORITIES).
// Plain C++, no HIP: the pool (nbls_multi.cpp) and a host-only test (tests/c/pool_levels_test.cpp) share it.
#pragma once
#include <vector>
namespace nbls {
// The priorities of the levels, level 0 first.  `greatest` / `least` are what hipDeviceGetStreamPriorityRange reports (numerically greatest <= 0 <= least; equal when the
// device has one level).  Level 0 is the default priority 0 (what hipStreamCreate gives), then the levels above it, nearest first, then the levels below it; at most
// `cap` levels (cap <= 0: all).  A range that does not contain 0 yields the one level `greatest`.
inline std::vector<int> pool_priority_levels(int greatest, int least, int cap) {
  std::vector<int> lv;
  if (greatest > least) { const int t = greatest; greatest = least; least = t; }
  if (greatest > 0 || least < 0) { lv.push_back(greatest); return lv; }
  lv.push_back(0);
  for (int p = -1; p >= greatest; p--) lv.push_back(p);
  for (int p = 1; p <= least; p++) lv.push_back(p);
  if (cap > 0 && (int)lv.size() > cap) lv.resize((size_t)cap);
  return lv;
}
// Level of context i of a pool of `depth` contexts on `queues` hardware queues per level and `levels` levels: 0 for every context when the streams fit the queues of one
// level (or there is one level), else i mod levels -- depth <= levels x queues then gives every stream a queue of its own; beyond that, streams share as they did.
inline int pool_priority_level(int i, int depth, int queues, int levels) {
  if (levels <= 1 || depth <= queues) return 0;
  return i % levels;
}
}  // namespace nbls
