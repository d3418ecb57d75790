// pool_pick.h -- which context of a balanced pool takes the next batch (nbls_pool_init_ex, NBLS_POOL_BALANCE).
// Plain C++, no HIP: the pool (nbls_multi.cpp) and a host-only test (tests/c/pool_pick_test.cpp) share it.
#pragma once
namespace nbls {
// outstanding[i] = batches enqueued on context i whose completion event has not been seen yet, i = 0 .. depth-1; K = the most a context may have outstanding;
// `after` = the context used last (any value: it is reduced mod depth; -1 before the first submit, so that the first pick is context 0).
// Returns the context with the fewest outstanding among those below K; ties go round-robin, to the first such context behind `after` (wrapping around).  From all-zero
// counts, depth consecutive picks (each counted as outstanding) therefore visit every context once, in index order: a pool nobody waits on behaves like the round-robin one.
// -1: every context is at K (or depth < 1, K < 1): the caller waits until one retires.
inline int pool_pick(const int* outstanding, int depth, int K, int after) {
  if (!outstanding || depth < 1 || K < 1) return -1;
  int start = (after % depth + depth + 1) % depth, best = -1;
  for (int j = 0; j < depth; j++) {
    const int i = (start + j) % depth;
    if (outstanding[i] < K && (best < 0 || outstanding[i] < outstanding[best])) best = i;
  }
  return best;
}
}  // namespace nbls
