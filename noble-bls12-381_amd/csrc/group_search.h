// group_search.h -- which contiguous group a position belongs to.  Keys of a set (agg_kernels.hip), identifiers of a polynomial (poly_kernels.hip), scalars of a sum
// (msm_kernels.hip) and shares of a threshold group (fr_exec.h, also compiled into the test-only simulator) all lie group after group behind ngroups + 1 increasing offsets;
// the search is written here once.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define NBLS_GS_HD __host__ __device__ inline
#else
#define NBLS_GS_HD inline
#endif

namespace nbls {
// the last g in [lo, hi) with off[g] <= k.  The caller knows off[lo] <= k; when k < off[hi] as well, off[g] <= k < off[g + 1] (with empty groups: the one that owns k)
NBLS_GS_HD uint32_t group_search(const uint32_t* off, uint32_t lo, uint32_t hi, uint32_t k) {
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}
}  // namespace nbls
