// agg_kernels.hip -- the data movement of nbls_verify_aggregates (pipelines_multi_verify.cpp): which set every key belongs to, the identity in place of the keys that add
// nothing, the gather from a key table (nbls_keyset), one status byte per set, and the fixed point that stands in for a zero sum on its way into a Miller loop (the shared-message
// forms' group keys, the KZG verifier's combined points).  The additions themselves are the MSM's list-driven rounds (msm_kernels.hip msm_pairs_kernel +
// P_G1_ADD_AB); nothing here computes on curve points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "group_search.h"
#include "kernel_parts.h"
#include "launchers.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

// one thread per key k of the call: its set j (koff[j] <= k < koff[j + 1]; the n + 1 offsets are relative and, sets being non-empty, strictly increasing), its rank in the set,
// its status (st_src[index[k]] from a key table, st_src[k] without an index), and first_bad[j] = the lowest k of set j whose status is >= 2 (a key that did not decode)
__global__ void agg_keys_kernel(u32 nkeys, u32 n, const u32* __restrict__ koff, const u32* __restrict__ index, const int8_t* __restrict__ st_src, u32* __restrict__ set_id,
                                u32* __restrict__ rank, int8_t* __restrict__ st, u32* __restrict__ first_bad) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  const u32 lo = group_search(koff, 0, n, k);
  set_id[k] = lo;
  rank[k] = k - koff[lo];
  const int8_t v = st_src[index ? index[k] : k];
  st[k] = v;
  if (v >= 2) atomicMin(&first_bad[lo], k);
}

// dst[k] = the projective identity where key k's status is not 0 (a zero key adds nothing, as PointG1.ZERO.add does; a key that did not decode is replaced so that the sum stays
// defined), else src[index[k]] (src[k] without an index: src may then be dst).  q = 16-byte vectors per point, one vector per thread.
__global__ void agg_points_kernel(u64 nkeys, u32 q, const u32* __restrict__ index, const int8_t* __restrict__ st, const uint4* __restrict__ ident, const uint4* src, uint4* dst) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nkeys * q) return;
  const VecPart v = vec_split(t, q);
  dst[t] = st[v.elem] ? ident[v.part] : src[(index ? (u64)index[v.elem] : v.elem) * q + v.part];
}

// out[j] = the status of set j's first key that did not decode, else the aggregate's (1 when the keys sum to the zero point, 0 otherwise)
__global__ void agg_status_kernel(u32 n, const u32* __restrict__ first_bad, const int8_t* __restrict__ st, const int8_t* __restrict__ zero, int8_t* __restrict__ out) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u32 f = first_bad[j];
  out[j] = f != 0xffffffffu ? st[f] : zero[j];
}

// pts[i] = `fixed`, a valid affine point, where zero[i] == 1 (the flag of P_G1_TO_AFFINE or of the MSM: the sum is the zero point, which cannot go into a Miller loop), and
// *flag = 1 when a flag word is given; the caller takes its verdict from the flags, not from that factor.  Six 16-byte vectors per point, one per thread.
__global__ void agg_fix_zero_kernel(u32 n, const int8_t* __restrict__ zero, const uint4* __restrict__ fixed, uint4* __restrict__ pts, u32* __restrict__ flag) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (u64)n * 6) return;
  const VecPart v = vec_split(t, 6);
  if (zero[v.elem] != 1) return;
  pts[t] = fixed[v.part];
  if (flag && v.part == 0) atomicOr(flag, 1u);
}
}  // namespace

extern "C" {
int nbls_agg_keys_launch(unsigned nkeys, unsigned n, const uint32_t* koff, const uint32_t* index, const int8_t* st_src, uint32_t* set_id, uint32_t* rank, int8_t* st,
                         uint32_t* first_bad, hipStream_t stream) {
  if (!nkeys || !n) return 0;
  const hipError_t e = hipMemsetAsync(first_bad, 0xff, (size_t)n * 4, stream);
  return e != hipSuccess ? (int)e : launch_1d(agg_keys_kernel, nkeys, 256, 0, stream, nkeys, n, koff, index, st_src, set_id, rank, st, first_bad);
}
int nbls_agg_points_launch(size_t nkeys, unsigned elem_bytes, const uint32_t* index, const void* st, const void* ident, const void* src, void* dst, hipStream_t stream) {
  const u32 q = elem_bytes / 16;
  return launch_1d(agg_points_kernel, (u64)nkeys * q, 256, 0, stream, nkeys, q, index, st, ident, src, dst);
}
int nbls_agg_status_launch(unsigned n, const uint32_t* first_bad, const int8_t* st, const void* zero, void* out, hipStream_t stream) {
  return launch_1d(agg_status_kernel, n, 256, 0, stream, n, first_bad, st, zero, out);
}
int nbls_agg_fix_zero_launch(unsigned n, const void* zero, const void* fixed96, void* pts96, uint32_t* flag, hipStream_t stream) {
  return launch_1d(agg_fix_zero_kernel, (u64)n * 6, 256, 0, stream, n, zero, fixed96, pts96, flag);
}
}
