// agg_kernels.hip -- the data movement of nbls_verify_aggregates (pipelines_multi_verify.cpp): which set every key belongs to, the identity in place of the keys that add
// nothing, the gather from a key table (nbls_keyset), and one status byte per set.  The additions themselves are the MSM's list-driven rounds (msm_kernels.hip msm_pairs_kernel +
// P_G1_ADD_AB); nothing here computes on curve points.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
typedef uint32_t u32;
typedef uint64_t u64;

// one thread per key k of the call: its set j (koff[j] <= k < koff[j + 1]; the n + 1 offsets are relative and, sets being non-empty, strictly increasing), its rank in the set,
// its status (st_src[index[k]] from a key table, st_src[k] without an index), and first_bad[j] = the lowest k of set j whose status is >= 2 (a key that did not decode)
__global__ void agg_keys_kernel(u32 nkeys, u32 n, const u32* __restrict__ koff, const u32* __restrict__ index, const int8_t* __restrict__ st_src, u32* __restrict__ set_id,
                                u32* __restrict__ rank, int8_t* __restrict__ st, u32* __restrict__ first_bad) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  u32 lo = 0, hi = n;   // koff[lo] <= k < koff[hi]
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (koff[mid] <= k) lo = mid; else hi = mid;
  }
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
  const u64 k = t / q; const u32 part = (u32)(t - k * q);
  dst[t] = st[k] ? ident[part] : src[(index ? (u64)index[k] : k) * q + part];
}

// out[j] = the status of set j's first key that did not decode, else the aggregate's (1 when the keys sum to the zero point, 0 otherwise)
__global__ void agg_status_kernel(u32 n, const u32* __restrict__ first_bad, const int8_t* __restrict__ st, const int8_t* __restrict__ zero, int8_t* __restrict__ out) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u32 f = first_bad[j];
  out[j] = f != 0xffffffffu ? st[f] : zero[j];
}

inline unsigned blocks_for(u64 threads) { return (unsigned)((threads + 255) / 256); }
}  // namespace

extern "C" {
int nbls_agg_keys_launch(unsigned nkeys, unsigned n, const void* koff, const void* index, const void* st_src, void* set_id, void* rank, void* st, void* first_bad, void* stream) {
  if (!nkeys || !n) return 0;
  const hipError_t e = hipMemsetAsync(first_bad, 0xff, (size_t)n * 4, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(agg_keys_kernel, dim3(blocks_for(nkeys)), dim3(256), 0, (hipStream_t)stream, nkeys, n, (const u32*)koff, (const u32*)index, (const int8_t*)st_src, (u32*)set_id,
                     (u32*)rank, (int8_t*)st, (u32*)first_bad);
  return (int)hipGetLastError();
}
int nbls_agg_points_launch(size_t nkeys, unsigned elem_bytes, const void* index, const void* st, const void* ident, const void* src, void* dst, void* stream) {
  if (!nkeys) return 0;
  const u32 q = elem_bytes / 16;
  hipLaunchKernelGGL(agg_points_kernel, dim3(blocks_for((u64)nkeys * q)), dim3(256), 0, (hipStream_t)stream, (u64)nkeys, q, (const u32*)index, (const int8_t*)st, (const uint4*)ident,
                     (const uint4*)src, (uint4*)dst);
  return (int)hipGetLastError();
}
int nbls_agg_status_launch(unsigned n, const void* first_bad, const void* st, const void* zero, void* out, void* stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(agg_status_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, (const u32*)first_bad, (const int8_t*)st, (const int8_t*)zero, (int8_t*)out);
  return (int)hipGetLastError();
}
}
