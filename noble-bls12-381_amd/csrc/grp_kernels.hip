// grp_kernels.hip -- the data movement of the shared-message entry points (nbls_verify_multiple_shared and its twins, pipelines_multi_verify.cpp) that the kernels of
// agg_kernels.hip / msm_kernels.hip do not cover already: the flag for a message group whose weighted keys sum to the zero point, and the per-set pass's pair layout with
// H(m) gathered through the message index.  The ordered gather of the ladder's outputs IS agg_points_kernel (index = the sets in group order, statuses in group order from
// agg_keys_kernel); the sums are the MSM's list-driven rounds.  Nothing here computes on curve points.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
typedef uint32_t u32;
typedef uint64_t u64;

// zero[g] != 0 (P_G1_TO_AFFINE's flag: group g's weighted keys sum to the zero point): *flag = 1 and rpk[g] = `fixed`, a valid affine point, so that the Miller loop the pair
// still runs through works on a curve point; the combined result is not counted then.  Six 16-byte vectors per point, one per thread.
__global__ void grp_zero_kernel(u32 m, const int8_t* __restrict__ zero, const uint4* __restrict__ fixed, uint4* __restrict__ rpk, u32* __restrict__ flag) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (u64)m * 6) return;
  const u64 g = t / 6; const u32 part = (u32)(t - g * 6);
  if (!zero[g]) return;
  rpk[t] = fixed[part];
  if (part == 0) atomicOr(flag, 1u);
}

// rlc_interleave_kernel (rlc_kernels.hip) with one H per MESSAGE: g1x[i] = pk_i || -G1 (192 B), g2x[i] = h[idx[i]] || sig_i (384 B); idx[i] < the number of messages was checked
// on the host.  16-byte vectors, one per thread.
__global__ void grp_interleave_kernel(u32 n, const u32* __restrict__ idx, const uint4* __restrict__ pk, const uint4* __restrict__ neg_g1, const uint4* __restrict__ h,
                                      const uint4* __restrict__ sig, uint4* __restrict__ g1x, uint4* __restrict__ g2x) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (u64)n * 36) return;
  const u64 i = t / 36; const u32 part = (u32)(t - i * 36);
  if (part < 12) g1x[i * 12 + part] = part < 6 ? pk[i * 6 + part] : neg_g1[part - 6];
  else { const u32 q = part - 12; g2x[i * 24 + q] = q < 12 ? h[(u64)idx[i] * 12 + q] : sig[i * 12 + q - 12]; }
}

inline unsigned blocks_for(u64 threads) { return (unsigned)((threads + 255) / 256); }
}  // namespace

extern "C" {
int nbls_grp_zero_launch(unsigned m, const void* zero, const void* fixed96, void* rpk96, void* flag_u32, void* stream) {
  if (!m) return 0;
  hipLaunchKernelGGL(grp_zero_kernel, dim3(blocks_for((u64)m * 6)), dim3(256), 0, (hipStream_t)stream, m, (const int8_t*)zero, (const uint4*)fixed96, (uint4*)rpk96, (u32*)flag_u32);
  return (int)hipGetLastError();
}
int nbls_grp_interleave_launch(unsigned n, const void* msg_index, const void* pk96, const void* neg_g1, const void* h192, const void* sig192, void* g1x, void* g2x, void* stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(grp_interleave_kernel, dim3(blocks_for((u64)n * 36)), dim3(256), 0, (hipStream_t)stream, n, (const u32*)msg_index, (const uint4*)pk96, (const uint4*)neg_g1,
                     (const uint4*)h192, (const uint4*)sig192, (uint4*)g1x, (uint4*)g2x);
  return (int)hipGetLastError();
}
}
