// rlc_kernels.hip -- the data movement of nbls_verify_multiple (pipelines_multi_verify.cpp): the secret weights of the random linear combination, the interleaved pair layout
// of the per-set pass, and the per-set comparison of the final exponentiations with one.  The group and field arithmetic runs as step programs (P_G1_MUL64, the MSM, the Miller
// loops); nothing here computes on curve points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rlc_weights.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;

// out[32 i ..] = r_i (rlc_weights.h), one thread per set: a single SHA-256 block each
__global__ void rlc_weights_kernel(u32 n, const uint8_t* __restrict__ seed32, uint8_t* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  nbls::rlc_weight(seed32, (u64)i, out + 32ull * i);
}

// the per-set pass runs P_MILLER_RAW2 (two pairs per item) over records g1x[i] = pk_i || -G1 (192 B) and g2x[i] = H(m_i) || sig_i (384 B), 16-byte vectors, one per thread
__global__ void rlc_interleave_kernel(u32 n, const uint4* __restrict__ pk, const uint4* __restrict__ neg_g1, const uint4* __restrict__ h, const uint4* __restrict__ sig,
                                      uint4* __restrict__ g1x, uint4* __restrict__ g2x) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (u64)n * 36) return;
  const u64 i = t / 36; const u32 part = (u32)(t - i * 36);
  if (part < 12) g1x[i * 12 + part] = part < 6 ? pk[i * 6 + part] : neg_g1[part - 6];
  else { const u32 q = part - 12; g2x[i * 24 + q] = q < 12 ? h[i * 12 + q] : sig[i * 12 + q - 12]; }
}

// ok[i] = 1 when the 576 wire bytes of item i are Fp12.ONE (byte 47 = 1, every other byte 0: fp12_wire_is_one in pipelines_verify.cpp), else 0
__global__ void rlc_is_one_kernel(u32 n, const uint4* __restrict__ f, uint8_t* __restrict__ ok) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 acc = 0;
  for (int k = 0; k < 36; k++) {
    const uint4 v = f[36ull * i + k];
    acc |= v.x | v.y | v.z | (k == 2 ? v.w ^ 0x01000000u : v.w);
  }
  ok[i] = acc == 0;
}

inline unsigned blocks_for(u64 threads) { return (unsigned)((threads + 255) / 256); }
}  // namespace

extern "C" {
int nbls_rlc_weights_launch(unsigned n, const void* seed32, void* out, void* stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(rlc_weights_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, (const uint8_t*)seed32, (uint8_t*)out);
  return (int)hipGetLastError();
}
int nbls_rlc_interleave_launch(unsigned n, const void* pk96, const void* neg_g1, const void* h192, const void* sig192, void* g1x, void* g2x, void* stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(rlc_interleave_kernel, dim3(blocks_for((u64)n * 36)), dim3(256), 0, (hipStream_t)stream, n, (const uint4*)pk96, (const uint4*)neg_g1, (const uint4*)h192,
                     (const uint4*)sig192, (uint4*)g1x, (uint4*)g2x);
  return (int)hipGetLastError();
}
int nbls_rlc_is_one_launch(unsigned n, const void* f576, void* ok, void* stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(rlc_is_one_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, (const uint4*)f576, (uint8_t*)ok);
  return (int)hipGetLastError();
}
}
