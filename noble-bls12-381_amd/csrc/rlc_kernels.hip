// rlc_kernels.hip -- the data movement of nbls_verify_multiple (pipelines_multi_verify.cpp): the secret weights of the random linear combination, the interleaved pair layout
// of the per-set pass (one hash per set or, through a message index, one per message: the shared-message forms), and the per-set comparison of the final exponentiations
// with one.  The group and field arithmetic runs as step programs (P_G1_MUL64, the MSM, the Miller loops); nothing here computes on curve points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rlc_weights.h"
#include "kernel_parts.h"
#include "launchers.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

// out[32 i ..] = r_i (rlc_weights.h), one thread per set: a single SHA-256 block each
__global__ void rlc_weights_kernel(u32 n, const uint8_t* __restrict__ seed32, uint8_t* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  nbls::rlc_weight(seed32, (u64)i, out + 32ull * i);
}

// the per-set pass runs P_MILLER_RAW2 (two pairs per item) over records g1x[i] = pk_i || -G1 (192 B) and g2x[i] = H || sig_i (384 B), 16-byte vectors, one per thread.  H = h[i], one
// hash per set, or with a message index (the shared-message forms) h[idx[i]], one hash per MESSAGE; idx[i] < the number of messages was checked on the host
__global__ void rlc_interleave_kernel(u32 n, const u32* __restrict__ idx, const uint4* __restrict__ pk, const uint4* __restrict__ neg_g1, const uint4* __restrict__ h,
                                      const uint4* __restrict__ sig, uint4* __restrict__ g1x, uint4* __restrict__ g2x) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (u64)n * 36) return;
  const VecPart v = vec_split(t, 36);
  const u64 i = v.elem; const u32 part = v.part;
  if (part < 12) g1x[i * 12 + part] = part < 6 ? pk[i * 6 + part] : neg_g1[part - 6];
  else { const u32 q = part - 12; g2x[i * 24 + q] = q < 12 ? h[(idx ? (u64)idx[i] : i) * 12 + q] : sig[i * 12 + q - 12]; }
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

}  // namespace

extern "C" {
int nbls_rlc_weights_launch(unsigned n, const void* seed32, void* out, hipStream_t stream) { return launch_1d(rlc_weights_kernel, n, 256, 0, stream, n, seed32, out); }
int nbls_rlc_interleave_launch(unsigned n, const uint32_t* msg_index, const void* pk96, const void* neg_g1, const void* h192, const void* sig192, void* g1x, void* g2x,
                               hipStream_t stream) {
  return launch_1d(rlc_interleave_kernel, (u64)n * 36, 256, 0, stream, n, msg_index, pk96, neg_g1, h192, sig192, g1x, g2x);
}
int nbls_rlc_is_one_launch(unsigned n, const void* f576, void* ok, hipStream_t stream) { return launch_1d(rlc_is_one_kernel, n, 256, 0, stream, n, f576, ok); }
}
