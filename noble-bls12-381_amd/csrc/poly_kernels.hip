// poly_kernels.hip -- the data movement of nbls_g*_poly_eval (pipelines_poly.cpp): which group every identifier belongs to, the coefficient every item of a slab meets in one
// Horner step, and the closing status kernel.  The curve arithmetic runs as step programs (the decoders, the Horner steps of programs.h ExtraProg, to-affine, compress);
// nothing here computes on curve points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "group_search.h"
#include "kernel_parts.h"
#include "launchers.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

// one thread per identifier k of the call: its group g (off[g] <= k < off[g + 1]; the ngroups + 1 offsets are relative and strictly increasing)
__global__ void __launch_bounds__(256) poly_group_kernel(u32 n, u32 ngroups, const u32* __restrict__ off, u32* __restrict__ group_of) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) group_of[k] = group_search(off, 0, ngroups, k);
}

// Step j of a slab of `items` identifiers (group_of: the slab's first entry): dst[i] = coefficient j of item i's group, the identity when the group has no coefficient j (a
// shorter polynomial is aligned at the low end: with an identity accumulator and an identity coefficient the step is a no-op).  pts: the call's coefficients as raw projective
// points, coff: their ngroups + 1 relative offsets.  q = 16-byte vectors per point, one vector per thread.
__global__ void __launch_bounds__(256) poly_coef_kernel(u64 items, u32 q, u32 j, const u32* __restrict__ group_of, const u32* __restrict__ coff, const uint4* __restrict__ ident,
                                                        const uint4* __restrict__ pts, uint4* __restrict__ dst) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= items * q) return;
  const VecPart v = vec_split(t, q);
  const u32 g = group_of[v.elem], b = coff[g], e = coff[g + 1];
  dst[t] = j < e - b ? pts[(u64)(b + j) * q + v.part] : ident[v.part];
}

// status[k] = the decoder status of the first coefficient of k's group that did not decode, else 1 when F(x_k) is the zero point, else 0; the identifier's `e` output bytes
// are closed by the status (kernel_parts.h close_compressed)
__global__ void __launch_bounds__(256) poly_status_kernel(u32 n, u32 e, const u32* __restrict__ group_of, const u32* __restrict__ first_bad, const int8_t* __restrict__ st,
                                                          const int8_t* __restrict__ zero, uint8_t* __restrict__ out, int8_t* __restrict__ status) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const u32 f = first_bad[group_of[k]];
  const int8_t v = f != 0xffffffffu ? st[f] : zero[k];
  status[k] = v;
  close_compressed(out + (u64)k * e, e, v);
}

}  // namespace

extern "C" {
int nbls_poly_group_launch(unsigned n, unsigned ngroups, const uint32_t* off, uint32_t* group_of, hipStream_t stream) {
  return launch_1d(poly_group_kernel, ngroups ? n : 0, 256, 0, stream, n, ngroups, off, group_of);
}
int nbls_poly_coef_launch(size_t items, unsigned elem_bytes, unsigned j, const uint32_t* group_of, const uint32_t* coff, const void* ident, const void* pts, void* dst,
                          hipStream_t stream) {
  const u32 q = elem_bytes / 16;
  return launch_1d(poly_coef_kernel, (u64)items * q, 256, 0, stream, items, q, j, group_of, coff, ident, pts, dst);
}
int nbls_poly_status_launch(unsigned n, unsigned out_bytes, const uint32_t* group_of, const uint32_t* first_bad, const int8_t* st, const void* zero, void* out, void* status,
                            hipStream_t stream) {
  return launch_1d(poly_status_kernel, n, 256, 0, stream, n, out_bytes, group_of, first_bad, st, zero, out, status);
}
}
