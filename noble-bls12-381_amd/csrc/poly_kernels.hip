// poly_kernels.hip -- the data movement of nbls_g*_poly_eval (pipelines_poly.cpp): which group every identifier belongs to, the coefficient every item of a slab meets in one
// Horner step, and the closing status kernel.  The curve arithmetic runs as step programs (the decoders, the Horner steps of programs.h ExtraProg, to-affine, compress);
// nothing here computes on curve points.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
typedef uint32_t u32;
typedef uint64_t u64;

// one thread per identifier k of the call: its group g (off[g] <= k < off[g + 1]; the ngroups + 1 offsets are relative and strictly increasing)
__global__ void __launch_bounds__(256) poly_group_kernel(u32 n, u32 ngroups, const u32* __restrict__ off, u32* __restrict__ group_of) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  u32 lo = 0, hi = ngroups;   // off[lo] <= k < off[hi]
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) >> 1;
    if (off[mid] <= k) lo = mid; else hi = mid;
  }
  group_of[k] = lo;
}

// Step j of a slab of `items` identifiers (group_of: the slab's first entry): dst[i] = coefficient j of item i's group, the identity when the group has no coefficient j (a
// shorter polynomial is aligned at the low end: with an identity accumulator and an identity coefficient the step is a no-op).  pts: the call's coefficients as raw projective
// points, coff: their ngroups + 1 relative offsets.  q = 16-byte vectors per point, one vector per thread.
__global__ void __launch_bounds__(256) poly_coef_kernel(u64 items, u32 q, u32 j, const u32* __restrict__ group_of, const u32* __restrict__ coff, const uint4* __restrict__ ident,
                                                        const uint4* __restrict__ pts, uint4* __restrict__ dst) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= items * q) return;
  const u64 i = t / q; const u32 part = (u32)(t - i * q);
  const u32 g = group_of[i], b = coff[g], e = coff[g + 1];
  dst[t] = j < e - b ? pts[(u64)(b + j) * q + part] : ident[part];
}

// status[k] = the decoder status of the first coefficient of k's group that did not decode, else 1 when F(x_k) is the zero point, else 0; the identifier's `e` output bytes
// (16-byte vectors) become 0xc0 00.. for status 1 and all-zero for a status >= 2
__global__ void __launch_bounds__(256) poly_status_kernel(u32 n, u32 e, const u32* __restrict__ group_of, const u32* __restrict__ first_bad, const int8_t* __restrict__ st,
                                                          const int8_t* __restrict__ zero, uint8_t* __restrict__ out, int8_t* __restrict__ status) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const u32 f = first_bad[group_of[k]];
  const int8_t v = f != 0xffffffffu ? st[f] : zero[k];
  status[k] = v;
  if (v) {
    uint4* o = (uint4*)(out + (u64)k * e);
    for (u32 w = 0; w < e / 16; w++) o[w] = make_uint4(w == 0 && v == 1 ? 0xc0u : 0u, 0u, 0u, 0u);
  }
}

inline unsigned blocks_for(u64 threads) { return (unsigned)((threads + 255) / 256); }
}  // namespace

extern "C" {
int nbls_poly_group_launch(unsigned n, unsigned ngroups, const void* off, void* group_of, void* stream) {
  if (!n || !ngroups) return 0;
  hipLaunchKernelGGL(poly_group_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, ngroups, (const u32*)off, (u32*)group_of);
  return (int)hipGetLastError();
}
int nbls_poly_coef_launch(size_t items, unsigned elem_bytes, unsigned j, const void* group_of, const void* coff, const void* ident, const void* pts, void* dst, void* stream) {
  if (!items) return 0;
  const u32 q = elem_bytes / 16;
  hipLaunchKernelGGL(poly_coef_kernel, dim3(blocks_for((u64)items * q)), dim3(256), 0, (hipStream_t)stream, (u64)items, q, j, (const u32*)group_of, (const u32*)coff,
                     (const uint4*)ident, (const uint4*)pts, (uint4*)dst);
  return (int)hipGetLastError();
}
int nbls_poly_status_launch(unsigned n, unsigned out_bytes, const void* group_of, const void* first_bad, const void* st, const void* zero, void* out, void* status, void* stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(poly_status_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, out_bytes, (const u32*)group_of, (const u32*)first_bad, (const int8_t*)st,
                     (const int8_t*)zero, (uint8_t*)out, (int8_t*)status);
  return (int)hipGetLastError();
}
}
