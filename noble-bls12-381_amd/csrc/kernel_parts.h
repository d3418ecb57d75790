// kernel_parts.h -- what the data-movement kernel files share on the device side (rlc / agg / fr / poly / kzg / msm _kernels.hip, and the launchers of xmd / pow / vm_wide):
// the one-thread-per-unit launch, the split of a thread index into (element, 16-byte part), and the closing of a compressed result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbls {
// One thread per unit: nothing for zero units, else ceil(units / block) workgroups of `block` threads; the launch's error code.  The arguments are converted to the kernel's
// own parameter types here, so a launcher passes its void* through.
template <class... P, class... A>
inline int launch_1d(void (*kernel)(P...), uint64_t units, unsigned block, unsigned lds_bytes, hipStream_t s, A... a) {
  if (!units) return 0;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((units + block - 1) / block)), dim3(block), lds_bytes, s, (P)a...);
  return (int)hipGetLastError();
}

// thread t of a kernel that moves elements of q 16-byte vectors, one vector per thread, consecutive threads on consecutive vectors of one element (coalesced)
struct VecPart { uint64_t elem; uint32_t part; };
__device__ inline VecPart vec_split(uint64_t t, uint32_t q) {
  const uint64_t e = t / q;
  return VecPart{e, (uint32_t)(t - e * q)};
}

// the `e` bytes (16-byte vectors) of a compressed point whose status is not 0: 0xc0 00.. for the zero point (status 1), all-zero bytes for anything else (nothing was computed)
__device__ inline void close_compressed(uint8_t* out, uint32_t e, int status) {
  if (!status) return;
  uint4* o = (uint4*)out;
  for (uint32_t w = 0; w < e / 16; w++) o[w] = make_uint4(w == 0 && status == 1 ? 0xc0u : 0u, 0u, 0u, 0u);
}
}  // namespace nbls
