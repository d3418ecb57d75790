// fr_kernels.hip -- the scalar field on the device (fr_exec.h: the arithmetic, written once and shared with the simulator) and the data movement of threshold recombination
// (pipelines_threshold.cpp): elementwise Fr operations, conversion between wire bytes and Montgomery form, the Lagrange coefficients at zero of contiguous groups, and the
// closing status kernel of nbls_g*_combine_shares.  The curve arithmetic of the recombination runs as step programs (the decoders, the ladders, the segmented sum).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_exec.h"
#include "nbls.h"   // NBLS_ST_BAD_IDS

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

constexpr int LAG_BLOCK = 64;   // one wavefront per workgroup: a tile is 64 identifiers, the loop bounds below are the wavefront's own

// nbls_fr_op_batch: one element per lane, wire bytes in and out
__global__ void __launch_bounds__(64) fr_op_kernel(u32 n, int op, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint8_t* __restrict__ out, int8_t* __restrict__ status) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  status[i] = (int8_t)fr_op_bytes(op, a + 32ull * i, b ? b + 32ull * i : a + 32ull * i, out + 32ull * i);
}

// 32 bytes big-endian (any value) -> Montgomery limbs; the way back to canonical bytes is fr_lagrange_out_kernel's
__global__ void fr_to_mont_kernel(u32 n, const uint8_t* __restrict__ in, Fr* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fr_from_bytes(in + 32ull * i);
}

// One share per lane: share k of group g (off[g] <= k < off[g + 1]; ngroups + 1 relative, strictly increasing offsets) gets lambda_k in Montgomery form, its group, and the
// group's flag is raised when x_k = 0 or x_k equals another identifier of the group.  The groups are contiguous, so the identifiers a wavefront needs are ONE range: from the
// start of its first lane's group to the end of its last lane's.  The range passes through LDS in tiles of 64 (every lane stages one identifier), and every lane then reads
// identifier j of the tile from the same address -- a broadcast, no bank conflict -- and folds it into its products under a mask that says whether j lies in the lane's own
// group and whether it is the lane's own share.  The loop bounds are the wavefront's, never a lane's: lanes past n run along with the last share's group and store nothing.
__global__ void __launch_bounds__(LAG_BLOCK) fr_lagrange_kernel(u32 n, u32 ngroups, const u32* __restrict__ off, const Fr* __restrict__ x, Fr* __restrict__ lambda,
                                                               u32* __restrict__ group_of, u32* __restrict__ bad_group) {
  __shared__ Fr tile[LAG_BLOCK];
  __shared__ u32 range[2];
  const u32 k0 = blockIdx.x * LAG_BLOCK, k = k0 + threadIdx.x, kk = k < n ? k : n - 1;
  const u32 g = fr_group_of(off, ngroups, kk), gb = off[g], ge = off[g + 1];
  if (threadIdx.x == 0) range[0] = gb;
  if (threadIdx.x == LAG_BLOCK - 1) range[1] = ge;
  FrLagrange s = fr_lagrange_begin(x[kk]);
  __syncthreads();
  const u32 rb = range[0], re = range[1];
  for (u32 t = rb; t < re; t += LAG_BLOCK) {
    const u32 j = t + threadIdx.x;
    tile[threadIdx.x] = x[j < re ? j : re - 1];
    __syncthreads();
    const u32 cnt = re - t < (u32)LAG_BLOCK ? re - t : (u32)LAG_BLOCK;
    fr_lagrange_tile(s, tile, t, cnt, gb, ge, kk);
    __syncthreads();
  }
  u32 bad;
  const Fr l = fr_lagrange_finish(s, &bad);
  if (k < n) {
    lambda[k] = l;
    group_of[k] = g;
    if (bad) atomicOr(&bad_group[g], 1u);
  }
}

// lambda (Montgomery) -> canonical 32-byte big-endian scalars, all-zero for the shares of a flagged group
__global__ void fr_lagrange_out_kernel(u32 n, const Fr* __restrict__ lambda, const u32* __restrict__ group_of, const u32* __restrict__ bad_group, uint8_t* __restrict__ out) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const Fr v = fr_from_mont(lambda[k]);
  fr_store_be(fr_select((u32)0 - (u32)(bad_group[group_of[k]] != 0), fr_zero(), v), out + 32ull * k);
}

// status[g] = NBLS_ST_BAD_IDS for a flagged group, else the decoder status of the group's first share that did
// not decode, else 1 when the combination is the zero point, else 0; the group's `e` output bytes (16-byte vectors) become 0xc0 00.. for status 1 and all-zero for a status >= 2
__global__ void fr_combine_status_kernel(u32 ngroups, u32 e, const u32* __restrict__ bad_group, const u32* __restrict__ first_bad, const int8_t* __restrict__ st,
                                         const int8_t* __restrict__ zero, uint8_t* __restrict__ out, int8_t* __restrict__ status) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  int8_t v = NBLS_ST_BAD_IDS;
  if (!bad_group[g]) { const u32 f = first_bad[g]; v = f != 0xffffffffu ? st[f] : zero[g]; }
  status[g] = v;
  if (v) {
    uint4* o = (uint4*)(out + (u64)g * e);
    for (u32 q = 0; q < e / 16; q++) o[q] = make_uint4(q == 0 && v == 1 ? 0xc0u : 0u, 0u, 0u, 0u);
  }
}

// status[g] = NBLS_ST_BAD_IDS for a flagged group, else 0 (nbls_lagrange_at_zero)
__global__ void fr_group_status_kernel(u32 ngroups, const u32* __restrict__ bad_group, int8_t* __restrict__ status) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < ngroups) status[g] = bad_group[g] ? NBLS_ST_BAD_IDS : 0;
}

inline unsigned blocks_for(u64 threads, unsigned per = 256) { return (unsigned)((threads + per - 1) / per); }
}  // namespace

extern "C" {
int nbls_fr_op_launch(unsigned n, int op, const void* a32, const void* b32, void* out32, void* status, void* stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(fr_op_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, (hipStream_t)stream, n, op, (const uint8_t*)a32, (const uint8_t*)b32, (uint8_t*)out32, (int8_t*)status);
  return (int)hipGetLastError();
}
// ids32: n identifiers (wire bytes) in ngroups contiguous groups -> out32: n canonical coefficients; X, L: n Montgomery elements each; group_of: n words; bad_group: ngroups words
int nbls_fr_lagrange_launch(unsigned n, unsigned ngroups, const void* off, const void* ids32, void* X, void* L, void* group_of, void* bad_group, void* out32, void* stream) {
  if (!n || !ngroups) return 0;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(bad_group, 0, (size_t)ngroups * 4, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(fr_to_mont_kernel, dim3(blocks_for(n)), dim3(256), 0, s, n, (const uint8_t*)ids32, (Fr*)X);
  hipLaunchKernelGGL(fr_lagrange_kernel, dim3(blocks_for(n, LAG_BLOCK)), dim3(LAG_BLOCK), 0, s, n, ngroups, (const u32*)off, (const Fr*)X, (Fr*)L, (u32*)group_of, (u32*)bad_group);
  hipLaunchKernelGGL(fr_lagrange_out_kernel, dim3(blocks_for(n)), dim3(256), 0, s, n, (const Fr*)L, (const u32*)group_of, (const u32*)bad_group, (uint8_t*)out32);
  return (int)hipGetLastError();
}
int nbls_fr_combine_status_launch(unsigned ngroups, unsigned out_bytes, const void* bad_group, const void* first_bad, const void* st, const void* zero, void* out, void* status,
                                  void* stream) {
  if (!ngroups) return 0;
  hipLaunchKernelGGL(fr_combine_status_kernel, dim3(blocks_for(ngroups)), dim3(256), 0, (hipStream_t)stream, ngroups, out_bytes, (const u32*)bad_group, (const u32*)first_bad,
                     (const int8_t*)st, (const int8_t*)zero, (uint8_t*)out, (int8_t*)status);
  return (int)hipGetLastError();
}
int nbls_fr_group_status_launch(unsigned ngroups, const void* bad_group, void* status, void* stream) {
  if (!ngroups) return 0;
  hipLaunchKernelGGL(fr_group_status_kernel, dim3(blocks_for(ngroups)), dim3(256), 0, (hipStream_t)stream, ngroups, (const u32*)bad_group, (int8_t*)status);
  return (int)hipGetLastError();
}
}
