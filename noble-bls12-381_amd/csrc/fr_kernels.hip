// fr_kernels.hip -- the scalar field on the device (fr_exec.h: the arithmetic, written once and shared with the simulator) and the data movement of threshold recombination
// (pipelines_threshold.cpp): elementwise Fr operations, conversion between wire bytes and Montgomery form, the Lagrange coefficients at zero of contiguous groups, and the
// closing status kernel of nbls_g*_combine_shares.  The curve arithmetic of the recombination runs as step programs (the decoders, the ladders, the segmented sum).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_exec.h"
#include "nbls.h"   // NBLS_ST_BAD_IDS
#include "kernel_parts.h"
#include "launchers.h"

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
// not decode, else 1 when the combination is the zero point, else 0; the group's `e` output bytes are closed by the status (kernel_parts.h close_compressed)
__global__ void fr_combine_status_kernel(u32 ngroups, u32 e, const u32* __restrict__ bad_group, const u32* __restrict__ first_bad, const int8_t* __restrict__ st,
                                         const int8_t* __restrict__ zero, uint8_t* __restrict__ out, int8_t* __restrict__ status) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  int8_t v = NBLS_ST_BAD_IDS;
  if (!bad_group[g]) { const u32 f = first_bad[g]; v = f != 0xffffffffu ? st[f] : zero[g]; }
  status[g] = v;
  close_compressed(out + (u64)g * e, e, v);
}

// status[g] = NBLS_ST_BAD_IDS for a flagged group, else 0 (nbls_lagrange_at_zero)
__global__ void fr_group_status_kernel(u32 ngroups, const u32* __restrict__ bad_group, int8_t* __restrict__ status) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < ngroups) status[g] = bad_group[g] ? NBLS_ST_BAD_IDS : 0;
}

}  // namespace

extern "C" {
int nbls_fr_op_launch(unsigned n, int op, const void* a32, const void* b32, void* out32, void* status, hipStream_t stream) {
  return launch_1d(fr_op_kernel, n, 64, 0, stream, n, op, a32, b32, out32, status);
}
// ids32: n identifiers (wire bytes) in ngroups contiguous groups -> out32: n canonical coefficients; X, L: n Montgomery elements each; group_of: n words; bad_group: ngroups words
int nbls_fr_lagrange_launch(unsigned n, unsigned ngroups, const uint32_t* off, const void* ids32, void* X, void* L, uint32_t* group_of, uint32_t* bad_group, void* out32,
                            hipStream_t stream) {
  if (!n || !ngroups) return 0;
  int e = (int)hipMemsetAsync(bad_group, 0, (size_t)ngroups * 4, stream);
  if (!e) e = launch_1d(fr_to_mont_kernel, n, 256, 0, stream, n, ids32, X);
  if (!e) e = launch_1d(fr_lagrange_kernel, n, LAG_BLOCK, 0, stream, n, ngroups, off, X, L, group_of, bad_group);
  if (!e) e = launch_1d(fr_lagrange_out_kernel, n, 256, 0, stream, n, L, group_of, bad_group, out32);
  return e;
}
int nbls_fr_combine_status_launch(unsigned ngroups, unsigned out_bytes, const uint32_t* bad_group, const uint32_t* first_bad, const int8_t* st, const void* zero, void* out,
                                  void* status, hipStream_t stream) {
  return launch_1d(fr_combine_status_kernel, ngroups, 256, 0, stream, ngroups, out_bytes, bad_group, first_bad, st, zero, out, status);
}
int nbls_fr_group_status_launch(unsigned ngroups, const uint32_t* bad_group, void* status, hipStream_t stream) {
  return launch_1d(fr_group_status_kernel, ngroups, 256, 0, stream, ngroups, bad_group, status);
}
}
