// msm_kernels.hip -- data movement of the multi-scalar multiplication sum_i [k_i]P_i (bucket method), for one sum and for many
// independent sums that share every launch (pipelines_msm.cpp: bucket_slices).  The group arithmetic itself runs as wave-VM step programs
// (P_G*_ADD_AB, P_G*_ADD2, P_G*_HORNER, P_G*_SHIFTADD, XP_DBLADD_G*); the kernels here only decide WHICH points meet: window digits of the
// scalars, a device radix sort of the keys (hipCUB), and gathers by index.  The window width c is a run-time argument, and every key carries
// the sum it belongs to:
//   key = (group * nwin + window) << c | digit
// so a run of equal keys never crosses a group, and the key is at the same time the index of its bucket; the single sum is one group with c = 12.
// Points are raw projective elements of E = 192 (G1) or 384 (G2) bytes, moved as 16-byte vectors, one vector per thread, consecutive threads
// on consecutive vectors of the same point (coalesced).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "scalar_split.h"
#include "group_search.h"
#include "kernel_parts.h"
#include "launchers.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

// One thread per item e of a slab: scalar i = i0 + e / dims of the call, part d = e % dims of its split (dims = 1: unsplit; the split scalars lie dims * 32 bytes per scalar;
// scalars are 32-byte big-endian integers).  The item's group is found in the call's offsets (off[0 .. ngroups], relative to the first scalar; empty groups own nothing), or
// is i / n_pts in the rows form (n_pts > 0), where the point is i % n_pts and off is not read.  keys[w * m + e] = ((group - g0) * nwin + w) << c | digit_w,
// vals[w * m + e] = point * dims + d (the index of the converted point).  The single sum: i0 = g0 = 0 and n_pts = its points, so group 0, key = w << c | digit_w, val = e.
// The rows form is the case glen = n_pts, pt_block = k_mod = 0 of a wider map (the two passes of the FK20 cell proofs, pipelines_kzg_cells.cpp): the group is i / glen, the
// point i % n_pts, moved on by n_pts for every pt_block scalars (pt_block > 0: block b of the scalars meets points b n_pts ..), and the scalar read is i % k_mod (k_mod > 0: one
// array of k_mod scalars serves every block)
__global__ void msm_keys_kernel(u32 m, u32 dims, u32 nwin, u32 c, u32 i0, u32 g0, u32 ngroups, u32 n_pts, u32 glen, u32 pt_block, u32 k_mod, const u32* __restrict__ off,
                                const uint8_t* __restrict__ scalars, u32* __restrict__ keys, u32* __restrict__ vals) {
  const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const u32 i = i0 + e / dims, d = e % dims;
  u32 g, pt;
  if (n_pts) { g = i / glen; pt = i % n_pts + (pt_block ? (i / pt_block) * n_pts : 0u); }
  else { g = group_search(off, g0, ngroups, i); pt = i; }   // off[g0] <= i holds for every item of the slab
  const u32* k = (const u32*)(scalars + 32ull * ((u64)(k_mod ? i % k_mod : i) * dims + d));
  u32 w[9];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(k[7 - j]);
  w[8] = 0;
  const u32 base = (g - g0) * nwin, val = pt * dims + d, mask = (1u << c) - 1;
  for (u32 win = 0; win < nwin; win++) {
    const u32 bit = c * win, word = bit >> 5, o = bit & 31;
    const u64 v = (u64)w[word] | ((u64)w[word + 1] << 32);
    keys[(u64)win * m + e] = ((base + win) << c) | ((u32)(v >> o) & mask);
    vals[(u64)win * m + e] = val;
  }
}

// Scalar decomposition for the endomorphism split and its sign-aligned recoding: scalar_split.h (written once, compiled here and into the test-only simulator).
__global__ void msm_decompose_kernel(u32 n, u32 dims, const uint8_t* __restrict__ scalars, uint8_t* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  nbls::scalar_decompose(scalars + 32ull * i, dims, out + 32ull * dims * i);
}
__global__ void msm_sac_kernel(u32 n, const uint8_t* __restrict__ scalars, uint8_t* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  nbls::scalar_sac_recode(scalars + 32ull * i, out + 128ull * i);
}

// dst[j] = src[idx[j]]   (q = 16-byte vectors per element)
__global__ void msm_gather_kernel(u64 m, u32 q, const u32* __restrict__ idx, const uint4* __restrict__ src, uint4* __restrict__ dst) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * q) return;
  const VecPart v = vec_split(t, q);
  dst[t] = src[(u64)idx[v.elem] * q + v.part];
}

// rank of every element inside its run of equal keys: starts[j] = j at the head of a run, else 0; an inclusive max-scan (hipCUB)
// turns that into the index of the run's head, rank = j - head.  The last element of a run reports the run length; the longest
// run bounds the number of rounds of the segmented sum.
__global__ void msm_heads_flag_kernel(u64 m, const u32* __restrict__ keys, u32* __restrict__ starts) {
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  starts[j] = (j > 0 && keys[j - 1] != keys[j]) ? (u32)j : 0u;
}
__global__ void msm_rank_kernel(u64 m, const u32* __restrict__ keys, u32* __restrict__ pos /* in: head index, out: rank */, u32* __restrict__ maxrun) {
  __shared__ u32 blockmax;                       // one global atomic per workgroup (same-address atomics serialise: one per run cost 0.24 ms at 90 k runs)
  if (threadIdx.x == 0) blockmax = 0;
  __syncthreads();
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) {
    const u32 r = (u32)j - pos[j];
    pos[j] = r;
    if (j + 1 == m || keys[j + 1] != keys[j]) atomicMax(&blockmax, r + 1);
  }
  __syncthreads();
  if (threadIdx.x == 0 && blockmax) atomicMax(maxrun, blockmax);
}

// Segmented sum over the sorted list as a balanced tree inside every run: in the round with stride d the elements whose rank
// is a multiple of 2d absorb the element d places further on (when it is in the same run).  This kernel lists those
// elements (ballot + prefix counts); the addition program then addresses its operands through the list (KernelArgs.item_index).
// The order of the list is irrelevant: every pair is independent.
__global__ void __launch_bounds__(1024) msm_pairs_kernel(u64 m, u32 d, const u32* __restrict__ keys, const u32* __restrict__ pos, u32* __restrict__ list, u32* __restrict__ count) {
  // 4096 elements per workgroup, ONE global atomic per workgroup (same-address atomics serialise: one per wavefront cost 1.5 ms at 2^24 elements)
  __shared__ u32 wbase[4][16];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 j0 = (u64)blockIdx.x * 4096 + tid;
  bool act[4]; u64 mask[4];
#pragma unroll
  for (int it = 0; it < 4; it++) {
    const u64 j = j0 + it * 1024;
    act[it] = false;
    if (j < m && (pos[j] & (2 * d - 1)) == 0 && j + d < m) act[it] = keys[j + d] == keys[j];
    mask[it] = __ballot(act[it]);
    if (lane == 0) wbase[it][wave] = (u32)__popcll(mask[it]);
  }
  __syncthreads();
  if (tid == 0) {
    u32 tot = 0;
    for (int it = 0; it < 4; it++) for (int w = 0; w < 16; w++) { const u32 c = wbase[it][w]; wbase[it][w] = tot; tot += c; }
    const u32 g = tot ? atomicAdd(count, tot) : 0;
    for (int it = 0; it < 4; it++) for (int w = 0; w < 16; w++) wbase[it][w] += g;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 4; it++)
    if (act[it]) list[wbase[it][wave] + (u32)__popcll(mask[it] & ((1ull << lane) - 1))] = (u32)(j0 + it * 1024);
}

__global__ void msm_fill_kernel(u64 count, u32 q, const uint4* __restrict__ ident, uint4* __restrict__ dst) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * q) return;
  dst[t] = ident[vec_split(t, q).part];
}

// buckets[key] = P[j] for the head j of every run
__global__ void msm_heads_kernel(u64 m, u32 q, const u32* __restrict__ keys, const uint4* __restrict__ P, uint4* __restrict__ buckets) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * q) return;
  const VecPart v = vec_split(t, q);
  const u32 key = keys[v.elem];
  if (v.elem > 0 && keys[v.elem - 1] == key) return;
  buckets[(u64)key * q + v.part] = P[t];
}

// sum_b b * B_b = sum_t 2^t * (sum of the buckets whose index has bit t set), for every (group, window) = bw: G[((bw * c + t) << (c - 1)) + j] = the j-th such bucket of bw
__global__ void msm_bitsel_kernel(u64 count, u32 q, u32 c, const uint4* __restrict__ buckets, uint4* __restrict__ G) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * q) return;
  const VecPart v = vec_split(t, q);
  const u32 j = (u32)(v.elem & ((1u << (c - 1)) - 1)); const u64 grp = v.elem >> (c - 1);
  const u64 bw = grp / c; const u32 bit = (u32)(grp - bw * c);
  const u32 b = ((j >> bit) << (bit + 1)) | (1u << bit) | (j & ((1u << bit) - 1));
  G[t] = buckets[((bw << c) + b) * q + v.part];
}

}  // namespace

extern "C" {
int nbls_msm_keys_launch(unsigned m, unsigned dims, unsigned nwin, unsigned c, unsigned i0, unsigned g0, unsigned ngroups, unsigned n_pts, const uint32_t* off,
                         const void* scalars, uint32_t* keys, uint32_t* vals, hipStream_t stream) {
  return launch_1d(msm_keys_kernel, m, 256, 0, stream, m, dims, nwin, c, i0, g0, ngroups, n_pts, n_pts, 0u, 0u, off, scalars, keys, vals);
}
// the wider map of the rows form (msm_keys_kernel): n_pts, glen > 0
int nbls_msm_keys_map_launch(unsigned m, unsigned dims, unsigned nwin, unsigned c, unsigned i0, unsigned g0, unsigned ngroups, unsigned n_pts, unsigned glen, unsigned pt_block,
                             unsigned k_mod, const void* scalars, uint32_t* keys, uint32_t* vals, hipStream_t stream) {
  if (!n_pts || !glen) return (int)hipErrorInvalidValue;
  return launch_1d(msm_keys_kernel, m, 256, 0, stream, m, dims, nwin, c, i0, g0, ngroups, n_pts, glen, pt_block, k_mod, (const uint32_t*)nullptr, scalars, keys, vals);
}
int nbls_msm_decompose_launch(unsigned n, unsigned dims, const void* scalars, void* out, hipStream_t stream) {
  return launch_1d(msm_decompose_kernel, n, 256, 0, stream, n, dims, scalars, out);
}
int nbls_msm_sac_launch(unsigned n, const void* scalars, void* out, hipStream_t stream) { return launch_1d(msm_sac_kernel, n, 256, 0, stream, n, scalars, out); }
// temp == NULL: returns the scratch size in *temp_bytes
int nbls_msm_sort_launch(void* temp, size_t* temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t m, int key_bits,
                         hipStream_t stream) {
  return (int)hipcub::DeviceRadixSort::SortPairs(temp, *temp_bytes, keys_in, keys_out, vals_in, vals_out, (int)m, 0, key_bits, stream);
}
int nbls_msm_gather_launch(size_t m, unsigned elem_bytes, const uint32_t* idx, const void* src, void* dst, hipStream_t stream) {
  const u32 q = elem_bytes / 16;
  return launch_1d(msm_gather_kernel, (u64)m * q, 256, 0, stream, m, q, idx, src, dst);
}
// temp == NULL: returns the scan's scratch size in *temp_bytes
int nbls_msm_rank_launch(void* temp, size_t* temp_bytes, size_t m, const uint32_t* keys, uint32_t* pos, uint32_t* maxrun, hipStream_t stream) {
  if (!temp) return (int)hipcub::DeviceScan::InclusiveScan(nullptr, *temp_bytes, pos, pos, hipcub::Max(), (int)m, stream);
  if (!m) return 0;
  int e = (int)hipMemsetAsync(maxrun, 0, 4, stream);
  if (!e) e = launch_1d(msm_heads_flag_kernel, m, 256, 0, stream, m, keys, pos);
  if (!e) e = (int)hipcub::DeviceScan::InclusiveScan(temp, *temp_bytes, pos, pos, hipcub::Max(), (int)m, stream);
  if (!e) e = launch_1d(msm_rank_kernel, m, 256, 0, stream, m, keys, pos, maxrun);
  return e;
}
// 4096 elements per workgroup of 1024 threads
int nbls_msm_pairs_launch(size_t m, unsigned d, const uint32_t* keys, const uint32_t* pos, uint32_t* list, uint32_t* count, hipStream_t stream) {
  if (!m) return 0;
  const hipError_t e = hipMemsetAsync(count, 0, 4, stream);
  return e != hipSuccess ? (int)e : launch_1d(msm_pairs_kernel, ((u64)m + 3) / 4, 1024, 0, stream, m, d, keys, pos, list, count);
}
int nbls_msm_fill_launch(size_t count, unsigned elem_bytes, const void* ident, void* dst, hipStream_t stream) {
  const u32 q = elem_bytes / 16;
  return launch_1d(msm_fill_kernel, (u64)count * q, 256, 0, stream, count, q, ident, dst);
}
int nbls_msm_heads_launch(size_t m, unsigned elem_bytes, const uint32_t* keys, const void* P, void* buckets, hipStream_t stream) {
  const u32 q = elem_bytes / 16;
  return launch_1d(msm_heads_kernel, (u64)m * q, 256, 0, stream, m, q, keys, P, buckets);
}
// nbw = groups * nwin
int nbls_msm_bitsel_launch(size_t nbw, unsigned c, unsigned elem_bytes, const void* buckets, void* G, hipStream_t stream) {
  const u32 q = elem_bytes / 16;
  const u64 count = ((u64)nbw * c) << (c - 1);
  return launch_1d(msm_bitsel_kernel, count * q, 256, 0, stream, count, q, c, buckets, G);
}
}
