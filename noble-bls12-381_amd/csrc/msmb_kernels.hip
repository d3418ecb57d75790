// msmb_kernels.hip -- data movement of the batched multi-scalar multiplication (pipelines_msm_batch.cpp): many independent sums share every launch of the bucket method.
// What msm_kernels.hip fixes at compile time is a run-time argument here -- the window width c -- and every key carries the sum it belongs to:
//   key = (group * nwin + window) << c | digit
// so a run of equal keys never crosses a group, and the key is at the same time the index of its bucket.  The sort, the ranks, the pair lists, the gather and the heads are the
// kernels of msm_kernels.hip unchanged.  Points are raw projective elements of 192 (G1) or 384 (G2) bytes, moved as 16-byte vectors, one vector per thread, consecutive
// threads on consecutive vectors of the same point.  No kernel here uses an atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
typedef uint32_t u32;
typedef uint64_t u64;

// One thread per item e of a slab: scalar i = i0 + e / dims of the call, part d = e % dims of its split (dims = 1: unsplit; the split scalars lie dims * 32 bytes per scalar).
// The item's group is found in the call's offsets (off[0 .. ngroups], relative to the first scalar; empty groups own nothing), or is i / n_pts in the rows form (n_pts > 0),
// where the point is i % n_pts.  keys[w * m + e] = ((group - g0) * nwin + w) << c | digit_w, vals[w * m + e] = point * dims + d (the index of the converted point).
__global__ void msmb_keys_kernel(u32 m, u32 dims, u32 nwin, u32 c, u32 i0, u32 g0, u32 ngroups, u32 n_pts, const u32* __restrict__ off, const uint8_t* __restrict__ scalars,
                                 u32* __restrict__ keys, u32* __restrict__ vals) {
  const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const u32 i = i0 + e / dims, d = e % dims;
  u32 g, pt;
  if (n_pts) { g = i / n_pts; pt = i - g * n_pts; }
  else {
    u32 lo = g0, hi = ngroups;      // the last g with off[g] <= i: off[g0] <= i holds for every item of the slab, and off[g + 1] > i follows
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
    g = lo; pt = i;
  }
  const u32* k = (const u32*)(scalars + 32ull * ((u64)i * dims + d));
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

// sum_b b * B_b = sum_t 2^t * (sum of the buckets whose index has bit t set), for every (group, window) = bw: G[((bw * c + t) << (c - 1)) + j] = the j-th such bucket of bw
__global__ void msmb_bitsel_kernel(u64 count, u32 q, u32 c, const uint4* __restrict__ buckets, uint4* __restrict__ G) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * q) return;
  const u64 e = t / q; const u32 part = (u32)(t - e * q);
  const u32 j = (u32)(e & ((1u << (c - 1)) - 1)); const u64 grp = e >> (c - 1);
  const u64 bw = grp / c; const u32 bit = (u32)(grp - bw * c);
  const u32 b = ((j >> bit) << (bit + 1)) | (1u << bit) | (j & ((1u << bit) - 1));
  G[t] = buckets[((bw << c) + b) * q + part];
}

inline unsigned blocks_for(u64 threads) { return (unsigned)((threads + 255) / 256); }
}  // namespace

extern "C" {
int nbls_msmb_keys_launch(unsigned m, unsigned dims, unsigned nwin, unsigned c, unsigned i0, unsigned g0, unsigned ngroups, unsigned n_pts, const void* off, const void* scalars,
                          void* keys, void* vals, void* stream) {
  hipLaunchKernelGGL(msmb_keys_kernel, dim3(blocks_for(m)), dim3(256), 0, (hipStream_t)stream, m, dims, nwin, c, i0, g0, ngroups, n_pts, (const u32*)off, (const uint8_t*)scalars,
                     (u32*)keys, (u32*)vals);
  return (int)hipGetLastError();
}
// nbw = (groups of the slab) * nwin
int nbls_msmb_bitsel_launch(size_t nbw, unsigned c, unsigned elem_bytes, const void* buckets, void* G, void* stream) {
  const u32 q = elem_bytes / 16;
  const u64 count = ((u64)nbw * c) << (c - 1);
  hipLaunchKernelGGL(msmb_bitsel_kernel, dim3(blocks_for(count * q)), dim3(256), 0, (hipStream_t)stream, count, q, c, (const uint4*)buckets, (uint4*)G);
  return (int)hipGetLastError();
}
}
