// groth16_prove_kernels.hip -- the scalar-field side of the Groth16 prover (pipelines_groth16_prove.cpp): the witness check, the three R1CS matrix-vector products, the
// pointwise step of the quotient, the scalars of the four sums and the small kernels around the key and the proof's bytes.  The lane code is g16p_exec.h's, shared with the
// simulator (nbls_sim_g16p_*); the transforms are kzg_kernels.hip's, the curve arithmetic runs as step programs (decoder, MSM, compression).  Every store is a plain C++ vector
// or byte store; the flags are bytes that every writer sets to the same 1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "g16p_exec.h"   // fr_exec.h
#include "nbls.h"
#include "kernel_parts.h"
#include "launchers.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

constexpr int PB = 256;   // lanes of a workgroup: four wavefronts

// one element of z | r | s per lane (g16p_exec.h g16p_witness_element).  16-byte loads and stores, no LDS
__global__ void __launch_bounds__(PB) g16p_witness_kernel(u64 n_vars, const uint8_t* __restrict__ w32, Fr* __restrict__ z, uint8_t* __restrict__ flags) {
  const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
  if (i < n_vars + 2) g16p_witness_element(n_vars, i, w32, z, flags);
}

// lane (l ^ mask)'s value, inside the wavefront
__device__ inline Fr fr_lane_xor(const Fr& v, u32 mask) {
  Fr o;
#pragma unroll
  for (int l = 0; l < FR_NL; l++) o.l[l] = (u32)__shfl_xor((int)v.l[l], (int)mask);
  return o;
}
// a = A z, b = B z, c = C z and the flag a_j b_j == c_j.  order: the N rows, longest first (by the longest of a row's three lists); the first n_wave of them get a wavefront
// each -- the lanes stride the entries, then six levels of cross-lane additions --, the others a lane each.  The three matrices of a row are summed by the same wavefront,
// so the flag needs no second pass.  The unit of the grid is the wavefront: n_wave + ceil((N - n_wave) / 64) of them, four to a workgroup, no barrier and no LDS -- at its 102 VGPRs
// four workgroups fit a compute unit, four wavefronts a SIMD, to hide the 32-byte gathers of z behind each other's products.  Rows of similar length share a wavefront, which is what the order is for.
// Stores: 16-byte vectors to position rev(j) of the three vectors
__global__ void __launch_bounds__(PB) g16p_spmv_kernel(u32 log2_n, u32 n_wave, const u32* __restrict__ order, G16pMatrix A, G16pMatrix B, G16pMatrix C, const Fr* __restrict__ z,
                                                       uint8_t* __restrict__ v32, uint8_t* __restrict__ flags) {
  const u32 N = 1u << log2_n, lane = threadIdx.x & (G16P_WAVE - 1);
  const u64 wave = (u64)blockIdx.x * (PB / G16P_WAVE) + threadIdx.x / G16P_WAVE;
  if (wave < n_wave) {   // (uniform over the wavefront)
    const u32 row = order[wave];
    Fr a = g16p_row_part(A, z, row, lane, G16P_WAVE), b = g16p_row_part(B, z, row, lane, G16P_WAVE), c = g16p_row_part(C, z, row, lane, G16P_WAVE);
    for (u32 m = 1; m < G16P_WAVE; m <<= 1) { a = fr_add(a, fr_lane_xor(a, m)); b = fr_add(b, fr_lane_xor(b, m)); c = fr_add(c, fr_lane_xor(c, m)); }
    if (lane == 0) g16p_row_store(log2_n, row, a, b, c, v32, flags);
    return;
  }
  const u64 k = (wave - n_wave) * G16P_WAVE + lane + n_wave;
  if (k >= N) return;
  const u32 row = order[k];
  g16p_row_store(log2_n, row, g16p_row_part(A, z, row, 0, 1), g16p_row_part(B, z, row, 0, 1), g16p_row_part(C, z, row, 0, 1), v32, flags);
}

// the pointwise step of the quotient, one element per lane, in place on a's rows (a32 is read and written by the same lane: no __restrict__ on it)
__global__ void __launch_bounds__(PB) g16p_quotient_kernel(u32 log2_n, u64 n, uint8_t* a32, const uint8_t* __restrict__ b32, const uint8_t* __restrict__ c32,
                                                           const int8_t* __restrict__ st3, Fr kinv) {
  const u64 idx = (u64)blockIdx.x * PB + threadIdx.x;
  if (idx < (n << log2_n)) g16p_quot_element(log2_n, n, idx, a32, b32, c32, st3, kinv);
}
// nbls_groth16_quotient's check of the caller's values, one element per lane
__global__ void __launch_bounds__(PB) g16p_check_kernel(u32 log2_n, u64 n, const uint8_t* __restrict__ a32, const uint8_t* __restrict__ b32, const uint8_t* __restrict__ c32,
                                                        uint8_t* __restrict__ violated) {
  const u64 idx = (u64)blockIdx.x * PB + threadIdx.x;
  if (idx < (n << log2_n)) g16p_check_element(log2_n, idx, a32, b32, c32, violated);
}
__global__ void g16p_quot_status_kernel(u64 n, const int8_t* __restrict__ st3, const uint8_t* __restrict__ violated, int8_t* __restrict__ status) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) status[i] = (int8_t)g16p_quot_status(n, i, st3, violated);
}

// one scalar per lane (g16p_exec.h g16p_scalar_element)
__global__ void __launch_bounds__(PB) g16p_scalars_kernel(G16pScalars S) {
  const u64 i = (u64)blockIdx.x * PB + threadIdx.x;
  if (i < g16p_scalar_count(S.n_vars, S.n_public, S.N)) g16p_scalar_element(S, i);
}

// the key's query points behind the decoder, one 16-byte vector per thread (q vectors a point): a zero point (status 1) becomes `fixed`, a point of the subgroup, and its
// mask byte 1 -- its scalar is forced to zero by g16p_scalars_kernel
__global__ void g16p_mask_kernel(u64 n, u32 q, const int8_t* __restrict__ st, const uint4* __restrict__ fixed, uint4* __restrict__ pts, uint8_t* __restrict__ mask) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * q) return;
  const VecPart v = vec_split(t, q);
  const bool zero = st[v.elem] == 1;
  if (zero) pts[t] = fixed[v.part];
  if (v.part == 0) mask[v.elem] = zero ? 1 : 0;
}

// the proof's bytes and status, twelve 16-byte vectors, one per thread.  out192 holds compress(A) | compress(B) | compress(C); zero3: the zero flags of A, B, C.  status: the
// first of NBLS_ST_NON_CANONICAL, NBLS_ST_G16_UNSATISFIED, 1 (A or B is the zero point), 0; a proof whose status is not 0 is 192 zero bytes; a zero C is 0xc0 00..
__global__ void g16p_finish_kernel(const uint8_t* __restrict__ flags, const int8_t* __restrict__ zero3, uint4* __restrict__ out192, int8_t* __restrict__ status) {
  const u32 t = threadIdx.x;
  if (t >= 12) return;
  const int st = flags[G16P_F_NONCANON] ? NBLS_ST_NON_CANONICAL : flags[G16P_F_UNSAT] ? NBLS_ST_G16_UNSATISFIED : (zero3[0] == 1 || zero3[1] == 1) ? 1 : 0;
  if (st) out192[t] = make_uint4(0, 0, 0, 0);
  else if (t >= 9 && zero3[2] == 1) out192[t] = make_uint4(t == 9 ? 0xc0u : 0u, 0, 0, 0);
  if (t == 0) *status = (int8_t)st;
}
}  // namespace

extern "C" {
// w32: n_vars + 2 elements (z | r | s), 16-byte aligned; z: n_vars elements of limbs, 32-byte aligned; flags: G16P_FLAGS bytes, cleared by the caller
int nbls_g16p_witness_launch(size_t n_vars, const void* w32, void* z, void* flags, hipStream_t stream) {
  if (((uintptr_t)w32 & 15) || ((uintptr_t)z & 31)) return (int)hipErrorInvalidValue;
  return launch_1d(g16p_witness_kernel, (u64)n_vars + 2, PB, 0, stream, (u64)n_vars, w32, z, flags);
}
// the three products of 2^log2_n rows (mats: rows, cols, vals of A, of B, of C; order: 2^log2_n row indices, the first n_wave of them summed by a wavefront each; z and the
// vals 32-byte aligned, v32 16-byte aligned: 3 << log2_n elements)
int nbls_g16p_spmv_launch(unsigned log2_n, unsigned n_wave, const uint32_t* order, const void* const mats[9], const void* z, void* v32, void* flags, hipStream_t stream) {
  if (log2_n < 1 || log2_n > 24 || n_wave > (1u << log2_n) || ((uintptr_t)v32 & 15) || (((uintptr_t)z | (uintptr_t)mats[2] | (uintptr_t)mats[5] | (uintptr_t)mats[8]) & 31))
    return (int)hipErrorInvalidValue;
  const G16pMatrix A{(const u32*)mats[0], (const u32*)mats[1], (const Fr*)mats[2]}, B{(const u32*)mats[3], (const u32*)mats[4], (const Fr*)mats[5]},
      C{(const u32*)mats[6], (const u32*)mats[7], (const Fr*)mats[8]};
  const u64 waves = (u64)n_wave + (((u64)1 << log2_n) - n_wave + G16P_WAVE - 1) / G16P_WAVE;
  return launch_1d(g16p_spmv_kernel, waves * G16P_WAVE, PB, 0, stream, log2_n, n_wave, order, A, B, C, z, v32, flags);
}
// n rows of 2^log2_n elements each (16-byte aligned arrays); st3: 3 n statuses; kinv: g16p_quot_factor as eight words
int nbls_g16p_quotient_launch(unsigned log2_n, size_t n, void* a32, const void* b32, const void* c32, const void* st3, const uint32_t* kinv, hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 24 || (((uintptr_t)a32 | (uintptr_t)b32 | (uintptr_t)c32) & 15)) return (int)hipErrorInvalidValue;
  Fr k;
  for (int i = 0; i < FR_NL; i++) k.l[i] = kinv[i];
  return launch_1d(g16p_quotient_kernel, (u64)n << log2_n, PB, 0, stream, log2_n, (u64)n, a32, b32, c32, st3, k);
}
// violated: n bytes, cleared by the caller
int nbls_g16p_check_launch(unsigned log2_n, size_t n, const void* a32, const void* b32, const void* c32, void* violated, hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 24 || (((uintptr_t)a32 | (uintptr_t)b32 | (uintptr_t)c32) & 15)) return (int)hipErrorInvalidValue;
  return launch_1d(g16p_check_kernel, (u64)n << log2_n, PB, 0, stream, log2_n, (u64)n, a32, b32, c32, violated);
}
int nbls_g16p_quot_status_launch(size_t n, const void* st3, const void* violated, void* status, hipStream_t stream) {
  return launch_1d(g16p_quot_status_kernel, n, PB, 0, stream, (u64)n, st3, violated, status);
}
int nbls_g16p_scalars_launch(const nbls::G16pScalars* S, hipStream_t stream) {
  if ((((uintptr_t)S->w32 | (uintptr_t)S->h32 | (uintptr_t)S->sa | (uintptr_t)S->sb | (uintptr_t)S->sc) & 15) || S->n_vars <= S->n_public) return (int)hipErrorInvalidValue;
  return launch_1d(g16p_scalars_kernel, g16p_scalar_count(S->n_vars, S->n_public, S->N), PB, 0, stream, *S);
}
// n points of elem_bytes (96 or 192) each
int nbls_g16p_mask_launch(size_t n, unsigned elem_bytes, const void* st, const void* fixed, void* pts, void* mask, hipStream_t stream) {
  if (!n) return 0;
  if ((elem_bytes != 96 && elem_bytes != 192) || (((uintptr_t)fixed | (uintptr_t)pts) & 15)) return (int)hipErrorInvalidValue;
  return launch_1d(g16p_mask_kernel, (u64)n * (elem_bytes / 16), PB, 0, stream, (u64)n, elem_bytes / 16, st, fixed, pts, mask);
}
int nbls_g16p_finish_launch(const void* flags, const void* zero3, void* out192, void* status, hipStream_t stream) {
  if ((uintptr_t)out192 & 15) return (int)hipErrorInvalidValue;
  return launch_1d(g16p_finish_kernel, 64, 64, 0, stream, flags, zero3, out192, status);
}
}
