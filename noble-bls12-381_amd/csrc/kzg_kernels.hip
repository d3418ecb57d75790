// kzg_kernels.hip -- the scalar-field side of KZG verification (pipelines_kzg.cpp) and proving (pipelines_kzg_prove.cpp: the quotient of an opening, the canonical check of
// blobs that are only committed to, the closing kernel of the compressed results): polynomials in evaluation form evaluated at a point (nbls_fr_eval_roots, and y_i = p_i(z_i) of
// nbls_kzg_verify_blobs), the table of roots of unity, and the small Fr kernels around the two MSMs of the combined check and the ladders of the per-item pass.  The arithmetic is
// fr_exec.h's and the workgroups' choreography fr_workgroup.h's, both written once and shared with the simulator (vm_sim.cpp); the curve arithmetic runs as step programs
// (decoder, MSM, ladders, Miller loops).
// Further down: the transform and the cells of EIP-7594, their recovery from half of the cells (pipelines_kzg_cells.cpp) and the interpolation of cells for their verifier
// (pipelines_kzg_verify_cells.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include "fr_workgroup.h"   // fr_exec.h, nbls.h; the workgroup bodies of the kernels below
#include "kernel_parts.h"
#include "launchers.h"

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
using namespace nbls;

constexpr int EV = FR_EVAL_LANES;   // 256 lanes = four wavefronts per polynomial

// table[j] = omega^rev(j) in Montgomery form, one entry per lane: built once per context and log2_n (two short exponentiations per entry; 4096 entries at most)
__global__ void kzg_roots_kernel(u32 log2_n, Fr* __restrict__ table) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < (1u << log2_n)) table[j] = fr_root_entry(fr_omega(log2_n), log2_n, j);
}

// One workgroup per polynomial, lane t on the terms t, t + 256, .. (ceil(N / 256) of them: the loop bounds are the workgroup's), ONE fixed-chain inversion per lane.  N < 256
// leaves lanes idle under fr_eval_lane's mask.  Dynamic LDS: the running products of the batch inversion, 8 KB per term of a lane (128 KB at N = 4096), [term][limb][lane] so that
// a wavefront's 64 words fall on 64 banks.  The 256 partial sums meet in an LDS tree (8 KB) of modular additions; at most one lane of the workgroup meets a vanishing denominator
// (the roots are distinct) and leaves its index in LDS.  The bodies: fr_workgroup.h kzg_eval_body, kzg_quotient_body
__global__ void __launch_bounds__(EV) kzg_eval_kernel(u32 log2_n, const uint8_t* __restrict__ evals, const uint8_t* __restrict__ z32, const Fr* __restrict__ roots,
                                                      uint8_t* __restrict__ out32, int8_t* __restrict__ status) {
  extern __shared__ u32 pre[];
  __shared__ Fr part[EV];
  __shared__ u32 sh_hit, sh_bad;
  const u64 p = blockIdx.x;
  kzg_eval_body(FrWorkgroup<EV>(), log2_n, evals + ((p * 32) << log2_n), z32 + 32 * p, roots, out32 + 32 * p, status + p, pre, part, &sh_hit, &sh_bad);
}
// The quotient of an opening (nbls_fr_quotient_roots, the proofs of pipelines_kzg_prove.cpp): no more LDS than the evaluation takes; q_j = (y - f_j) / (z - w_j) as 32 bytes
// big-endian -- the batched MSM's scalar array
__global__ void __launch_bounds__(EV) kzg_quotient_kernel(u32 log2_n, const uint8_t* __restrict__ evals, const uint8_t* __restrict__ z32, const Fr* __restrict__ roots,
                                                          uint8_t* __restrict__ out_y32, uint8_t* __restrict__ out_q32, int8_t* __restrict__ status) {
  extern __shared__ u32 pre[];
  __shared__ Fr part[EV];
  __shared__ Fr sh_y;
  __shared__ u32 sh_hit, sh_bad;
  const u64 p = blockIdx.x;
  kzg_quotient_body(FrWorkgroup<EV>(), log2_n, evals + ((p * 32) << log2_n), z32 + 32 * p, roots, out_y32 + 32 * p, out_q32 + ((p * 32) << log2_n), status + p, pre, part, &sh_y,
                    &sh_hit, &sh_bad);
}

// ---- The transform (nbls_fr_ntt), the cells of EIP-7594 (nbls_kzg_compute_cells) and the quotient rows of their proofs (pipelines_kzg_cells.cpp); fr_exec.h has the network.
constexpr int NT = FR_NTT_LANES;
// the table of the inverse roots, (1 / omega)^rev(j): what the stages towards the coefficients divide by.  A permutation of the table of roots, made once per context and log2_n
__global__ void kzg_inv_roots_kernel(u32 log2_n, const Fr* __restrict__ roots, Fr* __restrict__ table) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < (1u << log2_n)) table[j] = roots[fr_inv_root_index(log2_n, j)];
}
// One workgroup per polynomial, the whole polynomial in dynamic LDS (32 N bytes: 128 KB at N = 4096), one barrier per stage; fr_workgroup.h kzg_ntt_body has the modes and the
// refusals.  shift32 = g for every blob of the cells mode: shift_stride = 0.  in32 / out32 / coef32 are 16-byte aligned; out_stride = the bytes of an output row
__global__ void __launch_bounds__(NT) kzg_ntt_kernel(u32 log2_n, u32 mode, const uint8_t* __restrict__ in32, const uint8_t* __restrict__ shift32, u32 shift_stride,
                                                     const Fr* __restrict__ roots, const Fr* __restrict__ iroots, uint8_t* __restrict__ out32, u64 out_stride,
                                                     uint8_t* __restrict__ coef32, int8_t* __restrict__ status) {
  extern __shared__ u32 a[];
  __shared__ Fr sh_s;
  __shared__ u32 sh_bad, sh_zero;
  const u64 p = blockIdx.x;
  kzg_ntt_body(FrWorkgroup<NT>(), log2_n, mode, in32 + ((p * 32) << log2_n), shift32 ? shift32 + (u64)shift_stride * p : nullptr, roots, iroots, out32 + p * out_stride, out_stride,
               coef32 ? coef32 + ((p * 32) << log2_n) : nullptr, status ? status + p : nullptr, a, &sh_s, &sh_bad, &sh_zero);
}
// Transforms of up to 2^24 elements (nbls_fr_ntt_large / nbls_fr_ntt_dev; fr_exec.h has the split, fr_workgroup.h kzg_ntt_pass_body and kzg_ntt_tail_body the bodies).
// One run of global stages: workgroup = (polynomial, hi, tile of 2^c consecutive lo), its 2^(q + c) elements in dynamic LDS (at most 128 KB), one barrier per stage.  in32
// and out32 are equal or disjoint (every workgroup reads and writes the same elements): no __restrict__.  shift32: n shifts, or NULL; sinv: n elements, or NULL
__global__ void __launch_bounds__(NT) kzg_ntt_pass_kernel(FrNttRun R, u32 inverse, const uint8_t* in32, uint8_t* out32, const uint8_t* __restrict__ shift32,
                                                          const Fr* __restrict__ sinv, const Fr* __restrict__ table, u32* flags, int8_t* __restrict__ status) {
  extern __shared__ u32 a[];
  const u32 lt = R.log2_n - R.j0 - R.q - R.c, w = blockIdx.x, within = w & ((1u << (lt + R.j0)) - 1);   // lt: the log of the tiles of one hi
  const u64 p = w >> (lt + R.j0), row = (p * 32) << R.log2_n;
  kzg_ntt_pass_body(FrWorkgroup<NT>(), R, inverse != 0, within >> lt, (within & ((1u << lt) - 1)) << R.c, within == 0, in32 + row, out32 + row, shift32 ? shift32 + 32 * p : nullptr,
                    sinv ? sinv + p : nullptr, table, flags + p, status ? status + p : nullptr, a);
}
// The tails: workgroup = block B of 2^log2_t elements of a polynomial of 2^log2_k blocks, kzg_ntt_kernel's stages with the block's own shift
__global__ void __launch_bounds__(NT) kzg_ntt_tail_kernel(u32 log2_t, u32 log2_k, u32 inverse, Fr w, const uint8_t* in32, uint8_t* out32, const uint8_t* __restrict__ shift32,
                                                          Fr* sinv, const Fr* __restrict__ roots, const Fr* __restrict__ iroots, u32* flags, int8_t* __restrict__ status) {
  extern __shared__ u32 a[];
  __shared__ Fr sh_s;
  const u64 blk = blockIdx.x, p = blk >> log2_k, off = (blk * 32) << log2_t;
  kzg_ntt_tail_body(FrWorkgroup<NT>(), log2_t, log2_k, inverse != 0, (u32)blk & ((1u << log2_k) - 1), w, in32 + off, out32 + off, shift32 ? shift32 + 32 * p : nullptr, sinv + p, roots,
                    iroots, flags + p, status ? status + p : nullptr, a, &sh_s);
}
// The quotient rows of n blobs' cell proofs, one lane per chain (fr_exec.h fr_cell_chain): lane (blob, k, j), j fastest, so that a wavefront reads and writes consecutive
// elements.  coef32: n x N coefficients (all-zero for a refused blob: its rows come out zero); sroots: the table of the 2 N / c roots (s_k = entry k); out_q32: n x (2 N / c)
// rows of N scalars; row_st[row] = the status of the row's blob, for the closing kernel
__global__ void __launch_bounds__(256) kzg_cell_rows_kernel(u32 log2_n, u32 log2_cell, u32 n, const uint8_t* __restrict__ coef32, const Fr* __restrict__ sroots,
                                                            const int8_t* __restrict__ blob_st, uint8_t* __restrict__ out_q32, int8_t* __restrict__ row_st) {
  const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= ((u64)n << (log2_n + 1))) return;
  const u32 blob = (u32)(gid >> (log2_n + 1)), within = (u32)gid & ((2u << log2_n) - 1), k = within >> log2_cell, j = within & ((1u << log2_cell) - 1);
  const u64 row = ((u64)blob << (log2_n + 1 - log2_cell)) + k;
  fr_cell_chain(coef32 + (((u64)blob * 32) << log2_n), log2_n, log2_cell, j, sroots[k], out_q32 + ((row * 32) << log2_n));
  if (j == 0) row_st[row] = blob_st[blob];
}

// ---- All cell proofs of a blob together (FK20: nbls_kzg_fk20_create and the two *_fk20 calls, pipelines_kzg_cells.cpp); fr_exec.h has the identities and the arithmetic.
// The per-blob scalars of pass A: the size-M transform of every zero-padded stripe of the coefficients, FR_FK_LANES lanes a workgroup, its stripes side by side in dynamic LDS
// (16 KB up to M = 512, 32 M bytes above), one barrier per stage.  coef32: n x N coefficients (all-zero for a refused blob: zero scalars); out32: n x M x c scalars, [blob][i][j]
__global__ void __launch_bounds__(FR_FK_LANES) kzg_fk20_scalars_kernel(u32 log2_n, u32 log2_cell, u32 n, const uint8_t* __restrict__ coef32, const Fr* __restrict__ sroots,
                                                                       uint8_t* __restrict__ out32) {
  extern __shared__ u32 a[];
  kzg_fk20_scalars_body(FrWorkgroup<FR_FK_LANES>(), log2_n, log2_cell, n, blockIdx.x, coef32, sroots, out32, a);
}
// row_st[blob * M + k] = blob_st[blob]: what the closing kernel reads per proof
__global__ void kzg_fk20_row_status_kernel(u32 log2_m, u32 n, const int8_t* __restrict__ blob_st, int8_t* __restrict__ row_st) {
  const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid < ((u64)n << log2_m)) row_st[gid] = blob_st[gid >> log2_m];
}
// the scalars of the handle's one MSM, one lane each: c M groups of n' - 1 powers of w_i
__global__ void kzg_fk20_powers_kernel(u32 log2_cell, u32 log2_m, u32 count, const Fr* __restrict__ sroots, uint8_t* __restrict__ out32) {
  const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < count) fr_store_q(fr_fk_power(sroots, log2_cell, log2_m, idx), out32 + 32ull * idx);
}
// the projection matrix B, one lane per entry: out32[(k M + i) * 32]
__global__ void kzg_fk20_matrix_kernel(u32 log2_m, const Fr* __restrict__ sroots, const Fr* __restrict__ isroots, uint8_t* __restrict__ out32) {
  const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >> (2 * log2_m)) return;
  fr_store_q(fr_fk_matrix_entry(sroots, isroots, log2_m, idx >> log2_m, idx & ((1u << log2_m) - 1)), out32 + 32ull * idx);
}

// ---- The recovery of blobs from at least half of their cells (nbls_kzg_recover_cells, pipelines_kzg_cells.cpp); fr_exec.h has the route and the arithmetic.
// The Z values of n blobs, one lane per (blob, value): value v < M = 2^log2_m is Zs(s_v), value M + j the inverse 1 / Zs(7^c s_j) of block j -- M / 2 inversions a blob, none
// per element.  slot: n x M (the host's slot maps); pre[blob] != 0: the index set was refused, nothing is written; zv: n x 3 M / 2 values, Montgomery form
__global__ void __launch_bounds__(256) kzg_recover_z_kernel(u32 log2_m, u32 n, const u32* __restrict__ slot, const int8_t* __restrict__ pre, const Fr* __restrict__ sroots,
                                                            const FrRecoverConsts* __restrict__ kc, Fr* __restrict__ zv) {
  const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 per = 3u << (log2_m - 1);
  if (gid >= (u64)n * per) return;
  const u32 blob = (u32)(gid / per), v = (u32)(gid % per);
  if (pre[blob]) return;
  zv[gid] = fr_recover_z(sroots, slot + ((u64)blob << log2_m), log2_m, v, kc->c7);
}
// One workgroup per blob, one polynomial in dynamic LDS at a time (32 N bytes), kzg_ntt_kernel's lanes, stages and barriers; fr_workgroup.h kzg_recover_body has the six
// transforms and the statuses.  cells / out32 / coef32 are 16-byte aligned; coef32 is read back by the lanes that wrote it (no __restrict__)
__global__ void __launch_bounds__(NT) kzg_recover_kernel(u32 log2_n, u32 log2_cell, const uint8_t* __restrict__ cells, const u32* __restrict__ slot_all,
                                                         const int8_t* __restrict__ pre, const Fr* __restrict__ zv_all, const FrRecoverConsts* __restrict__ kc,
                                                         const Fr* __restrict__ roots, const Fr* __restrict__ iroots, uint8_t* __restrict__ out32, uint8_t* coef32,
                                                         int8_t* __restrict__ status) {
  extern __shared__ u32 a[];
  __shared__ u32 sh_bad, sh_diff;
  const u32 log2_m = log2_n + 1 - log2_cell;
  const u64 p = blockIdx.x;
  kzg_recover_body(FrWorkgroup<NT>(), log2_n, log2_cell, cells, slot_all + (p << log2_m), pre[p], zv_all + p * (3u << (log2_m - 1)), *kc, roots, iroots,
                   out32 + ((p * 64) << log2_n), coef32 + ((p * 32) << log2_n), status + p, a, &sh_bad, &sh_diff);
}

// blobs that are only committed to (no quotient kernel reads them): status[i] = NBLS_ST_NON_CANONICAL where an element of blob i is >= r, and that blob's row is zeroed in
// place, so that the MSM reads canonical scalars only.  One workgroup per blob
__global__ void __launch_bounds__(256) kzg_canon_kernel(u32 log2_n, uint8_t* __restrict__ evals, int8_t* __restrict__ status) {
  __shared__ u32 sh_bad;
  kzg_canon_body(FrWorkgroup<256>(), log2_n, evals + (((u64)blockIdx.x * 32) << log2_n), status + blockIdx.x, &sh_bad);
}
// the n compressed sums of a prover call, in place: status[i] = the first non-zero of st_a[i], st_b[i] (either array may be NULL); all-zero bytes where it is set, 0xc0 00..
// where the sum is the zero point (zero[i] == 1)
__global__ void kzg_prove_tail_kernel(u32 n, const int8_t* __restrict__ zero, const int8_t* __restrict__ st_a, const int8_t* __restrict__ st_b, uint8_t* __restrict__ out48,
                                      int8_t* __restrict__ status) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int8_t a = st_a ? st_a[i] : 0, b = st_b ? st_b[i] : 0, v = a ? a : b;
  status[i] = v;
  close_compressed(out48 + 48ull * i, 48, v ? v : zero[i] == 1);   // (st_a, st_b hold 0 or NBLS_ST_NON_CANONICAL)
}

// the status of an item before its scalars are looked at, from the two decoders: the commitment's if >= 2, else 10 + the proof's if >= 2, else `rest`
__device__ inline int kzg_pre_status(int sc, int sp, int rest) { return sc >= 2 ? sc : sp >= 2 ? 10 + sp : rest; }
__device__ inline void copy96(uint8_t* dst, const uint8_t* src) {
  const uint4* s = (const uint4*)src; uint4* d = (uint4*)dst;
#pragma unroll
  for (int q = 0; q < 6; q++) d[q] = s[q];
}

// The scalars of the combined check, one item per lane.  dst: the decoder statuses of the n commitments, then of the n proofs; w32: the weights r_i; z32 / y32: 32 bytes
// big-endian; yst (may be NULL): the status of the device evaluation that produced y_i.  pre[i] = the item's status before any pairing (commitment, proof, canonical scalars: in
// that order).  An item with pre != 0 gets zero scalars everywhere; a zero point (decoder status 1) takes part as the identity: zero scalars for that point alone.  Every point that
// a zero scalar stands for is replaced by the generator, so that the MSM reads points of the curve only; aff[2 n] = the generator, the point of sum_i r_i y_i.
//   s1[i] = r_i (the 64-bit MSM over the proofs);  s2[i] = r_i, s2[n + i] = r_i z_i mod r (the 256-bit MSM);  t[i] = r_i y_i mod r, plain limbs, summed by kzg_sum_kernel
__global__ void kzg_items_kernel(u32 n, const int8_t* __restrict__ dst, const uint8_t* __restrict__ w32, const uint8_t* __restrict__ z32, const uint8_t* __restrict__ y32,
                                 const int8_t* __restrict__ yst, const uint8_t* __restrict__ gen96, uint8_t* __restrict__ aff, uint8_t* __restrict__ s1, uint8_t* __restrict__ s2,
                                 Fr* __restrict__ t, int8_t* __restrict__ pre) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == 0) copy96(aff + 192ull * n, gen96);
  const int sc = dst[i], sp = dst[n + i];
  const Fr zr = fr_load_be(z32 + 32ull * i), yr = fr_load_be(y32 + 32ull * i);
  const bool nc = (fr_ge_r_mask(zr) | fr_ge_r_mask(yr)) != 0 || (yst && yst[i] != 0);
  const int st = kzg_pre_status(sc, sp, nc ? NBLS_ST_NON_CANONICAL : 0);
  pre[i] = (int8_t)st;
  const u32 live = (u32)0 - (u32)(st == 0), use_c = live & ((u32)0 - (u32)(sc == 0)), use_p = live & ((u32)0 - (u32)(sp == 0));
  const Fr zero = fr_zero(), r = fr_load_be(w32 + 32ull * i), rm = fr_mul(r, fr_r2());
  fr_store_be(fr_select(use_p, r, zero), s1 + 32ull * i);
  fr_store_be(fr_select(use_c, r, zero), s2 + 32ull * i);
  fr_store_be(fr_select(use_p, fr_mul(rm, fr_select(live, zr, zero)), zero), s2 + 32ull * (n + i));
  t[i] = fr_select(live, fr_mul(rm, fr_select(live, yr, zero)), zero);
  if (!use_c) copy96(aff + 96ull * i, gen96);
  if (!use_p) copy96(aff + 96ull * (n + i), gen96);
}
// out32 = -(sum_i t[i]) mod r as 32 bytes big-endian: one workgroup, the lanes striding over the items, an LDS tree of modular additions
__global__ void __launch_bounds__(EV) kzg_sum_kernel(u32 n, const Fr* __restrict__ t, uint8_t* __restrict__ out32) {
  __shared__ Fr part[EV];
  kzg_sum_body(FrWorkgroup<EV>(), n, t, out32, part);
}
// the per-item pass: zs[i] = z_i (zero where the item is out or its proof is the zero point), ny[i] = -y_i mod r (zero where the item is out)
__global__ void kzg_item_scalars_kernel(u32 n, const int8_t* __restrict__ pre, const int8_t* __restrict__ dst, const uint8_t* __restrict__ z32, const uint8_t* __restrict__ y32,
                                        uint8_t* __restrict__ zs, uint8_t* __restrict__ ny) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 live = (u32)0 - (u32)(pre[i] == 0), use_p = live & ((u32)0 - (u32)(dst[n + i] == 0));
  const Fr zero = fr_zero();
  fr_store_be(fr_select(use_p, fr_load_be(z32 + 32ull * i), zero), zs + 32ull * i);
  fr_store_be(fr_neg(fr_select(live, fr_load_be(y32 + 32ull * i), zero)), ny + 32ull * i);
}
// status[i] of the per-item pass (pst: the decoder statuses of the n proofs).  x = C_i + [z_i]pi_i - [y_i]G1 (the cells: C - [I_k(tau)]G1 + [s_k]pi_k): with a zero proof the tuple holds exactly when x is the zero point; with a non-zero proof a zero x fails
// (e(pi, [tau]G2) is not one) and otherwise the pairing product decides (one[i]: the final exponentiation is Fp12.ONE)
__global__ void kzg_item_status_kernel(u32 n, const int8_t* __restrict__ pre, const int8_t* __restrict__ pst, const int8_t* __restrict__ xzero, const uint8_t* __restrict__ one,
                                       int8_t* __restrict__ status) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool pz = pst[i] == 1, xz = xzero[i] == 1;
  const bool ok = pz ? xz : (!xz && one[i] != 0);
  status[i] = pre[i] ? pre[i] : ok ? 0 : NBLS_ST_NOT_VERIFIED;
}

// ---- The cells of EIP-7594 on the verifier's side (pipelines_kzg_verify_cells.cpp); fr_exec.h has the arithmetic.
constexpr int CL = FR_CELL_LANES;
// the table of the M = 2^log2_m inverse shifts 1 / h_k of (log2_n, log2_cell), Montgomery form: built once per context and pair, as the tables of roots are
__global__ void kzg_cell_ishifts_kernel(u32 log2_n, u32 log2_m, Fr* __restrict__ table) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < (1u << log2_m)) table[k] = fr_cell_ishift_entry(fr_omega(log2_n + 1), log2_n, log2_m, k);
}
// lane (t ^ mask)'s value: the c <= 64 lanes of a cell lie inside one wavefront, so a stage's exchange is a cross-lane read -- no LDS, and no barrier between the stages
__device__ inline Fr fr_lane_xor(const Fr& v, u32 mask) {
  Fr o;
#pragma unroll
  for (int l = 0; l < FR_NL; l++) o.l[l] = (u32)__shfl_xor((int)v.l[l], (int)mask);
  return o;
}
// The interpolation polynomials of n_cells cells of c = 2^log2_cell <= 64 elements each, c lanes per cell (fr_exec.h fr_cell_*): a wavefront holds 64 / c cells side by side, a
// workgroup four wavefronts.  Lane group q of the launch takes the cells q, q + groups, .. -- the same number of rounds on every lane, a round past the end on the last cell
// with nothing kept -- and in every round: the elements in (32 bytes big-endian, 16-byte aligned), the canonical check over the group, the log2_cell stages towards the
// coefficients, times (1 / h_k)^i / c with 1 / h_k = ishifts[cell_index[k]].  pre (may be NULL): a cell with pre[k] != 0 is out; so is one with an element >= r.  A cell that
// is out has all-zero coefficients.  st_out (may be NULL): pre[k], else NBLS_ST_NON_CANONICAL, else 0.
//   sum == 0 (rows): -a_(k,i) as 32 bytes big-endian to rows32[k * c + i], the rows of msm_rows_dev
//   sum != 0:        the lane adds w_k a_(k,i) over its rounds (w32: the weights, 32 bytes big-endian, < r) in registers; the workgroup's groups meet in an LDS tree and
//                    leave ONE row of c elements, partial[blockIdx.x * c + i], plain limbs -- kzg_cell_sum_kernel adds the rows.  No coefficient goes to memory
template <bool sum>   // (two kernels, so that a trace tells the modes apart)
__global__ void __launch_bounds__(CL) kzg_cell_interp_kernel(u32 log2_cell, u32 n_cells, const uint8_t* __restrict__ cells, const u32* __restrict__ cell_index,
                                                             const int8_t* __restrict__ pre, const uint8_t* __restrict__ w32, const Fr* __restrict__ iroots,
                                                             const Fr* __restrict__ ishifts, uint8_t* __restrict__ rows32, Fr* __restrict__ partial, int8_t* __restrict__ st_out) {
  __shared__ Fr part[CL];
  const u32 t = threadIdx.x, c = 1u << log2_cell, i = t & (c - 1);
  const u32 groups = (gridDim.x * CL) >> log2_cell, q = (blockIdx.x * CL + t) >> log2_cell, rounds = (n_cells + groups - 1) / groups;
  Fr acc = fr_zero();
  for (u32 w = 0; w < rounds; w++) {
    const u64 k = (u64)q + (u64)w * groups;
    const bool valid = k < n_cells;
    const u32 kk = valid ? (u32)k : n_cells - 1;
    Fr v = fr_load_q(cells + (((u64)kk << log2_cell) + i) * 32);
    u32 bad = fr_ge_r_mask(v);
    for (u32 m = 1; m < c; m <<= 1) bad |= (u32)__shfl_xor((int)bad, (int)m);
    const int p = pre ? pre[kk] : 0;
    const u32 out = bad | ((u32)0 - (u32)(p != 0)) | ((u32)0 - (u32)!valid);
    v = fr_select(bad, fr_zero(), v);
    for (u32 ll = 0; ll < log2_cell; ll++) v = fr_cell_stage(v, fr_lane_xor(v, 1u << ll), i, ll, log2_cell, iroots);
    const Fr a = fr_cell_coeff(v, ishifts[cell_index[kk]], i, log2_cell, out);
    if (sum) acc = fr_add(acc, fr_mul(a, fr_mul(fr_load_q(w32 + 32ull * kk), fr_r2())));
    else if (valid) fr_store_q(fr_neg(a), rows32 + (((u64)kk << log2_cell) + i) * 32);
    if (st_out && valid && i == 0) st_out[kk] = (int8_t)fr_cell_status(p, bad);
  }
  if (!sum) return;   // (uniform)
  const FrWorkgroup<CL> lanes;
  lanes.phase([&](u32 l) { part[l] = acc; });
  fr_tree(lanes, part, c);   // (every wavefront meets every barrier)
  if (t < c) partial[(u64)blockIdx.x * c + t] = part[t];
}
// out32[i] = -(sum over the n_parts partial rows of column i) mod r as 32 bytes big-endian, i < c: one workgroup, lane group g on the rows g, g + groups, ..
__global__ void __launch_bounds__(CL) kzg_cell_sum_kernel(u32 log2_cell, u32 n_parts, const Fr* __restrict__ partial, uint8_t* __restrict__ out32) {
  __shared__ Fr part[CL];
  kzg_cell_sum_body(FrWorkgroup<CL>(), log2_cell, n_parts, partial, out32, part);
}
// pre0[k]: what the two decoders say about cell k before its elements are looked at -- the named commitment's status if >= 2, else 10 + the proof's if >= 2, else 0
__global__ void kzg_cell_pre_kernel(u32 n, const int8_t* __restrict__ dstc, const int8_t* __restrict__ dstp, const u32* __restrict__ ci, int8_t* __restrict__ pre0) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int sc = dstc[ci[k]], sp = dstp[k];
  pre0[k] = (int8_t)kzg_pre_status(sc, sp, 0);
}
// kzg_items_kernel's part for cells, one cell per lane.  dstc / affc: the decoder's statuses and points of the commitments, named by ci[k]; dstp / affp: of the n proofs; pre:
// the cells' statuses before any pairing (kzg_cell_interp_kernel's st_out); sroots: the table of the M roots, s_k = entry cell_index[k].  A cell with pre != 0 gets zero
// scalars everywhere; a zero point takes part as the identity: zero scalars for that point alone.  The commitment of every cell is gathered into gath (its status into gst),
// and every point that a zero scalar stands for is the generator, so that the MSMs read points of the curve only.
//   s1[k] = r_k (the 64-bit MSM over the proofs);  s2[k] = r_k (over the gathered commitments);  s3[k] = r_k s_k mod r (the 256-bit MSM over the proofs);
//   zs[k] = s_k (the ladder of the per-cell pass; zero where the cell is out or its proof is the zero point)
__global__ void kzg_cell_items_kernel(u32 n, const int8_t* __restrict__ dstc, const int8_t* __restrict__ dstp, const u32* __restrict__ ci, const u32* __restrict__ cell_index,
                                      const int8_t* __restrict__ pre, const uint8_t* __restrict__ w32, const Fr* __restrict__ sroots, const uint8_t* __restrict__ gen96,
                                      const uint8_t* __restrict__ affc, uint8_t* __restrict__ affp, uint8_t* __restrict__ gath, int8_t* __restrict__ gst,
                                      uint8_t* __restrict__ s1, uint8_t* __restrict__ s2, uint8_t* __restrict__ s3, uint8_t* __restrict__ zs) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int sc = dstc[ci[k]], sp = dstp[k];
  const u32 live = (u32)0 - (u32)(pre[k] == 0), use_c = live & ((u32)0 - (u32)(sc == 0)), use_p = live & ((u32)0 - (u32)(sp == 0));
  const Fr zero = fr_zero(), r = fr_load_be(w32 + 32ull * k), sk = sroots[cell_index[k]];
  fr_store_be(fr_select(use_p, r, zero), s1 + 32ull * k);
  fr_store_be(fr_select(use_c, r, zero), s2 + 32ull * k);
  fr_store_be(fr_select(use_p, fr_mul(r, sk), zero), s3 + 32ull * k);
  fr_store_be(fr_select(use_p, fr_from_mont(sk), zero), zs + 32ull * k);
  gst[k] = (int8_t)sc;
  copy96(gath + 96ull * k, use_c ? affc + 96ull * ci[k] : gen96);
  if (!use_p) copy96(affp + 96ull * k, gen96);
}

// The running products of N = 4096 take more than the 64 KB a launch may ask for by default.  The limit is a per-device function attribute: set once on every device a launch of
// `kernel` is made on (as nbls_vm_launch does); the common case, already set, takes no lock.  The flags of the four kernels that ask for it live here
enum LdsKernel { LDS_EVAL, LDS_QUOTIENT, LDS_NTT, LDS_RECOVER, LDS_NTT_PASS, LDS_NTT_TAIL, LDS_KERNELS };
int lds_limit(LdsKernel which, const void* kernel) {
  static std::atomic<bool> attr_set[LDS_KERNELS][64];
  static std::mutex attr_mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  std::atomic<bool>& set = attr_set[which][dev];
  if (!set.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> g(attr_mu);
    if (!set.load(std::memory_order_relaxed)) {
      const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * FR_NL * EV * 4);
      if (e != hipSuccess) return (int)e;
      set.store(true, std::memory_order_release);
    }
  }
  return 0;
}
}  // namespace

extern "C" {
int nbls_kzg_roots_launch(unsigned log2_n, void* table, hipStream_t stream) { return launch_1d(kzg_roots_kernel, (u64)1 << log2_n, 64, 0, stream, log2_n, table); }
// n polynomials of 2^log2_n elements each (1 <= log2_n <= 12) at their points z -> out32 (n x 32 bytes) and status (n bytes, not NULL)
int nbls_kzg_eval_launch(unsigned log2_n, unsigned n, const void* evals32, const void* z32, const void* roots, void* out32, void* status, hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 12) return (int)hipErrorInvalidValue;
  const unsigned terms = ((1u << log2_n) + EV - 1) / EV, lds = terms * FR_NL * EV * 4;
  const int e = lds_limit(LDS_EVAL, (const void*)kzg_eval_kernel);
  return e ? e : launch_1d(kzg_eval_kernel, (u64)n * EV, EV, lds, stream, log2_n, evals32, z32, roots, out32, status);
}
// the same n polynomials -> out_y32 (n x 32), the quotient rows out_q32 (n x 2^log2_n x 32 bytes, 16-byte aligned) and status (n bytes, not NULL)
int nbls_kzg_quotient_launch(unsigned log2_n, unsigned n, const void* evals32, const void* z32, const void* roots, void* out_y32, void* out_q32, void* status,
                             hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 12 || ((uintptr_t)out_q32 & 15)) return (int)hipErrorInvalidValue;
  const unsigned terms = ((1u << log2_n) + EV - 1) / EV, lds = terms * FR_NL * EV * 4;
  const int e = lds_limit(LDS_QUOTIENT, (const void*)kzg_quotient_kernel);
  return e ? e : launch_1d(kzg_quotient_kernel, (u64)n * EV, EV, lds, stream, log2_n, evals32, z32, roots, out_y32, out_q32, status);
}
int nbls_kzg_inv_roots_launch(unsigned log2_n, const void* roots, void* table, hipStream_t stream) {
  return launch_1d(kzg_inv_roots_kernel, (u64)1 << log2_n, 64, 0, stream, log2_n, roots, table);
}
// n polynomials of 2^log2_n elements through kzg_ntt_kernel (mode: FrNttMode; the arrays as the kernel states them; shift32, coef32 and status may be NULL)
int nbls_kzg_ntt_launch(unsigned log2_n, unsigned mode, unsigned n, const void* in32, const void* shift32, unsigned shift_stride, const void* roots, const void* iroots,
                        void* out32, void* coef32, void* status, hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 12 || mode > FR_NTT_CELLS || (mode == FR_NTT_CELLS && !shift32) || (((uintptr_t)in32 | (uintptr_t)out32 | (uintptr_t)coef32) & 15))
    return (int)hipErrorInvalidValue;
  const int e = lds_limit(LDS_NTT, (const void*)kzg_ntt_kernel);
  const u64 out_stride = (u64)(mode == FR_NTT_CELLS ? 64 : 32) << log2_n;
  return e ? e : launch_1d(kzg_ntt_kernel, (u64)n * NT, NT, 32u << log2_n, stream, log2_n, mode, in32, shift32, shift_stride, roots, iroots, out32, out_stride, coef32, status);
}
// run R of the global stages of n polynomials of 2^R.log2_n elements (R: fr_nttl_run's; table: the roots, or the inverse roots where `inverse`, of the size the global
// stages have together; in32 == out32, or disjoint; shift32 / sinv / status may be NULL; flags: n words)
int nbls_kzg_ntt_pass_launch(const nbls::FrNttRun* run, unsigned inverse, unsigned n, const void* in32, void* out32, const void* shift32, const void* sinv, const void* table,
                             void* flags, void* status, hipStream_t stream) {
  if (!n) return 0;
  const FrNttRun R = *run;
  if (R.log2_n < 2 || R.log2_n > FR_NTTL_MAX_LOG2 || !R.q || R.q > FR_NTTL_MAX_PASS || !R.c || R.c > FR_NTT_LOG2_LANES || R.q + R.c > FR_NTTL_MAX_TILE || R.j0 + R.q + R.c > R.log2_n ||
      R.j0 + R.q > 12 || ((u64)n << R.log2_n) > ((u64)1 << FR_NTTL_MAX_LOG2) || !flags || (((uintptr_t)in32 | (uintptr_t)out32) & 15))
    return (int)hipErrorInvalidValue;
  const int e = lds_limit(LDS_NTT_PASS, (const void*)kzg_ntt_pass_kernel);
  return e ? e : launch_1d(kzg_ntt_pass_kernel, ((u64)n << (R.log2_n - R.q - R.c)) * NT, NT, 32u << (R.q + R.c), stream, R, inverse, in32, out32, shift32, sinv, table, flags, status);
}
// the 2^log2_k tails of 2^log2_t elements of each of n polynomials (w32: omega_N, or its inverse where `inverse`, as 8 words in Montgomery form; roots / iroots: the
// tables of size 2^log2_t; sinv: n elements; flags: n words; shift32 and status may be NULL)
int nbls_kzg_ntt_tail_launch(unsigned log2_t, unsigned log2_k, unsigned inverse, unsigned n, const uint32_t* w32, const void* in32, void* out32, const void* shift32, void* sinv,
                             const void* roots, const void* iroots, void* flags, void* status, hipStream_t stream) {
  if (!n) return 0;
  if (log2_t < 1 || log2_t > FR_NTTL_MAX_TAIL || log2_k < 1 || log2_k > 12 || ((u64)n << (log2_t + log2_k)) > ((u64)1 << FR_NTTL_MAX_LOG2) || !sinv || !flags ||
      (((uintptr_t)in32 | (uintptr_t)out32) & 15))
    return (int)hipErrorInvalidValue;
  Fr w;
  for (int i = 0; i < FR_NL; i++) w.l[i] = w32[i];
  const int e = lds_limit(LDS_NTT_TAIL, (const void*)kzg_ntt_tail_kernel);
  return e ? e : launch_1d(kzg_ntt_tail_kernel, ((u64)n << log2_k) * NT, NT, 32u << log2_t, stream, log2_t, log2_k, inverse, w, in32, out32, shift32, sinv, roots, iroots, flags, status);
}
// the quotient rows of n blobs (n << (log2_n + 1) lanes; the table of 2^(log2_n + 1 - log2_cell) roots has at most 2^12 entries)
int nbls_kzg_cell_rows_launch(unsigned log2_n, unsigned log2_cell, unsigned n, const void* coef32, const void* sroots, const void* blob_st, void* out_q32, void* row_st,
                              hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 12 || (((uintptr_t)coef32 | (uintptr_t)out_q32) & 15)) return (int)hipErrorInvalidValue;
  return launch_1d(kzg_cell_rows_kernel, (u64)n << (log2_n + 1), 256, 0, stream, log2_n, log2_cell, n, coef32, sroots, blob_st, out_q32, row_st);
}
// n blobs through kzg_recover_z_kernel and kzg_recover_kernel (the arrays as the kernels state them; slot: n << log2_m words, log2_m = log2_n + 1 - log2_cell <= 12; zv: room for
// 3 n << (log2_m - 1) elements; out32: n rows of 2 N elements; coef32: n rows of N, never NULL; status: n bytes, never NULL).  Two launches, whatever n is
int nbls_kzg_recover_launch(unsigned log2_n, unsigned log2_cell, unsigned n, const void* cells, const uint32_t* slot, const void* pre, const void* sroots, const void* consts,
                            const void* roots, const void* iroots, void* zv, void* out32, void* coef32, void* status, hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 12 || !coef32 || !status || (((uintptr_t)cells | (uintptr_t)out32 | (uintptr_t)coef32) & 15))
    return (int)hipErrorInvalidValue;
  const unsigned log2_m = log2_n + 1 - log2_cell;
  int e = lds_limit(LDS_RECOVER, (const void*)kzg_recover_kernel);
  if (!e) e = launch_1d(kzg_recover_z_kernel, (u64)n * (3u << (log2_m - 1)), 256, 0, stream, log2_m, n, slot, pre, sroots, consts, zv);
  return e ? e : launch_1d(kzg_recover_kernel, (u64)n * NT, NT, 32u << log2_n, stream, log2_n, log2_cell, cells, slot, pre, zv, consts, roots, iroots, out32, coef32, status);
}
// evals32: n blobs of 2^log2_n elements, 16-byte aligned, zeroed in place where non-canonical
int nbls_kzg_canon_launch(unsigned log2_n, unsigned n, void* evals32, void* status, hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 12 || ((uintptr_t)evals32 & 15)) return (int)hipErrorInvalidValue;
  return launch_1d(kzg_canon_kernel, (u64)n * 256, 256, 0, stream, log2_n, evals32, status);
}
int nbls_kzg_prove_tail_launch(unsigned n, const void* zero, const void* st_a, const void* st_b, void* out48, void* status, hipStream_t stream) {
  if (n && ((uintptr_t)out48 & 15)) return (int)hipErrorInvalidValue;
  return launch_1d(kzg_prove_tail_kernel, n, 256, 0, stream, n, zero, st_a, st_b, out48, status);
}
int nbls_kzg_items_launch(unsigned n, const void* dst, const void* w32, const void* z32, const void* y32, const void* yst, const void* gen96, void* aff, void* s1, void* s2,
                          void* t, void* pre, hipStream_t stream) {
  if (!n) return 0;
  const int e = launch_1d(kzg_items_kernel, n, 64, 0, stream, n, dst, w32, z32, y32, yst, gen96, aff, s1, s2, t, pre);
  return e ? e : launch_1d(kzg_sum_kernel, EV, EV, 0, stream, n, t, (uint8_t*)s2 + 64ull * n);
}
// the scalars of pass A for n blobs (log2_m = log2_n + 1 - log2_cell <= 11: at most 64 KB of LDS; coef32 and out32 16-byte aligned)
int nbls_kzg_fk20_scalars_launch(unsigned log2_n, unsigned log2_cell, unsigned n, const void* coef32, const void* sroots, void* out32, hipStream_t stream) {
  if (!n) return 0;
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 11 || (((uintptr_t)coef32 | (uintptr_t)out32) & 15)) return (int)hipErrorInvalidValue;
  const unsigned lm = log2_n + 1 - log2_cell;
  return launch_1d(kzg_fk20_scalars_kernel, (u64)fr_fk_workgroups(lm, log2_cell, n) * FR_FK_LANES, FR_FK_LANES, fr_fk_lds_words(lm) * 4, stream, log2_n, log2_cell, n, coef32, sroots,
                   out32);
}
int nbls_kzg_fk20_row_status_launch(unsigned log2_m, unsigned n, const void* blob_st, void* row_st, hipStream_t stream) {
  return launch_1d(kzg_fk20_row_status_kernel, (u64)n << log2_m, 256, 0, stream, log2_m, n, blob_st, row_st);
}
// the c M (n' - 1) scalars of the handle's MSM (none for n' = 1)
int nbls_kzg_fk20_powers_launch(unsigned log2_n, unsigned log2_cell, const void* sroots, void* out32, hipStream_t stream) {
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 11 || ((uintptr_t)out32 & 15)) return (int)hipErrorInvalidValue;
  const unsigned lm = log2_n + 1 - log2_cell;
  const u64 count = ((u64)1 << (log2_cell + lm)) * ((1u << (lm - 1)) - 1);
  if (count >> 32) return (int)hipErrorInvalidValue;
  return launch_1d(kzg_fk20_powers_kernel, count, 256, 0, stream, log2_cell, lm, (u32)count, sroots, out32);
}
int nbls_kzg_fk20_matrix_launch(unsigned log2_m, const void* sroots, const void* isroots, void* out32, hipStream_t stream) {
  if (log2_m < 1 || log2_m > 11 || ((uintptr_t)out32 & 15)) return (int)hipErrorInvalidValue;
  return launch_1d(kzg_fk20_matrix_kernel, (u64)1 << (2 * log2_m), 256, 0, stream, log2_m, sroots, isroots, out32);
}
// the table of the 2^log2_m inverse shifts of (log2_n, log2_cell = log2_n + 1 - log2_m)
int nbls_kzg_cell_ishifts_launch(unsigned log2_n, unsigned log2_m, void* table, hipStream_t stream) {
  if (log2_n < 1 || log2_n > 12 || log2_m < 1 || log2_m > log2_n + 1) return (int)hipErrorInvalidValue;
  return launch_1d(kzg_cell_ishifts_kernel, (u64)1 << log2_m, 64, 0, stream, log2_n, log2_m, table);
}
// n_cells cells through kzg_cell_interp_kernel (the arrays as the kernel states them; cells, w32, rows32 and out32 16-byte aligned).  sum == 0: the rows to rows32.  Else the
// -S_i to out32 (c x 32 bytes) by way of `partial`, which holds fr_cell_workgroups(n_cells, log2_cell, true) rows of c elements
int nbls_kzg_cell_interp_launch(unsigned log2_cell, unsigned n_cells, int sum, const void* cells, const uint32_t* cell_index, const void* pre, const void* w32, const void* iroots,
                                const void* ishifts, void* rows32, void* partial, void* out32, void* st_out, hipStream_t stream) {
  if (!n_cells) return 0;
  if (log2_cell > 6 || (((uintptr_t)cells | (uintptr_t)w32 | (uintptr_t)rows32 | (uintptr_t)out32 | (uintptr_t)partial) & 15) || (sum ? !w32 || !partial || !out32 : !rows32) ||
      (log2_cell && !iroots))
    return (int)hipErrorInvalidValue;
  const unsigned wg = fr_cell_workgroups(n_cells, log2_cell, sum != 0);
  const int e = launch_1d(sum ? kzg_cell_interp_kernel<true> : kzg_cell_interp_kernel<false>, (u64)wg * CL, CL, 0, stream, log2_cell, n_cells, cells, cell_index, pre, w32, iroots,
                          ishifts, rows32, partial, st_out);
  return e || !sum ? e : launch_1d(kzg_cell_sum_kernel, CL, CL, 0, stream, log2_cell, wg, partial, out32);
}
int nbls_kzg_cell_pre_launch(unsigned n, const void* dstc, const void* dstp, const uint32_t* ci, void* pre0, hipStream_t stream) {
  return launch_1d(kzg_cell_pre_kernel, n, 256, 0, stream, n, dstc, dstp, ci, pre0);
}
int nbls_kzg_cell_items_launch(unsigned n, const void* dstc, const void* dstp, const uint32_t* ci, const uint32_t* cell_index, const void* pre, const void* w32, const void* sroots,
                               const void* gen96, const void* affc, void* affp, void* gath, void* gst, void* s1, void* s2, void* s3, void* zs, hipStream_t stream) {
  return launch_1d(kzg_cell_items_kernel, n, 64, 0, stream, n, dstc, dstp, ci, cell_index, pre, w32, sroots, gen96, affc, affp, gath, gst, s1, s2, s3, zs);
}
int nbls_kzg_item_scalars_launch(unsigned n, const void* pre, const void* dst, const void* z32, const void* y32, void* zs, void* ny, hipStream_t stream) {
  return launch_1d(kzg_item_scalars_kernel, n, 64, 0, stream, n, pre, dst, z32, y32, zs, ny);
}
int nbls_kzg_item_status_launch(unsigned n, const void* pre, const void* pst, const void* xzero, const void* one, void* status, hipStream_t stream) {
  return launch_1d(kzg_item_status_kernel, n, 256, 0, stream, n, pre, pst, xzero, one, status);
}
}
