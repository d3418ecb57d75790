// fr_workgroup.h -- the workgroup choreography of the Fr kernels, written once: which lanes do what between which two barriers, the LDS trees, the shared flags, the uniform
// early exits.  fr_exec.h has what ONE lane does; this file has what a workgroup does with it, as function templates over a workgroup view that exists twice:
//   device   phase(f) = f(threadIdx.x), then __syncthreads()          (kzg_kernels.hip, groth16_kernels.hip: a __global__ function is its index arithmetic, its __shared__
//                                                                      declarations and one call)
//   host     phase(f) = f(t) for every lane t of the workgroup, in turn  (vm_sim.cpp: an entry point is its argument rules, its tables, a loop over workgroups, the same call)
// The host model is faithful under two rules.  Everything a lane does between two barriers sits in ONE phase -- a lane that scales, stores and reloads only its own elements
// does so inside one lambda.  And no per-lane value lives across a barrier: what a body keeps outside its lambdas is the same on every lane of the workgroup (arguments, what
// it reads from shared memory behind a barrier), so the host computes it once.  Within a phase the lanes are then independent, and the host may visit them in either order
// (nbls_sim_set_lane_order): a phase whose result depends on the order is a missing barrier here.
// Left out on purpose: kzg_cell_interp_kernel and g16_input_sums_kernel exchange registers across lanes, fr_lagrange_kernel carries a per-lane state across its tile barriers;
// they keep their bodies (and their re-enactments in vm_sim.cpp) and share the tree and the closing sums below.
#pragma once
#include <stdint.h>
#include <string.h>
#include "fr_exec.h"
#include "../../include/nbls.h"   // NBLS_ST_*

namespace nbls {
enum { FR_ST_ZERO_DIVISOR = 5 };   // a shift that is 0 mod r: the status nbls_fr_op_batch gives INV / DIV of zero (nbls.h names no constant for it)

#if defined(__HIPCC__)
// (forced: left to its own estimate the compiler makes functions of some bodies, and a view or a local passed by address to a function costs the kernel a stack)
#define NBLS_WG_FN __device__ __forceinline__
template <uint32_t LANES> struct FrWorkgroup {
  __device__ static constexpr uint32_t lanes() { return LANES; }
  template <class F> __device__ __forceinline__ void phase(F f) const { f((uint32_t)threadIdx.x); __syncthreads(); }
  template <class F> __device__ __forceinline__ void last(F f) const { f((uint32_t)threadIdx.x); }
  __device__ void raise(uint32_t* flag) const { atomicOr(flag, 0xffffffffu); }
  __device__ void raise(uint32_t* flag, uint32_t bits) const { atomicOr(flag, bits); }
};
#else
#define NBLS_WG_FN inline
template <uint32_t LANES> struct FrWorkgroup {
  bool descending;   // the lanes of a phase from the top down
  static constexpr uint32_t lanes() { return LANES; }
  template <class F> void phase(F f) const { last(f); }
  template <class F> void last(F f) const { for (uint32_t i = 0; i < LANES; i++) f(descending ? LANES - 1 - i : i); }
  void raise(uint32_t* flag) const { *flag = 0xffffffffu; }
  void raise(uint32_t* flag, uint32_t bits) const { *flag |= bits; }
};
#endif

// the lane's 16-byte vectors t, t + lanes, .. of `count`: zeros to dst, or src's (both 16-byte aligned)
NBLS_WG_FN void fr_lane_zero16(uint8_t* dst, uint64_t count, uint32_t lane, uint32_t lanes) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (uint64_t j = lane; j < count; j += lanes) ((uint4*)dst)[j] = make_uint4(0u, 0u, 0u, 0u);
#else
  for (uint64_t j = lane; j < count; j += lanes) memset(dst + 16 * j, 0, 16);
#endif
}
NBLS_WG_FN void fr_lane_copy16(uint8_t* dst, const uint8_t* src, uint32_t count, uint32_t lane, uint32_t lanes) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (uint32_t j = lane; j < count; j += lanes) ((uint4*)dst)[j] = ((const uint4*)src)[j];
#else
  for (uint32_t j = lane; j < count; j += lanes) memcpy(dst + 16ull * j, src + 16ull * j, 16);
#endif
}

// THE tree: part[] holds one value per lane, written in an earlier phase; the sums of the lanes t, t + width, t + 2 width, .. to part[t], t < width (a power of two), by
// modular additions.  Ends behind a barrier
template <class WG> NBLS_WG_FN void fr_tree(WG wg, Fr* part, uint32_t width) {
  for (uint32_t s = wg.lanes() / 2; s >= width && s > 0; s >>= 1) wg.phase([&](uint32_t t) { if (t < s) part[t] = fr_add(part[t], part[t + s]); });
}

// ---- Evaluation and quotient (kzg_eval_kernel, kzg_quotient_kernel; nbls_sim_fr_eval_roots, nbls_sim_fr_quotient_roots).  One workgroup of FR_EVAL_LANES lanes per polynomial.
// The walk both open with (KEEP: fr_eval_lane_t's) -> z in Montgomery form; behind a barrier part[0] = the sum, *sh_hit = the root z is (or all ones; the roots are distinct:
// at most one lane writes it), *sh_bad = an element or z >= r.  pre: terms x 8 x lanes words
template <bool KEEP, class WG>
NBLS_WG_FN Fr kzg_eval_walk(WG wg, unsigned log2_n, const uint8_t* f32, const uint8_t* z32, const Fr* roots, uint32_t* pre, Fr* part, uint32_t* sh_hit, uint32_t* sh_bad) {
  const uint32_t N = 1u << log2_n;
  const Fr zraw = fr_load_be(z32), z = fr_mul(zraw, fr_r2());
  wg.phase([&](uint32_t t) { if (t == 0) { *sh_hit = 0xffffffffu; *sh_bad = fr_ge_r_mask(zraw); } });
  wg.phase([&](uint32_t t) {
    const FrEvalPart me = fr_eval_lane_t<KEEP>(f32, roots, z, N, t, wg.lanes(), pre);
    part[t] = me.sum;
    if (me.hit != 0xffffffffu) *sh_hit = me.hit;
    if (me.bad) wg.raise(sh_bad);
  });
  fr_tree(wg, part, 1);
  return z;
}
template <class WG>
NBLS_WG_FN void kzg_eval_body(WG wg, unsigned log2_n, const uint8_t* f32, const uint8_t* z32, const Fr* roots, uint8_t* out32, int8_t* status, uint32_t* pre, Fr* part,
                              uint32_t* sh_hit, uint32_t* sh_bad) {
  const Fr z = kzg_eval_walk<false>(wg, log2_n, f32, z32, roots, pre, part, sh_hit, sh_bad);
  wg.last([&](uint32_t t) { if (t == 0) *status = (int8_t)fr_eval_finish(part[0], *sh_hit, *sh_bad, z, log2_n, f32, out32); });
}
// The walk with the inverses 1 / (z - w_j) kept in the slots the running products came from, the tree for y, then a second walk over the lane's terms: q_j as 32 bytes
// big-endian and, where z is the root w_m (*sh_hit: the workgroup's), the products q_j w_j into a second tree over `part`; the lane that owns m closes with one inversion,
// q_m = -1 / z * sum.  A non-canonical input leaves a zero y and a zero row
template <class WG>
NBLS_WG_FN void kzg_quotient_body(WG wg, unsigned log2_n, const uint8_t* f32, const uint8_t* z32, const Fr* roots, uint8_t* y32, uint8_t* q32, int8_t* status,
                                  uint32_t* pre, Fr* part, Fr* sh_y, uint32_t* sh_hit, uint32_t* sh_bad) {
  const uint32_t N = 1u << log2_n;
  const Fr z = kzg_eval_walk<true>(wg, log2_n, f32, z32, roots, pre, part, sh_hit, sh_bad);
  const uint32_t hit = *sh_hit, bad = *sh_bad;
  wg.phase([&](uint32_t t) {
    if (t != 0) return;
    *sh_y = fr_select(bad, fr_zero(), fr_eval_value(part[0], hit, z, log2_n, f32));
    fr_store_be(*sh_y, y32);
    *status = (int8_t)(bad & NBLS_ST_NON_CANONICAL);
  });
  const Fr y = *sh_y;
  auto second = [&](uint32_t t) { part[t] = fr_quot_lane(f32, roots, y, hit, bad, N, t, wg.lanes(), pre, q32); };
  if (hit == 0xffffffffu) { wg.last(second); return; }
  wg.phase(second);
  fr_tree(wg, part, 1);
  wg.last([&](uint32_t t) { if (t == hit % wg.lanes()) fr_store_q(fr_select(bad, fr_zero(), fr_quot_within(part[0], z)), q32 + 32ull * hit); });
}

// ---- The transform (kzg_ntt_kernel; nbls_sim_fr_ntt, nbls_sim_kzg_cells) and the recovery (kzg_recover_kernel; nbls_sim_kzg_recover): FR_NTT_LANES lanes per polynomial, the
// polynomial in `a` (8 N words of shared memory), one barrier per stage.  All stages of one direction: towards the coefficients (`inverse`, table = the inverse roots) or the values
template <class WG> NBLS_WG_FN void fr_ntt_stages(WG wg, uint32_t* a, unsigned log2_n, bool inverse, const Fr* table) {
  for (unsigned k = 0; k < log2_n; k++) wg.phase([&](uint32_t t) { fr_ntt_stage(a, log2_n, inverse ? k : log2_n - 1 - k, inverse, table, t, wg.lanes()); });
}
// mode (FrNttMode):
//   TO_COEFFS  values in -> the stages with the inverse roots -> times 1 / N and (1 / s)^i -> coefficients out
//   TO_EVALS   coefficients in, times s^i -> the stages with the roots -> values out
//   CELLS      a blob in (shift32 = g = omega_2N) -> its bytes to the first half of the output row -> coefficients (to c32 as well, where given) -> times g^i -> values on
//              the coset to the second half
// f32 / o32 / c32: the polynomial's rows, 16-byte aligned; shift32, c32 and status may be NULL; out_stride = the bytes of the output row.  An element or a shift >= r
// (NBLS_ST_NON_CANONICAL), or a shift that is 0 mod r (FR_ST_ZERO_DIVISOR), leaves all-zero rows; the branch is the workgroup's.  One lane inverts the shift on the way to the
// coefficients; the others wait
template <class WG>
NBLS_WG_FN void kzg_ntt_body(WG wg, unsigned log2_n, uint32_t mode, const uint8_t* f32, const uint8_t* shift32, const Fr* roots, const Fr* iroots, uint8_t* o32,
                             uint64_t out_stride, uint8_t* c32, int8_t* status, uint32_t* a, Fr* sh_s, uint32_t* sh_bad, uint32_t* sh_zero) {
  const uint32_t N = 1u << log2_n, L = wg.lanes();
  wg.phase([&](uint32_t t) {
    if (t != 0) return;
    uint32_t bad = 0, zero = 0;
    if (shift32) *sh_s = fr_ntt_shift(shift32, mode == FR_NTT_TO_COEFFS, &bad, &zero);
    *sh_bad = bad; *sh_zero = zero;
  });
  wg.phase([&](uint32_t t) { if (fr_ntt_load(f32, N, t, L, a)) wg.raise(sh_bad); });
  const int st = *sh_bad ? NBLS_ST_NON_CANONICAL : *sh_zero ? FR_ST_ZERO_DIVISOR : 0;
  if (st) {
    wg.last([&](uint32_t t) {
      if (t == 0 && status) *status = (int8_t)st;
      fr_lane_zero16(o32, out_stride / 16, t, L);
      if (c32) fr_lane_zero16(c32, 2 * N, t, L);
    });
    return;
  }
  const Fr s = shift32 ? *sh_s : fr_one(), ninv = fr_inv_pow2(log2_n);
  auto ok = [&](uint32_t t) { if (t == 0 && status) *status = 0; };
  if (mode == FR_NTT_TO_EVALS) {
    wg.phase([&](uint32_t t) { if (shift32) fr_ntt_scale(a, N, t, L, FR_NTT_LOG2_LANES, nullptr, &s, nullptr); });
  } else {
    fr_ntt_stages(wg, a, log2_n, true, iroots);
    if (mode == FR_NTT_TO_COEFFS) {
      wg.last([&](uint32_t t) { ok(t); fr_ntt_scale(a, N, t, L, FR_NTT_LOG2_LANES, &ninv, shift32 ? &s : nullptr, nullptr); fr_ntt_store(a, N, t, L, o32); });
      return;
    }
    wg.phase([&](uint32_t t) { fr_lane_copy16(o32, f32, 2 * N, t, L); fr_ntt_scale(a, N, t, L, FR_NTT_LOG2_LANES, &ninv, &s, c32); });
    o32 += (uint64_t)32 << log2_n;
  }
  fr_ntt_stages(wg, a, log2_n, false, roots);
  wg.last([&](uint32_t t) { ok(t); fr_ntt_store(a, N, t, L, o32); });
}
// One blob, six transforms of size N:
//   the canonical check of every given element -> E Z on H -> S (kept in the blob's row c32) -> E Z on gH -> D -> T 7^i -> the values on 7 H -> block j times
//   1 / Zs(7^c s_j) -> the coefficients of P (to c32: what the proofs read) -> the values on H, compared and written to the first half of the output row o32 -> the
//   coefficients again, times g^i -> the values on gH, compared and written to the second half.
// A lane scales, combines, stores and reloads its OWN elements t, t + lanes, .. only: such steps share a phase.  Status: pre (NBLS_ST_BAD_CELLS), else NBLS_ST_NON_CANONICAL,
// else NBLS_ST_INCONSISTENT where a recomputed element differs from a given one, else 0; a refused blob leaves an all-zero row and all-zero coefficients, and the branch is
// the workgroup's.  slot / zv: the blob's; cells / o32 / c32 are 16-byte aligned; c32 is read back by the lanes that wrote it
template <class WG>
NBLS_WG_FN void kzg_recover_body(WG wg, unsigned log2_n, unsigned log2_cell, const uint8_t* cells, const uint32_t* slot, int pre, const Fr* zv, const FrRecoverConsts& kc,
                                 const Fr* roots, const Fr* iroots, uint8_t* o32, uint8_t* c32, int8_t* status, uint32_t* a, uint32_t* sh_bad, uint32_t* sh_diff) {
  const uint32_t N = 1u << log2_n, L = wg.lanes(), M = 1u << (log2_n + 1 - log2_cell);
  const unsigned LL = FR_NTT_LOG2_LANES;
  wg.phase([&](uint32_t t) { if (t == 0) { *sh_bad = 0; *sh_diff = 0; } });
  int st = pre;
  wg.phase([&](uint32_t t) {
    if (!st && (fr_recover_load(cells, slot, zv, log2_n, log2_cell, 0, t, L, a) | fr_recover_load(cells, slot, zv, log2_n, log2_cell, 1, t, L, nullptr))) wg.raise(sh_bad);
  });
  if (!st && *sh_bad) st = NBLS_ST_NON_CANONICAL;
  if (!st) {
    const Fr ninv = fr_inv_pow2(log2_n);
    fr_ntt_stages(wg, a, log2_n, true, iroots);
    wg.phase([&](uint32_t t) {
      fr_ntt_scale(a, N, t, L, LL, &ninv, nullptr, c32);   // S
      fr_recover_load(cells, slot, zv, log2_n, log2_cell, 1, t, L, a);
    });
    fr_ntt_stages(wg, a, log2_n, true, iroots);
    wg.phase([&](uint32_t t) {
      fr_ntt_scale(a, N, t, L, LL, &ninv, &kc.ginv, nullptr);   // D
      fr_recover_combine(a, c32, N, t, L, LL, kc);
    });
    fr_ntt_stages(wg, a, log2_n, false, roots);
    wg.phase([&](uint32_t t) { fr_recover_divide(a, zv + M, N, log2_cell, t, L); });
    fr_ntt_stages(wg, a, log2_n, true, iroots);
    wg.phase([&](uint32_t t) {
      fr_ntt_scale(a, N, t, L, LL, &ninv, &kc.seveninv, nullptr);   // P
      fr_ntt_store(a, N, t, L, c32);
    });
    fr_ntt_stages(wg, a, log2_n, false, roots);
    wg.phase([&](uint32_t t) {
      if (fr_recover_compare(a, cells, slot, log2_n, log2_cell, 0, t, L)) wg.raise(sh_diff);
      fr_ntt_store(a, N, t, L, o32);
      fr_ntt_load(c32, N, t, L, a);
      fr_ntt_scale(a, N, t, L, LL, nullptr, &kc.g, nullptr);
    });
    fr_ntt_stages(wg, a, log2_n, false, roots);
    wg.phase([&](uint32_t t) {
      if (fr_recover_compare(a, cells, slot, log2_n, log2_cell, 1, t, L)) wg.raise(sh_diff);
      fr_ntt_store(a, N, t, L, o32 + ((uint64_t)32 << log2_n));
    });
    if (*sh_diff) st = NBLS_ST_INCONSISTENT;
  }
  wg.last([&](uint32_t t) {   // (behind a barrier in every case: the zeros follow the row's earlier stores)
    if (t == 0) *status = (int8_t)st;
    if (st) { fr_lane_zero16(o32, 4 * N, t, L); fr_lane_zero16(c32, 2 * N, t, L); }
  });
}

// ---- Transforms past one workgroup's LDS (kzg_ntt_pass_kernel, kzg_ntt_tail_kernel; nbls_sim_fr_ntt_large); fr_exec.h has the split.  A polynomial is seen by many
// workgroups, so what refuses it lives in global memory: one flag word per polynomial (FR_NTTL_BAD | FR_NTTL_ZERO), cleared in front of the call's first launch and raised
// atomically; no launch reads the word it may raise, and the launch that runs last turns a flagged row into zeros and writes the status (the workgroup `reader`, one per
// polynomial, which is also the one that looks at the caller's shift).
NBLS_WG_FN int fr_nttl_status(uint32_t flag) { return flag & FR_NTTL_BAD ? NBLS_ST_NON_CANONICAL : flag & FR_NTTL_ZERO ? FR_ST_ZERO_DIVISOR : 0; }
// One run of global stages on the tile (hi, lo0) of one polynomial: f32 -> o32 (the polynomial's rows; equal, or disjoint), the tile in `a`, one barrier per stage.
//   towards the values   the run with stage 0 checks the canonical form of what it reads and multiplies element g by s^g (shift32: the caller's, may be NULL)
//   towards the coefficients (`inverse`, table = the inverse roots)   the run with stage 0 is the call's last launch: times 1 / N and (1 / s)^g (sinv: what the tail
//                        launch left, Montgomery form; NULL: no shift), or zeros, and the status
template <class WG>
NBLS_WG_FN void kzg_ntt_pass_body(WG wg, const FrNttRun& R, bool inverse, uint32_t hi, uint32_t lo0, bool reader, const uint8_t* f32, uint8_t* o32, const uint8_t* shift32,
                                  const Fr* sinv, const Fr* table, uint32_t* flag, int8_t* status, uint32_t* a) {
  const uint32_t L = wg.lanes(), lt = R.q + R.c;
  const bool first = R.j0 == 0;
  auto stage = [&](uint32_t k) { wg.phase([&](uint32_t t) { fr_run_stage(a, lt, lt - 1 - k, inverse, R.j0 + k == 0, table + ((size_t)hi << (k + 1)), t, L); }); };
  if (!inverse) {
    const Fr s = first && shift32 ? fr_from_bytes(shift32) : fr_one();
    wg.phase([&](uint32_t t) {
      const uint32_t bad = fr_run_load(R, f32, hi, lo0, t, L, a);
      if (!first) return;
      if (bad) wg.raise(flag, FR_NTTL_BAD);
      if (!shift32) return;
      if (reader && t == 0) {
        if (fr_ge_r_mask(fr_load_be(shift32))) wg.raise(flag, FR_NTTL_BAD);
        if (fr_is_zero_mask(s)) wg.raise(flag, FR_NTTL_ZERO);
      }
      fr_run_scale(a, R, lo0, t, L, FR_NTT_LOG2_LANES, nullptr, &s);
    });
    for (uint32_t k = 0; k < R.q; k++) stage(k);
    wg.last([&](uint32_t t) { fr_run_store(R, a, false, hi, lo0, t, L, o32); });
    return;
  }
  wg.phase([&](uint32_t t) { fr_run_load(R, f32, hi, lo0, t, L, a); });
  for (uint32_t k = R.q; k-- > 0;) stage(k);
  if (!first) { wg.last([&](uint32_t t) { fr_run_store(R, a, false, hi, lo0, t, L, o32); }); return; }
  const int st = fr_nttl_status(*flag);
  const Fr ninv = fr_inv_pow2(R.log2_n), si = sinv ? *sinv : fr_one();
  wg.last([&](uint32_t t) {
    if (reader && t == 0 && status) *status = (int8_t)st;
    if (!st) fr_run_scale(a, R, lo0, t, L, FR_NTT_LOG2_LANES, &ninv, sinv ? &si : nullptr);
    fr_run_store(R, a, st != 0, hi, lo0, t, L, o32);
  });
}
// One tail: block B of a polynomial (2^log2_t contiguous elements, f32 -> o32; B < 2^log2_k) through the stages of kzg_ntt_body with the shift s_B = w^rev(B), which one
// lane computes (w = omega_N towards the values, 1 / omega_N towards the coefficients; Montgomery form).
//   towards the values   the call's last launch: a flagged polynomial's blocks come out as zeros, and block 0 writes the status
//   towards the coefficients (`inverse`)   the call's first: the canonical check; block 0 looks at the caller's shift (shift32, may be NULL) and leaves 1 / s in *sinv.
//                        The factor 1 / 2^log2_t waits for the last run
template <class WG>
NBLS_WG_FN void kzg_ntt_tail_body(WG wg, unsigned log2_t, unsigned log2_k, bool inverse, uint32_t B, const Fr& w, const uint8_t* f32, uint8_t* o32, const uint8_t* shift32,
                                  Fr* sinv, const Fr* roots, const Fr* iroots, uint32_t* flag, int8_t* status, uint32_t* a, Fr* sh_s) {
  const uint32_t N = 1u << log2_t, L = wg.lanes();
  wg.phase([&](uint32_t t) {
    if (t != 0) return;
    *sh_s = fr_pow_index(w, fr_bitrev(B, log2_k), FR_NTTL_MAX_TAIL);   // (the exponent has at most 12 bits: all of them are walked, as fr_root_entry does)
    if (inverse && B == 0 && shift32) {
      uint32_t bad = 0, zero = 0;
      *sinv = fr_ntt_shift(shift32, true, &bad, &zero);
      if (bad) wg.raise(flag, FR_NTTL_BAD);
      if (zero) wg.raise(flag, FR_NTTL_ZERO);
    }
  });
  const Fr s = *sh_s;
  if (inverse) {
    wg.phase([&](uint32_t t) { if (fr_ntt_load(f32, N, t, L, a)) wg.raise(flag, FR_NTTL_BAD); });
    fr_ntt_stages(wg, a, log2_t, true, iroots);
    wg.last([&](uint32_t t) { fr_ntt_scale(a, N, t, L, FR_NTT_LOG2_LANES, nullptr, &s, nullptr); fr_ntt_store(a, N, t, L, o32); });
    return;
  }
  const int st = fr_nttl_status(*flag);
  if (st) {
    wg.last([&](uint32_t t) { if (B == 0 && t == 0 && status) *status = (int8_t)st; fr_lane_zero16(o32, 2 * N, t, L); });
    return;
  }
  wg.phase([&](uint32_t t) { fr_ntt_load(f32, N, t, L, a); fr_ntt_scale(a, N, t, L, FR_NTT_LOG2_LANES, nullptr, &s, nullptr); });
  fr_ntt_stages(wg, a, log2_t, false, roots);
  wg.last([&](uint32_t t) { if (B == 0 && t == 0 && status) *status = 0; fr_ntt_store(a, N, t, L, o32); });
}

// ---- The per-blob scalars of FK20's pass A (kzg_fk20_scalars_kernel; nbls_sim_kzg_fk20_scalars): workgroup `block` of FR_FK_LANES lanes, its stripes side by side in `a`
// (fr_fk_lds_words), one barrier per stage.  What a lane is (fr_fk_lane) follows from its number alone: every phase asks again
template <class WG>
NBLS_WG_FN void kzg_fk20_scalars_body(WG wg, unsigned log2_n, unsigned log2_cell, uint32_t n, uint32_t block, const uint8_t* coef32, const Fr* sroots, uint8_t* out32,
                                      uint32_t* a) {
  const unsigned lm = log2_n + 1 - log2_cell;
  wg.phase([&](uint32_t t) { fr_fk_load(coef32, log2_n, log2_cell, lm, fr_fk_lane(lm, log2_cell, n, block, t), a); });
  for (unsigned ll = lm; ll-- > 0;) wg.phase([&](uint32_t t) { fr_fk_stage(a, lm, ll, sroots, fr_fk_lane(lm, log2_cell, n, block, t)); });
  wg.last([&](uint32_t t) { fr_fk_store(a, log2_cell, lm, fr_fk_lane(lm, log2_cell, n, block, t), out32); });
}

// ---- A blob that is only committed to (kzg_canon_kernel; nbls_sim_kzg_canon): *status = NBLS_ST_NON_CANONICAL where an element is >= r, and the blob is then zeroed in place
template <class WG> NBLS_WG_FN void kzg_canon_body(WG wg, unsigned log2_n, uint8_t* f32, int8_t* status, uint32_t* sh_bad) {
  const uint32_t N = 1u << log2_n;
  wg.phase([&](uint32_t t) { if (t == 0) *sh_bad = 0; });
  wg.phase([&](uint32_t t) {
    uint32_t bad = 0;
    for (uint32_t j = t; j < N; j += wg.lanes()) bad |= fr_ge_r_mask(fr_load_be(f32 + 32ull * j));
    if (bad) wg.raise(sh_bad);
  });
  wg.last([&](uint32_t t) {
    if (t == 0) *status = (int8_t)(*sh_bad & NBLS_ST_NON_CANONICAL);
    if (*sh_bad) fr_lane_zero16(f32, 2 * N, t, wg.lanes());
  });
}

// ---- The closing sums, one workgroup each; part: one element per lane.
// out32 = -(sum_i v[i]) mod r as 32 bytes big-endian, the lanes striding over the n items (kzg_sum_kernel; nbls_sim_kzg_sum)
template <class WG> NBLS_WG_FN void kzg_sum_body(WG wg, uint32_t n, const Fr* v, uint8_t* out32, Fr* part) {
  wg.phase([&](uint32_t t) {
    Fr acc = fr_zero();
    for (uint32_t i = t; i < n; i += wg.lanes()) acc = fr_add(acc, v[i]);
    part[t] = acc;
  });
  fr_tree(wg, part, 1);
  wg.last([&](uint32_t t) { if (t == 0) fr_store_be(fr_neg(part[0]), out32); });
}
// out32[i] = -(sum over the n_parts partial rows of column i) mod r, i < c = 2^log2_cell: lane group g on the rows g, g + groups, .. (kzg_cell_sum_kernel; the sum mode of
// nbls_sim_kzg_cell_interp)
template <class WG> NBLS_WG_FN void kzg_cell_sum_body(WG wg, unsigned log2_cell, uint32_t n_parts, const Fr* partial, uint8_t* out32, Fr* part) {
  const uint32_t c = 1u << log2_cell;
  wg.phase([&](uint32_t t) {
    Fr acc = fr_zero();
    for (uint32_t p = t >> log2_cell; p < n_parts; p += wg.lanes() >> log2_cell) acc = fr_add(acc, partial[(uint64_t)p * c + (t & (c - 1))]);
    part[t] = acc;
  });
  fr_tree(wg, part, c);
  wg.last([&](uint32_t t) { if (t < c) fr_store_q(fr_neg(part[t]), out32 + 32ull * t); });
}
// out32[c] = the sum over the n_parts partial rows (m + 1 elements each) of column c, for the columns c <= m of tile `tile`: row group g on the rows g, g + G16_GROUPS, ..
// (g16_sum_kernel; nbls_sim_g16_input_sums)
template <class WG> NBLS_WG_FN void g16_sum_body(WG wg, uint32_t m, uint32_t tile, uint32_t n_parts, const Fr* partial, uint8_t* out32, Fr* part) {
  wg.phase([&](uint32_t t) {
    const uint32_t c = tile * G16_TILE + (t & (G16_TILE - 1));
    Fr acc = fr_zero();
    if (c <= m) for (uint32_t p = t / G16_TILE; p < n_parts; p += G16_GROUPS) acc = fr_add(acc, partial[(uint64_t)p * (m + 1) + c]);
    part[t] = acc;
  });
  fr_tree(wg, part, G16_TILE);
  wg.last([&](uint32_t t) { const uint32_t c = tile * G16_TILE + t; if (t < G16_TILE && c <= m) fr_store_q(part[t], out32 + 32ull * c); });
}
}  // namespace nbls
