// g16p_exec.h -- the lane code of the Groth16 prover's scalar-field kernels (groth16_prove_kernels.hip; pipelines_groth16_prove.cpp has the chain), written once and compiled
// twice like fr_exec.h: into the device kernels and into the test-only simulator (nbls_sim_g16p_*: tests/test_groth16_prove_sim.py runs the same bodies against Python integers).
//   The statement.  An R1CS instance: three sparse matrices A, B, C of N = 2^log2_n rows (row j belongs to the domain point omega_N^j) and n_vars columns, in CSR form; the
//   assignment z = (1, x_1 .. x_m, aux ..).  a = A z, b = B z, c = C z are written as values in bit-reversed order -- position rev(j) holds row j, the order of nbls_fr_ntt --
//   and the instance is satisfied when z_0 = 1 and a_j b_j = c_j for every j.
//   The quotient.  The interpolants then satisfy a(X) b(X) - c(X) = h(X) Z(X), Z = X^N - 1.  On the coset 7 <omega_N> the divisor is the constant Z(7 w) = 7^N - 1 (any
//   shift g with g^N != 1 serves; 7 is bellman's), so
//     h = to_coeffs_7( (to_evals_7(to_coeffs(a)) * to_evals_7(to_coeffs(b)) - to_evals_7(to_coeffs(c))) / (7^N - 1) )
//   with the transforms of nbls_fr_ntt_dev and ONE pointwise kernel between them.  deg h <= N - 2: the top coefficient is zero.
// Forms: the elements of the three vectors and of h are plain, 32 bytes big-endian in memory (what the transforms and the MSM read); z is kept as plain limbs (Fr, no byte
// swap in the gathers); the matrix coefficients and the one constant are in Montgomery form, so every product comes out plain.  A row's sum is exact, so the order of its
// additions cannot change a bit: a row summed by one lane and a row summed by a wavefront give the same bytes.
#pragma once
#include "fr_exec.h"

namespace nbls {

enum { G16P_WAVE = 64 };                          // the lanes that share a long row
// entries from which a row is summed by a wavefront (NBLS_TUNE_G16P_ROW_WAVE = 0).  From instruction counts, not from a measurement (EXPERIMENTS.md): an entry costs one
// product (~130 v_mad_u64_u32 and their carries) and one addition, the cross-lane sum 6 levels of 8 shuffles and one addition, and the wavefront's 63 other lanes would
// otherwise carry 63 rows -- so the wavefront form pays only where a row would hold its 63 neighbours up for longer than they take themselves: rows several times the typical
// 1 - 4 entries.  32 leaves every ordinary row with a lane
enum { G16P_ROW_WAVE_DEFAULT = 32 };
enum { G16P_F_NONCANON = 0, G16P_F_UNSAT = 1, G16P_FLAGS = 16 };   // the bytes of a witness's flag block: raised by plain stores of 1 (every writer stores the same value)

// an Fr of a 32-byte aligned array of limbs
NBLS_FR_HD Fr g16p_load_limbs(const Fr* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 lo = ((const uint4*)p)[0], hi = ((const uint4*)p)[1];
  return Fr{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
#else
  return *p;
#endif
}
NBLS_FR_HD void g16p_store_limbs(const Fr& v, Fr* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  ((uint4*)p)[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  ((uint4*)p)[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
#else
  *p = v;
#endif
}

// ---- the witness: element i of w32 = z_0 .. z_(n_vars-1) | r | s (32 bytes big-endian each).  The canonical check of all of them, z to limb form, z_0 == 1
NBLS_FR_HD void g16p_witness_element(uint64_t n_vars, uint64_t i, const uint8_t* w32, Fr* z, uint8_t* flags) {
  const Fr v = fr_load_q(w32 + 32 * i);
  if (fr_ge_r_mask(v)) flags[G16P_F_NONCANON] = 1;
  if (i < n_vars) g16p_store_limbs(v, z + i);
  if (i == 0) {
    Fr d = v; d.l[0] ^= 1u;
    if (!fr_is_zero_mask(d)) flags[G16P_F_UNSAT] = 1;
  }
}

// ---- the matrix-vector products.  rows: N + 1 offsets (the rows past the last constraint are empty); cols < n_vars; vals in Montgomery form
struct G16pMatrix { const uint32_t* rows; const uint32_t* cols; const Fr* vals; };
// the share of lane `lane` of `lanes` in row `row`: the entries lane, lane + lanes, ..  (lanes = 1: the whole row)
NBLS_FR_HD Fr g16p_row_part(const G16pMatrix& M, const Fr* z, uint32_t row, uint32_t lane, uint32_t lanes) {
  Fr acc = fr_zero();
  for (uint32_t k = M.rows[row] + lane, e = M.rows[row + 1]; k < e; k += lanes) acc = fr_add(acc, fr_mul(g16p_load_limbs(z + M.cols[k]), g16p_load_limbs(M.vals + k)));
  return acc;
}
// all ones where a_j b_j != c_j (plain elements below r)
NBLS_FR_HD uint32_t g16p_violated_mask(const Fr& a, const Fr& b, const Fr& c) {
  return ~fr_is_zero_mask(fr_sub(fr_mul(a, fr_mul(b, fr_r2())), c));
}
// row `row` of the three products to position rev(row) of v32 = a | b | c (N elements each), and the flag
NBLS_FR_HD void g16p_row_store(unsigned log2_n, uint32_t row, const Fr& a, const Fr& b, const Fr& c, uint8_t* v32, uint8_t* flags) {
  const uint64_t pos = fr_bitrev(row, log2_n), N = (uint64_t)1 << log2_n;
  fr_store_q(a, v32 + 32 * pos);
  fr_store_q(b, v32 + 32 * (N + pos));
  fr_store_q(c, v32 + 32 * (2 * N + pos));
  if (g16p_violated_mask(a, b, c)) flags[G16P_F_UNSAT] = 1;
}

// ---- the quotient's pointwise step
// 1 / (7^N - 1), Montgomery form: log2_n squarings and one inversion, on the host, once per call
NBLS_FR_HD Fr g16p_quot_factor(unsigned log2_n) {
  Fr seven = fr_zero(); seven.l[0] = 7;
  Fr p = fr_mul(seven, fr_r2());
  for (unsigned i = 0; i < log2_n; i++) p = fr_sqr(p);
  return fr_inv(fr_sub(p, fr_one()));
}
// element idx of n rows of 2^log2_n elements: (a' b' - c') kinv takes a's place; zero where the first transform refused one of the row's three vectors (st3: its statuses,
// rows of a | of b | of c)
NBLS_FR_HD void g16p_quot_element(unsigned log2_n, uint64_t n, uint64_t idx, uint8_t* a32, const uint8_t* b32, const uint8_t* c32, const int8_t* st3, const Fr& kinv) {
  const uint64_t row = idx >> log2_n;
  const uint32_t bad = (uint32_t)0 - (uint32_t)((st3[row] | st3[n + row] | st3[2 * n + row]) != 0);
  const Fr a = fr_load_q(a32 + 32 * idx), b = fr_load_q(b32 + 32 * idx), c = fr_load_q(c32 + 32 * idx);
  fr_store_q(fr_select(bad, fr_zero(), fr_mul(fr_sub(fr_mul(a, fr_mul(b, fr_r2())), c), kinv)), a32 + 32 * idx);
}
// nbls_groth16_quotient's check of the caller's values, element idx: the row's byte is raised where a_j b_j != c_j (an element >= r raises what nobody reads: the row's
// status is then NBLS_ST_NON_CANONICAL)
NBLS_FR_HD void g16p_check_element(unsigned log2_n, uint64_t idx, const uint8_t* a32, const uint8_t* b32, const uint8_t* c32, uint8_t* violated) {
  if (g16p_violated_mask(fr_load_q(a32 + 32 * idx), fr_load_q(b32 + 32 * idx), fr_load_q(c32 + 32 * idx))) violated[idx >> log2_n] = 1;
}
// the status of row `row` of nbls_groth16_quotient: NBLS_ST_NON_CANONICAL (21), else NBLS_ST_G16_UNSATISFIED (24), else 0
NBLS_FR_HD int g16p_quot_status(uint64_t n, uint64_t row, const int8_t* st3, const uint8_t* violated) {
  return (st3[row] | st3[n + row] | st3[2 * n + row]) ? 21 : violated[row] ? 24 : 0;
}

// ---- the scalars of the four sums, 32 bytes big-endian each:
//   sa = z | 1 | r                      against a_query | alpha_g1 | delta_g1                  (n_vars + 2)
//   sb = z | 1 | s                      against b_query | beta | delta, in G1 and in G2        (n_vars + 2)
//   sc = z_aux | h_0 .. h_(N-2) | s | r | -r s   against l_query | h_query | A | B1 | delta_g1 (n_aux + N + 2)
// The scalar of a masked query point (mask byte 1: the key holds the zero point there) is zero, and every scalar of a witness whose flags are raised is zero: an element
// >= r is nothing the sums may read.  w32 as above; h32: the quotient's coefficients
struct G16pScalars {
  uint64_t n_vars, n_public, N;
  const uint8_t *w32, *h32, *mask_a, *mask_b, *mask_l, *flags;
  uint8_t *sa, *sb, *sc;
};
NBLS_FR_HD uint64_t g16p_scalar_count(uint64_t n_vars, uint64_t n_public, uint64_t N) { return 2 * (n_vars + 2) + (n_vars - n_public - 1) + N + 2; }
NBLS_FR_HD void g16p_scalar_element(const G16pScalars& S, uint64_t i) {
  const uint64_t nv = S.n_vars, na = nv - S.n_public - 1, row = nv + 2;
  const uint32_t dead = (uint32_t)0 - (uint32_t)((S.flags[G16P_F_NONCANON] | S.flags[G16P_F_UNSAT]) != 0);
  const uint8_t *r32 = S.w32 + 32 * nv, *s32 = r32 + 32;
  Fr one = fr_zero(); one.l[0] = 1;
  Fr v; uint8_t* out;
  if (i < 2 * row) {
    const bool second = i >= row;
    const uint64_t j = second ? i - row : i;
    out = (second ? S.sb : S.sa) + 32 * j;
    if (j < nv) v = (second ? S.mask_b : S.mask_a)[j] ? fr_zero() : fr_load_q(S.w32 + 32 * j);
    else v = j == nv ? one : fr_load_q(second ? s32 : r32);
  } else {
    const uint64_t j = i - 2 * row;
    out = S.sc + 32 * j;
    if (j < na) v = S.mask_l[j] ? fr_zero() : fr_load_q(S.w32 + 32 * (S.n_public + 1 + j));
    else if (j < na + S.N - 1) v = fr_load_q(S.h32 + 32 * (j - na));
    else if (j == na + S.N - 1) v = fr_load_q(s32);
    else if (j == na + S.N) v = fr_load_q(r32);
    else v = fr_neg(fr_mul(fr_load_q(r32), fr_mul(fr_load_q(s32), fr_r2())));
  }
  fr_store_q(fr_select(dead, fr_zero(), v), out);
}

}  // namespace nbls
