// fr_exec.h -- the scalar field Fr = Z / r (reference math.ts:295-386; r = CURVE.r, math.ts:15) and the Lagrange coefficients at zero of threshold recombination.  Written once
// and compiled twice like pow_exec.h / fp_inv.h / rlc_weights.h: into fr_kernels.hip (one element per lane) and into the test-only simulator (nbls_sim_fr_*: tests/test_fr_sim.py
// runs the same sequences against Python integers and the reference's own vectors).
//   Form: eight 32-bit limbs, little-endian, Montgomery with R = 2^256 (a 32 x 32 + 64 multiply-add per limb pair: v_mad_u64_u32 on the device).  r < 2^255, so 2r < R and every
//   product of an operand < R with an operand < r comes out of the reduction below 2r: one masked subtraction makes it canonical.  The 28-bit limbs of the base field (mac28 /
//   redc28, NL = 14) exist to keep fourteen-limb column sums inside 64 bits without carries; eight limbs need no such room, and ten 28-bit limbs would cost 100 products per
//   multiplication where eight 32-bit limbs cost 64.
//   Control flow is uniform: no branch depends on an operand.  Comparisons and selections are masks; INV is the fixed chain x^(r - 2) (Fermat; 0 -> 0); POW walks all 256 bits of
//   its per-item exponent and selects.  Nothing here is an interface for secrets all the same: no value is wiped.
#pragma once
#include <stdint.h>
#include "group_search.h"
#if defined(__HIPCC__)
#define NBLS_FR_HD __host__ __device__ inline
#else
#define NBLS_FR_HD inline
#endif

namespace nbls {

enum { FR_NL = 8 };
struct Fr { uint32_t l[FR_NL]; };
enum FrOp { FR_ADD = 0, FR_SUB = 1, FR_NEG = 2, FR_MUL = 3, FR_SQR = 4, FR_INV = 5, FR_DIV = 6, FR_POW = 7, FR_NOPS = 8 };

// the constants (tests/test_fr_sim.py checks every one against Python integers through nbls_sim_fr_consts): r, -r^-1 mod 2^32, R^2 mod r, R mod r, r - 2
NBLS_FR_HD uint32_t fr_mod(int i) {
  const uint32_t v[FR_NL] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
  return v[i];
}
NBLS_FR_HD uint32_t fr_n0() { return 0xffffffffu; }
NBLS_FR_HD Fr fr_r2() { return Fr{{0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u}}; }
NBLS_FR_HD Fr fr_one() { return Fr{{0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau, 0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u}}; }
NBLS_FR_HD uint32_t fr_rm2(int i) { return i == 0 ? 0xffffffffu : i == 1 ? 0xfffffffeu : fr_mod(i); }
NBLS_FR_HD Fr fr_zero() { return Fr{{0, 0, 0, 0, 0, 0, 0, 0}}; }

// all-ones when a == 0, when a == b
NBLS_FR_HD uint32_t fr_is_zero_mask(const Fr& a) {
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) acc |= a.l[i];
  return (uint32_t)((((uint64_t)acc) - 1) >> 32);
}
// m ? a : b for a mask m of all ones or all zeros
NBLS_FR_HD Fr fr_select(uint32_t m, const Fr& a, const Fr& b) {
  Fr o;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) o.l[i] = (a.l[i] & m) | (b.l[i] & ~m);
  return o;
}
// t - r where (carry : t) >= r, else t; carry = the ninth limb (0 or 1)
NBLS_FR_HD Fr fr_cond_sub(const Fr& t, uint32_t carry) {
  Fr d; uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    const uint64_t v = (uint64_t)t.l[i] - fr_mod(i) - bw;
    d.l[i] = (uint32_t)v; bw = (v >> 32) & 1;
  }
  const uint32_t keep = (uint32_t)0 - (uint32_t)(bw & ~(uint64_t)carry & 1);   // the subtraction borrowed and there was no ninth limb: t < r
  return fr_select(keep, t, d);
}
NBLS_FR_HD Fr fr_add(const Fr& a, const Fr& b) {   // a, b < r
  Fr t; uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) { c += (uint64_t)a.l[i] + b.l[i]; t.l[i] = (uint32_t)c; c >>= 32; }
  return fr_cond_sub(t, (uint32_t)c);
}
NBLS_FR_HD Fr fr_sub(const Fr& a, const Fr& b) {   // a, b < r
  Fr t; uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) { const uint64_t v = (uint64_t)a.l[i] - b.l[i] - bw; t.l[i] = (uint32_t)v; bw = (v >> 32) & 1; }
  const uint32_t m = (uint32_t)0 - (uint32_t)bw;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) { c += (uint64_t)t.l[i] + (fr_mod(i) & m); t.l[i] = (uint32_t)c; c >>= 32; }
  return t;
}
NBLS_FR_HD Fr fr_neg(const Fr& a) { return fr_sub(fr_zero(), a); }
// a b / R mod r, canonical, for a < R and b < r (either may be in Montgomery form or not): operand scanning, one reduction step per limb of b
NBLS_FR_HD Fr fr_mul(const Fr& a, const Fr& b) {
  uint32_t t[FR_NL + 2];
#pragma unroll
  for (int i = 0; i < FR_NL + 2; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < FR_NL; j++) { c += (uint64_t)a.l[j] * b.l[i] + t[j]; t[j] = (uint32_t)c; c >>= 32; }
    c += t[FR_NL]; t[FR_NL] = (uint32_t)c; t[FR_NL + 1] = (uint32_t)(c >> 32);
    const uint32_t m = t[0] * fr_n0();
    c = ((uint64_t)m * fr_mod(0) + t[0]) >> 32;
#pragma unroll
    for (int j = 1; j < FR_NL; j++) { c += (uint64_t)m * fr_mod(j) + t[j]; t[j - 1] = (uint32_t)c; c >>= 32; }
    c += t[FR_NL]; t[FR_NL - 1] = (uint32_t)c;
    t[FR_NL] = t[FR_NL + 1] + (uint32_t)(c >> 32);
  }
  Fr o;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) o.l[i] = t[i];
  return fr_cond_sub(o, t[FR_NL]);
}
NBLS_FR_HD Fr fr_sqr(const Fr& a) { return fr_mul(a, a); }
// 32 bytes big-endian <-> limbs; any 256-bit value -> its residue in Montgomery form (new Fr(v) reduces first, math.ts:301-303: v R^2 / R = v R below 2r, then canonical)
NBLS_FR_HD uint32_t fr_bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }
NBLS_FR_HD Fr fr_load_be(const uint8_t* in32) {
  Fr v;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    const uint8_t* p = in32 + 4 * (FR_NL - 1 - i);
    v.l[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
  }
  return v;
}
NBLS_FR_HD void fr_store_be(const Fr& v, uint8_t* out32) {
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    uint8_t* p = out32 + 4 * (FR_NL - 1 - i);
    p[0] = (uint8_t)(v.l[i] >> 24); p[1] = (uint8_t)(v.l[i] >> 16); p[2] = (uint8_t)(v.l[i] >> 8); p[3] = (uint8_t)v.l[i];
  }
}
NBLS_FR_HD Fr fr_from_bytes(const uint8_t* in32) { return fr_mul(fr_load_be(in32), fr_r2()); }
NBLS_FR_HD Fr fr_from_mont(const Fr& a) { Fr one = fr_zero(); one.l[0] = 1; return fr_mul(a, one); }
NBLS_FR_HD void fr_to_bytes(const Fr& a, uint8_t* out32) { fr_store_be(fr_from_mont(a), out32); }
// x^(r - 2): the exponent is public and the same for every lane, so its bits steer the chain (256 squarings, 127 products of a fixed pattern) -- no operand does.  0 -> 0.
// The words of the exponent are walked by an unrolled loop: every index is a constant, nothing is looked up at run time
NBLS_FR_HD Fr fr_inv(const Fr& x) {
  Fr acc = fr_one();
#pragma unroll
  for (int w = FR_NL - 1; w >= 0; w--) {
    const uint32_t e = fr_rm2(w);
    for (int b = 31; b >= 0; b--) {
      acc = fr_sqr(acc);
      if ((e >> b) & 1) acc = fr_mul(acc, x);
    }
  }
  return acc;
}
// x^e for a per-item exponent e (plain limbs, any 256-bit value; Fr.pow, math.ts:333-335, reads it as an integer): all 256 bits, product selected by a mask
NBLS_FR_HD Fr fr_pow(const Fr& x, const Fr& e) {
  Fr acc = fr_one();
#pragma unroll
  for (int w = FR_NL - 1; w >= 0; w--) {
    const uint32_t ew = e.l[w];
    for (int b = 31; b >= 0; b--) {
      acc = fr_sqr(acc);
      acc = fr_select((uint32_t)0 - ((ew >> b) & 1), fr_mul(acc, x), acc);
    }
  }
  return acc;
}
// one element of nbls_fr_op_batch: wire bytes in, wire bytes out; returns 5 where INV / DIV meets 0 mod r (the reference throws; the output is then all-zero), else 0
NBLS_FR_HD int fr_op_bytes(int op, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
  const Fr a = fr_from_bytes(a32);
  Fr o = a; uint32_t bad = 0;
  if (op == FR_NEG) o = fr_neg(a);
  else if (op == FR_SQR) o = fr_sqr(a);
  else if (op == FR_INV) { bad = fr_is_zero_mask(a); o = fr_inv(a); }
  else if (op == FR_POW) o = fr_pow(a, fr_load_be(b32));
  else {
    const Fr b = fr_from_bytes(b32);
    if (op == FR_ADD) o = fr_add(a, b);
    else if (op == FR_SUB) o = fr_sub(a, b);
    else if (op == FR_MUL) o = fr_mul(a, b);
    else { bad = fr_is_zero_mask(b); o = fr_mul(a, fr_inv(b)); }   // FR_DIV
  }
  fr_to_bytes(o, out32);
  return (int)(bad & 5);
}

// ---- Lagrange coefficients at zero.  Share k of a group with identifiers x_1 .. x_t (Montgomery form) gets
//   lambda_k = prod_{j != k} x_j / (x_j - x_k) = N / (x_k prod_{j != k} (x_j - x_k)),  N = prod_j x_j.
// A lane owns one share and folds the identifiers that pass by into its two running products: fr_lagrange_fold for identifier j of the lane's own group (mine = all ones) or of
// another group sharing the tile (mine = 0: both products keep their value -- a selection, not a branch).  fr_lagrange_finish: the coefficient, and all ones in *bad when the
// lane sees its group's identifiers are unusable -- x_k = 0, or d_k = 0: x_k equals another identifier mod r (Fr is a field: the product vanishes only with a factor).
struct FrLagrange { Fr xk, num, den; };
NBLS_FR_HD FrLagrange fr_lagrange_begin(const Fr& xk) { return FrLagrange{xk, fr_one(), xk}; }
NBLS_FR_HD void fr_lagrange_fold(FrLagrange& s, const Fr& xj, uint32_t mine, uint32_t self) {
  const Fr one = fr_one();
  s.num = fr_mul(s.num, fr_select(mine, xj, one));
  s.den = fr_mul(s.den, fr_select(mine & ~self, fr_sub(xj, s.xk), one));
}
// the group of share k: off[g] <= k < off[g + 1] over ngroups + 1 strictly increasing offsets
NBLS_FR_HD uint32_t fr_group_of(const uint32_t* off, uint32_t ngroups, uint32_t k) { return group_search(off, 0, ngroups, k); }
// one staged tile: identifiers t .. t + cnt - 1 of the call, for the lane of share k whose group is [gb, ge)
NBLS_FR_HD void fr_lagrange_tile(FrLagrange& s, const Fr* tile, uint32_t t, uint32_t cnt, uint32_t gb, uint32_t ge, uint32_t k) {
  for (uint32_t c = 0; c < cnt; c++) {
    const uint32_t j = t + c;
    fr_lagrange_fold(s, tile[c], (uint32_t)0 - (uint32_t)(j >= gb && j < ge), (uint32_t)0 - (uint32_t)(j == k));
  }
}
NBLS_FR_HD Fr fr_lagrange_finish(const FrLagrange& s, uint32_t* bad) {
  *bad = fr_is_zero_mask(s.den);
  return fr_mul(s.num, fr_inv(s.den));
}

// ---- Polynomials in evaluation form over the N = 2^k roots of unity, k = 1 .. 12 (evaluate_polynomial_in_evaluation_form of EIP-4844; kzg_kernels.hip and nbls_sim_fr_eval_roots):
//   p(z) = (z^N - 1) / N * sum_j f_j w_j / (z - w_j),   w_j = omega^rev(j),  omega = 7^((r - 1) / N),  rev = the k-bit reversal;   p(w_j) = f_j.
// A workgroup of `lanes` lanes owns one polynomial; lane t owns the terms j = t, t + lanes, .. (ceil(N / lanes) of them).  fr_eval_lane inverts the lane's denominators
// with ONE fr_inv (Montgomery's trick: the running products wait in the workgroup's shared memory); a vanishing
// denominator is replaced by one under a mask and its index remembered; terms past N (N < lanes) are masked the same way.  The lane sums meet in a tree of fr_add -- exact, so
// the order of the additions cannot change a bit -- and fr_eval_finish closes: the factor (z^N - 1) / N, the element f_j itself where z = w_j, zero where an input was >= r.
// Values: the table and z are in Montgomery form; the elements f_j stay plain (a product plain x Montgomery is plain), so sums and results need no conversion.
NBLS_FR_HD uint32_t fr_ge_r_mask(const Fr& a) {   // all ones when the plain 256-bit value a is >= r: bytes_to_bls_field refuses it
  uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) bw = (((uint64_t)a.l[i] - fr_mod(i) - bw) >> 32) & 1;
  return (uint32_t)bw - 1;
}
NBLS_FR_HD Fr fr_rm1_shr(unsigned k) {   // (r - 1) >> k as plain limbs, 0 <= k < 32 (2^32 divides r - 1)
  Fr e;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    const uint32_t lo = i == 0 ? 0u : fr_mod(i), hi = i + 1 < FR_NL ? fr_mod(i + 1) : 0u;
    e.l[i] = k ? (lo >> k) | (hi << (32 - k)) : lo;
  }
  return e;
}
NBLS_FR_HD uint32_t fr_bitrev(uint32_t j, unsigned bits) {
  uint32_t o = 0;
  for (unsigned b = 0; b < bits; b++) o |= ((j >> b) & 1) << (bits - 1 - b);
  return o;
}
NBLS_FR_HD Fr fr_omega(unsigned log2_n) { Fr seven = fr_zero(); seven.l[0] = 7; return fr_pow(fr_mul(seven, fr_r2()), fr_rm1_shr(log2_n)); }
// entry j of the table of 2^log2_n roots in bit-reversed order, Montgomery form (the exponent has at most 12 bits; all of them are walked)
NBLS_FR_HD Fr fr_root_entry(const Fr& omega, unsigned log2_n, uint32_t j) {
  const uint32_t e = fr_bitrev(j, log2_n);
  Fr acc = fr_one();
  for (int b = 11; b >= 0; b--) {
    acc = fr_sqr(acc);
    acc = fr_select((uint32_t)0 - ((e >> b) & 1), fr_mul(acc, omega), acc);
  }
  return acc;
}
NBLS_FR_HD Fr fr_inv_pow2(unsigned log2_n) {   // 1 / 2^log2_n = r - (r - 1) / 2^log2_n, Montgomery form
  return fr_mul(fr_sub(fr_zero(), fr_rm1_shr(log2_n)), fr_r2());
}
struct FrEvalPart { Fr sum; uint32_t hit, bad; };   // the lane's plain partial sum | the index j with z = w_j, else 0xffffffff | all ones when an element the lane read is >= r
// pre: the products in front of each of the lane's denominators, terms x 8 x lanes words laid out [term][limb][lane] (LDS on the device: consecutive lanes on consecutive banks);
// held in registers, sixteen terms of unrolled code let the compiler hoist every load of the walk and spill (measured on gfx950: 256 VGPRs and 1252 bytes of private memory)
// KEEP (the quotient, below): the backward walk leaves 1 / (z - w_j), Montgomery form, in the slot the product in front of term j came from -- the same lane's own slot, read
// just before it is written.  The slot of a masked term (z = w_j, or j >= N) then holds a value nobody may use
template <bool KEEP>
NBLS_FR_HD FrEvalPart fr_eval_lane_t(const uint8_t* f32, const Fr* roots, const Fr& z, uint32_t N, uint32_t lane, uint32_t lanes, uint32_t* pre) {
  const uint32_t terms = (N + lanes - 1) / lanes;   // the workgroup's bound, the same for every lane
  const Fr one = fr_one();
  Fr acc = one;
  FrEvalPart o{fr_zero(), 0xffffffffu, 0};
  for (uint32_t k = 0; k < terms; k++) {
    const uint32_t j = lane + k * lanes, live = (uint32_t)0 - (uint32_t)(j < N), jj = j < N ? j : N - 1;
    const Fr d = fr_sub(z, roots[jj]);
    const uint32_t zm = fr_is_zero_mask(d) & live;
    o.hit = (o.hit & ~zm) | (j & zm);
#pragma unroll
    for (int i = 0; i < FR_NL; i++) pre[(k * FR_NL + i) * lanes + lane] = acc.l[i];
    acc = fr_mul(acc, fr_select(zm | ~live, one, d));
  }
  Fr inv = fr_inv(acc);
  for (uint32_t k = terms; k-- > 0;) {
    const uint32_t j = lane + k * lanes, live = (uint32_t)0 - (uint32_t)(j < N), jj = j < N ? j : N - 1;
    const Fr w = roots[jj], d0 = fr_sub(z, w);
    const Fr d = fr_select((fr_is_zero_mask(d0) & live) | ~live, one, d0);
    const Fr f = fr_load_be(f32 + 32ull * jj);
    o.bad |= fr_ge_r_mask(f) & live;
    Fr p;
#pragma unroll
    for (int i = 0; i < FR_NL; i++) p.l[i] = pre[(k * FR_NL + i) * lanes + lane];
    Fr t;                                                // f_j w_j / (z - w_j), plain
    if (KEEP) {
      const Fr id = fr_mul(inv, p);                      // 1 / (z - w_j), Montgomery form
#pragma unroll
      for (int i = 0; i < FR_NL; i++) pre[(k * FR_NL + i) * lanes + lane] = id.l[i];
      t = fr_mul(fr_mul(f, w), id);
    } else t = fr_mul(fr_mul(f, w), fr_mul(inv, p));
    inv = fr_mul(inv, d);
    o.sum = fr_add(o.sum, fr_select(live, t, fr_zero()));
  }
  return o;
}
NBLS_FR_HD FrEvalPart fr_eval_lane(const uint8_t* f32, const Fr* roots, const Fr& z, uint32_t N, uint32_t lane, uint32_t lanes, uint32_t* pre) {
  return fr_eval_lane_t<false>(f32, roots, z, N, lane, lanes, pre);
}
// the value alone: the factor (z^N - 1) / N on the workgroup's plain sum, or the element f_hit itself
NBLS_FR_HD Fr fr_eval_value(const Fr& sum, uint32_t hit, const Fr& z, unsigned log2_n, const uint8_t* f32) {
  Fr zn = z;
  for (unsigned i = 0; i < log2_n; i++) zn = fr_sqr(zn);
  const Fr fac = fr_mul(fr_sub(zn, fr_one()), fr_inv_pow2(log2_n));
  const uint32_t hm = (uint32_t)0 - (uint32_t)(hit != 0xffffffffu);
  return fr_select(hm, fr_load_be(f32 + 32ull * (hit & hm)), fr_mul(sum, fac));
}
// sum: the workgroup's plain sum; hit / bad: the lanes' combined (bad also where z itself was >= r) -> 32 bytes big-endian; returns the status (21 = NBLS_ST_NON_CANONICAL, else 0)
NBLS_FR_HD int fr_eval_finish(const Fr& sum, uint32_t hit, uint32_t bad, const Fr& z, unsigned log2_n, const uint8_t* f32, uint8_t* out32) {
  fr_store_be(fr_select(bad, fr_zero(), fr_eval_value(sum, hit, z, log2_n, f32)), out32);
  return (int)(bad & 21);
}
enum { FR_EVAL_LANES = 256 };   // lanes per polynomial: 16 terms each at N = 4096

// ---- The quotient of an opening in evaluation form (compute_kzg_proof_impl of EIP-4844; kzg_quotient_kernel and nbls_sim_fr_quotient_roots): with y = p(z),
//   q_j = (f_j - y) / (w_j - z)  where w_j != z,     q_m = sum_{j != m} (f_j - y) w_j / (z (z - w_j)) = -1 / z * sum_{j != m} q_j w_j  where z = w_m
// (compute_quotient_eval_within_domain; z = w_m is a root of unity, so it is not zero).  The lanes are fr_eval_lane's, run with KEEP: after that walk the slots of `pre` hold
// 1 / (z - w_j) in Montgomery form.  y and the elements are plain, so q_j = (y - f_j) * 1 / (z - w_j) is plain: it goes out as 32 bytes big-endian, the form the MSM reads.
// fr_quot_lane: the lane's terms -> out_q32 (N x 32 bytes; all-zero where `bad`; zero at the term `hit`, which fr_quot_within fills); returns the lane's plain share of
// sum_{j != hit} q_j w_j (zero when there is no hit: the products are then not formed -- hit is the workgroup's, the branch is uniform)
NBLS_FR_HD void fr_store_q(const Fr& v, uint8_t* out32) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* o = (uint4*)out32;   // (16-byte aligned: a row of a staged or carved block)
  o[0] = make_uint4(fr_bswap32(v.l[7]), fr_bswap32(v.l[6]), fr_bswap32(v.l[5]), fr_bswap32(v.l[4]));
  o[1] = make_uint4(fr_bswap32(v.l[3]), fr_bswap32(v.l[2]), fr_bswap32(v.l[1]), fr_bswap32(v.l[0]));
#else
  fr_store_be(v, out32);
#endif
}
NBLS_FR_HD Fr fr_quot_lane(const uint8_t* f32, const Fr* roots, const Fr& y, uint32_t hit, uint32_t bad, uint32_t N, uint32_t lane, uint32_t lanes, const uint32_t* pre, uint8_t* out_q32) {
  const uint32_t terms = (N + lanes - 1) / lanes;
  const Fr zero = fr_zero();
  Fr acc = zero;
  for (uint32_t k = 0; k < terms; k++) {
    const uint32_t j = lane + k * lanes;
    if (j >= N) break;   // (the lane's last term: nothing of the workgroup is left behind it)
    Fr id;
#pragma unroll
    for (int i = 0; i < FR_NL; i++) id.l[i] = pre[(k * FR_NL + i) * lanes + lane];
    const uint32_t out = bad | ((uint32_t)0 - (uint32_t)(j == hit));
    const Fr q = fr_select(out, zero, fr_mul(fr_sub(y, fr_load_be(f32 + 32ull * j)), id));
    fr_store_q(q, out_q32 + 32ull * j);
    if (hit != 0xffffffffu) acc = fr_add(acc, fr_mul(q, roots[j]));
  }
  return acc;
}
// q_m from the workgroup's sum (plain) and z = w_m (Montgomery form): one inversion, on the lane that owns m
NBLS_FR_HD Fr fr_quot_within(const Fr& sum, const Fr& z) { return fr_neg(fr_mul(sum, fr_inv(z))); }

// ---- The transform between the two forms of a polynomial of N = 2^k coefficients, k = 1 .. 12 (kzg_ntt_kernel and nbls_sim_fr_ntt; the cells of EIP-7594 are built on it):
//   coefficients c_0 .. c_{N-1}, natural order   <->   values v_j = p(s w_j) in the bit-reversed order of the table above, for a shift s != 0 (1: the roots themselves).
// A workgroup of `lanes` lanes owns one polynomial, resident in shared memory as `a`, 8 N words laid out [limb][index]: a wavefront that walks consecutive indices reads
// consecutive banks.  The network needs no permutation pass: X^(2 len) - zeta^2 splits into X^len - zeta and X^len + zeta, so block b of a stage with half-length len reduces
//   lo' = lo + zeta hi,   hi' = lo - zeta hi,   zeta = table[2 b]
// (the entry of omega^rev(2 b): the same for every butterfly of the block), from len = N / 2 down to 1 -- natural order in, bit-reversed out.  The way back undoes the stages in
// reverse order, lo = lo' + hi', hi = (lo' - hi') / zeta with the table of the inverse roots (fr_inv_root_index), and leaves every coefficient times N.  The block of
// the stage with len = N / 2 has zeta = 1: its product is not formed (the stage's, not the operand's, property).  Elements stay plain throughout (plain x Montgomery is plain);
// the tables, the shift's powers and 1 / N are in Montgomery form.  A stage is fr_ntt_stage on every lane, then a barrier; lane t owns the butterflies t, t + lanes, ..
// Lanes per polynomial: 512 = eight wavefronts, two on every SIMD of the compute unit the polynomial occupies (at N = 4096 its LDS admits one workgroup), four butterflies per
// lane and stage at N = 4096.  The kernel needs 152 VGPRs: a workgroup of 1024 lanes is held to 128 and spills (measured: 64 bytes of private memory per lane)
#ifndef NBLS_NTT_LOG2_LANES
#define NBLS_NTT_LOG2_LANES 9
#endif
enum { FR_NTT_LOG2_LANES = NBLS_NTT_LOG2_LANES, FR_NTT_LANES = 1 << FR_NTT_LOG2_LANES };
// the table of the inverse roots is a permutation of the table of roots: (1 / omega)^rev(j) = omega^(N - rev(j)) = entry rev(N - rev(j) mod N)
NBLS_FR_HD uint32_t fr_inv_root_index(unsigned log2_n, uint32_t j) { return fr_bitrev(((1u << log2_n) - fr_bitrev(j, log2_n)) & ((1u << log2_n) - 1), log2_n); }
enum FrNttMode { FR_NTT_TO_COEFFS = 0, FR_NTT_TO_EVALS = 1, FR_NTT_CELLS = 2 };   // (2: compute_cells' chain -- to coefficients, times g^i / N, to values on the coset)
NBLS_FR_HD Fr fr_load_q(const uint8_t* in32) {   // fr_store_q's way back
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 hi = ((const uint4*)in32)[0], lo = ((const uint4*)in32)[1];   // (16-byte aligned: a row of a staged or carved block)
  return Fr{{fr_bswap32(lo.w), fr_bswap32(lo.z), fr_bswap32(lo.y), fr_bswap32(lo.x), fr_bswap32(hi.w), fr_bswap32(hi.z), fr_bswap32(hi.y), fr_bswap32(hi.x)}};
#else
  return fr_load_be(in32);
#endif
}
NBLS_FR_HD Fr fr_ntt_get(const uint32_t* a, uint32_t N, uint32_t i) {
  Fr v;
#pragma unroll
  for (int l = 0; l < FR_NL; l++) v.l[l] = a[l * N + i];
  return v;
}
NBLS_FR_HD void fr_ntt_put(uint32_t* a, uint32_t N, uint32_t i, const Fr& v) {
#pragma unroll
  for (int l = 0; l < FR_NL; l++) a[l * N + i] = v.l[l];
}
// x^e for an index e of at most `bits` bits: all of them are walked
NBLS_FR_HD Fr fr_pow_index(const Fr& x, uint32_t e, unsigned bits) {
  Fr acc = fr_one();
  for (int b = (int)bits - 1; b >= 0; b--) {
    acc = fr_sqr(acc);
    acc = fr_select((uint32_t)0 - ((e >> b) & 1), fr_mul(acc, x), acc);
  }
  return acc;
}
// the lane's elements t, t + lanes, .. of a polynomial into `a`; returns all ones when one of them is >= r
NBLS_FR_HD uint32_t fr_ntt_load(const uint8_t* in32, uint32_t N, uint32_t lane, uint32_t lanes, uint32_t* a) {
  uint32_t bad = 0;
  for (uint32_t i = lane; i < N; i += lanes) {
    const Fr v = fr_load_q(in32 + 32ull * i);
    bad |= fr_ge_r_mask(v);
    fr_ntt_put(a, N, i, v);
  }
  return bad;
}
// the shift of a polynomial, read by one lane: -> s (Montgomery form; 1 / s where `invert`: the one inversion of the way back), *bad = all ones when it is >= r, *zero when
// it is 0 mod r (which is then also what the inversion returns: nobody uses it)
NBLS_FR_HD Fr fr_ntt_shift(const uint8_t* shift32, bool invert, uint32_t* bad, uint32_t* zero) {
  const Fr raw = fr_load_be(shift32), s = fr_mul(raw, fr_r2());
  *bad = fr_ge_r_mask(raw); *zero = fr_is_zero_mask(s);
  return invert ? fr_inv(s) : s;
}
// the lane's elements of `a` times f (NULL: 1) and, element i, times s^i (NULL: s = 1): the lane starts at s^lane and steps by s^lanes.  coef_out (may be NULL): the
// elements after the factor f and before the powers, as 32 bytes big-endian -- the coefficients that the cell proofs read
NBLS_FR_HD void fr_ntt_scale(uint32_t* a, uint32_t N, uint32_t lane, uint32_t lanes, unsigned log2_lanes, const Fr* f, const Fr* s, uint8_t* coef_out) {
  Fr pw = fr_one(), step = pw;
  if (s) {
    pw = fr_pow_index(*s, lane, log2_lanes);
    step = *s;
    for (unsigned b = 0; b < log2_lanes; b++) step = fr_sqr(step);
  }
  for (uint32_t i = lane; i < N; i += lanes) {
    Fr v = fr_ntt_get(a, N, i);
    if (f) v = fr_mul(v, *f);
    if (coef_out) fr_store_q(v, coef_out + 32ull * i);
    if (s) { v = fr_mul(v, pw); pw = fr_mul(pw, step); }
    fr_ntt_put(a, N, i, v);
  }
}
// one stage for one lane: half-length 2^log2_len; table = the roots (towards the values) or the inverse roots (`inverse`: towards the coefficients)
NBLS_FR_HD void fr_ntt_stage(uint32_t* a, unsigned log2_n, unsigned log2_len, bool inverse, const Fr* table, uint32_t lane, uint32_t lanes) {
  const uint32_t N = 1u << log2_n, len = 1u << log2_len;
  const bool unit = log2_len + 1 == log2_n;   // the one block of the stage has zeta = 1
  for (uint32_t b = lane; b < N / 2; b += lanes) {
    const uint32_t blk = b >> log2_len, lo = (blk << (log2_len + 1)) | (b & (len - 1)), hi = lo + len;
    const Fr u = fr_ntt_get(a, N, lo), v = fr_ntt_get(a, N, hi);
    if (inverse) {
      const Fr d = fr_sub(u, v);
      fr_ntt_put(a, N, lo, fr_add(u, v));
      fr_ntt_put(a, N, hi, unit ? d : fr_mul(d, table[2 * blk]));
    } else {
      const Fr t = unit ? v : fr_mul(v, table[2 * blk]);
      fr_ntt_put(a, N, lo, fr_add(u, t));
      fr_ntt_put(a, N, hi, fr_sub(u, t));
    }
  }
}
// the lane's elements of `a` as 32 bytes big-endian each
NBLS_FR_HD void fr_ntt_store(const uint32_t* a, uint32_t N, uint32_t lane, uint32_t lanes, uint8_t* out32) {
  for (uint32_t i = lane; i < N; i += lanes) fr_store_q(fr_ntt_get(a, N, i), out32 + 32ull * i);
}

// ---- Transforms of more elements than one workgroup holds: N = 2^L, L <= 24 (nbls_fr_ntt_large / nbls_fr_ntt_dev; kzg_ntt_pass_kernel, kzg_ntt_tail_kernel and
// nbls_sim_fr_ntt_large).  With T_N[j] = omega_N^rev_L(j) the table above, t the tail's log size and K = L - t <= 12, the network above splits into
//   K global stages j = 0 .. K - 1 (half-length N / 2^(j+1), block b with zeta = T_N[2 b], 2 b < 2^K: T_N[j] = T_(2^K)[j] for j < 2^K, so the table of 2^K roots serves
//     and no table of N roots exists), cut into runs of at most P consecutive stages, one launch per run;
//   2^K tails: after K stages block B (2^t contiguous elements) holds p mod (X^(2^t) - T_N[B]), and its values are those of that remainder on s_B w_j, w_j the table of
//     2^t roots, s_B = omega_N^rev_K(B) (s_B^(2^t) = T_N[B]): the transform above on the block with the shift s_B.
// A run j0 .. j0 + q - 1 is independent per (hi, lo) of index = hi 2^(L - j0) + row 2^(L - j0 - q) + lo: a network over the q bits of `row`, whose stage j0 + k has the
// block number (hi << k) | (the top k bits of row).  A workgroup takes one hi and 2^c consecutive lo -- a tile of 2^q rows of 2^c contiguous elements, element i of the
// tile at row i >> c, column i & (2^c - 1), in `a` laid out [limb][i] as above -- and runs the q stages as the stages of a transform of 2^(q + c) elements whose table
// starts at entry 2 (hi << k).  c <= the log of the lanes: a lane's elements t, t + lanes, .. then share their column, and their indices step by a fixed amount.
// The way back: the tails towards the coefficients with 1 / s_B, then the runs in reverse order with the inverse roots of size 2^K, then 1 / N in the run that has stage 0.
struct FrNttRun { uint32_t log2_n, j0, q, c; };
#if defined(__HIPCC__)
#define NBLS_FR_RUN_HD __host__ __device__ __forceinline__   // (forced: a run or a factor passed by address to a function the compiler declines to inline costs the kernel a stack)
#else
#define NBLS_FR_RUN_HD inline
#endif
enum { FR_NTTL_MAX_LOG2 = 24, FR_NTTL_MAX_TAIL = 12, FR_NTTL_MAX_PASS = 9, FR_NTTL_MAX_TILE = 12 };   // (9 stages of rows of 8 elements fill the tile of 2^12)
enum { FR_NTTL_DEFAULT_TAIL = 12, FR_NTTL_DEFAULT_PASS = 8 };   // t and P where the caller sets none (the sweep behind P: EXPERIMENTS.md)
enum { FR_NTTL_BAD = 1, FR_NTTL_ZERO = 2 };   // the bits of a polynomial's flag word: an element or the shift is >= r | the shift is 0 mod r
// the plan: K stages in ceil(K / P) runs whose lengths differ by one at most, the longer ones first; run i of them -> its first stage and its length
NBLS_FR_HD uint32_t fr_nttl_runs(uint32_t K, uint32_t P) { return (K + P - 1) / P; }
NBLS_FR_HD FrNttRun fr_nttl_run(uint32_t log2_n, uint32_t K, uint32_t P, uint32_t i) {
  const uint32_t runs = fr_nttl_runs(K, P), base = K / runs, more = K % runs;
  FrNttRun R;
  R.log2_n = log2_n; R.j0 = i * base + (i < more ? i : more); R.q = base + (i < more ? 1u : 0u);
  const uint32_t rest = log2_n - R.j0 - R.q, room = FR_NTTL_MAX_TILE - R.q;
  R.c = rest < room ? rest : room;
  if (R.c > FR_NTT_LOG2_LANES) R.c = FR_NTT_LOG2_LANES;
  return R;
}
// element i of the tile (hi, lo0) -> its index in the polynomial
NBLS_FR_RUN_HD uint32_t fr_run_index(const FrNttRun& R, uint32_t hi, uint32_t lo0, uint32_t i) {
  return (hi << (R.log2_n - R.j0)) + ((i >> R.c) << (R.log2_n - R.j0 - R.q)) + lo0 + (i & ((1u << R.c) - 1));
}
// the lane's elements of the tile into `a`; returns all ones when one of them is >= r
NBLS_FR_RUN_HD uint32_t fr_run_load(const FrNttRun& R, const uint8_t* in32, uint32_t hi, uint32_t lo0, uint32_t lane, uint32_t lanes, uint32_t* a) {
  const uint32_t T = 1u << (R.q + R.c);
  uint32_t bad = 0;
  for (uint32_t i = lane; i < T; i += lanes) {
    const Fr v = fr_load_q(in32 + 32ull * fr_run_index(R, hi, lo0, i));
    bad |= fr_ge_r_mask(v);
    fr_ntt_put(a, T, i, v);
  }
  return bad;
}
// the lane's elements of a tile of the run that has stage 0 (hi = 0) times f (NULL: 1) and, the element of index g in the polynomial, times s^g (NULL: s = 1): one power
// per lane, then steps of s^((lanes >> c) 2^(L - q)), the distance of the lane's consecutive elements
NBLS_FR_RUN_HD void fr_run_scale(uint32_t* a, const FrNttRun& R, uint32_t lo0, uint32_t lane, uint32_t lanes, unsigned log2_lanes, const Fr* f, const Fr* s) {
  const uint32_t T = 1u << (R.q + R.c);
  Fr pw = fr_one(), step = pw;
  if (s) {
    pw = fr_pow_index(*s, fr_run_index(R, 0, lo0, lane) & ((1u << R.log2_n) - 1), R.log2_n);
    step = *s;
    for (unsigned b = 0; b < log2_lanes - R.c + R.log2_n - R.q; b++) step = fr_sqr(step);
  }
  for (uint32_t i = lane; i < T; i += lanes) {
    Fr v = fr_ntt_get(a, T, i);
    if (f) v = fr_mul(v, *f);
    if (s) { v = fr_mul(v, pw); pw = fr_mul(pw, step); }
    fr_ntt_put(a, T, i, v);
  }
}
// fr_ntt_stage on a tile of 2^log2_tile elements: half-length 2^log2_len; table = entry 2 (hi << k) of the roots (or of the inverse roots) of size 2^K on; unit: the stage
// is stage 0 of the transform, whose one block has zeta = 1
NBLS_FR_RUN_HD void fr_run_stage(uint32_t* a, unsigned log2_tile, unsigned log2_len, bool inverse, bool unit, const Fr* table, uint32_t lane, uint32_t lanes) {
  const uint32_t T = 1u << log2_tile, len = 1u << log2_len;
  for (uint32_t b = lane; b < T / 2; b += lanes) {
    const uint32_t blk = b >> log2_len, lo = (blk << (log2_len + 1)) | (b & (len - 1)), hi = lo + len;
    const Fr u = fr_ntt_get(a, T, lo), v = fr_ntt_get(a, T, hi);
    if (inverse) {
      const Fr d = fr_sub(u, v);
      fr_ntt_put(a, T, lo, fr_add(u, v));
      fr_ntt_put(a, T, hi, unit ? d : fr_mul(d, table[2 * blk]));
    } else {
      const Fr t = unit ? v : fr_mul(v, table[2 * blk]);
      fr_ntt_put(a, T, lo, fr_add(u, t));
      fr_ntt_put(a, T, hi, fr_sub(u, t));
    }
  }
}
// the lane's elements of the tile back to the polynomial (zero: as all-zero bytes)
NBLS_FR_RUN_HD void fr_run_store(const FrNttRun& R, const uint32_t* a, bool zero, uint32_t hi, uint32_t lo0, uint32_t lane, uint32_t lanes, uint8_t* out32) {
  const uint32_t T = 1u << (R.q + R.c);
  for (uint32_t i = lane; i < T; i += lanes) fr_store_q(zero ? fr_zero() : fr_ntt_get(a, T, i), out32 + 32ull * fr_run_index(R, hi, lo0, i));
}

// ---- The quotient rows of the cell proofs (compute_cells_and_kzg_proofs of EIP-7594; kzg_cell_rows_kernel and nbls_sim_kzg_cell_rows).  Cell k of a polynomial p of N
// coefficients holds its values on the coset h_k <omega_c>, whose vanishing polynomial is X^c - s_k, s_k = h_k^c = entry k of the table of the 2 N / c roots of unity.  The
// proof's quotient is the floor quotient of p by it in coefficient form:  q_i = 0 for i >= N - c,  q_i = p_(i + c) + s_k q_(i + c)  downwards -- c independent chains of N / c
// steps.  A lane walks chain j of one row (i = j mod c) and writes it as big-endian scalars, the form the MSM reads; coefficients plain, s in Montgomery form
NBLS_FR_HD void fr_cell_chain(const uint8_t* coef32, unsigned log2_n, unsigned log2_cell, uint32_t j, const Fr& s, uint8_t* row32) {
  const uint32_t N = 1u << log2_n, c = 1u << log2_cell;
  Fr q = fr_zero();
  for (uint32_t i = N - c + j;; i -= c) {
    fr_store_q(q, row32 + 32ull * i);
    if (i < c) break;
    q = fr_add(fr_load_q(coef32 + 32ull * i), fr_mul(q, s));   // q_(i - c)
  }
}

// ---- All cell proofs of a blob together (FK20, Feist-Khovratovich; kzg_fk20_*_kernel and nbls_sim_kzg_fk20_*).  N coefficients p_i, c per cell, n' = N / c, M = 2 n' cells,
// w_i = omega_M^rev(i) = entry i of the table of the M roots (the order of every array below: position i stands for the exponent v = rev(i), which is what the network
// above leaves from natural input, so no permutation pass exists):
//   a^[j][i] = sum_{t < n'} p_(j + c t) w_i^t                              the per-blob scalars: the size-M transform of stripe j of the coefficients, zero-padded
//   X^[j][i] = sum_{t <= n' - 2} [w_i^t] [tau^(j + c (n' - 2 - t))]G1      the handle's fixed points
//   y^_i = sum_{j < c} [a^[j][i]] X^[j][i]                                 pass A;   h_u = IDFT_M(y^)_(n' - 1 + u), u <= n' - 2 (the cyclic convolution does not wrap)
//   proof_k = sum_u [s_k^u] h_u = sum_i [B[k][i]] y^_i,  B[k][i] = 1 / M * sum_{u <= n' - 2} s_k^u w_i^(-(n' - 1 + u))      pass B
// The scalars kernel: a workgroup of FR_FK_LANES lanes holds `stripes` transforms side by side in shared memory, stripe `sub` of the workgroup at a[(limb M + index) stripes +
// sub] -- thread t = lane * stripes + sub, so consecutive threads touch consecutive words of LDS and consecutive stripes j of the output.  M / 2 < FR_FK_LANES: one butterfly
// per lane and stage, 2 FR_FK_LANES / M stripes a workgroup; from M / 2 = FR_FK_LANES on one stripe a workgroup, M / (2 FR_FK_LANES) butterflies per lane.  Elements stay plain
enum { FR_FK_LANES = 256 };
struct FrFkLane { uint32_t sub, lane, lanes, stripes, blob, j, live; };   // live = 0: a stripe past the call's last (it loads zeros, meets every barrier and stores nothing)
NBLS_FR_HD FrFkLane fr_fk_lane(unsigned log2_m, unsigned log2_cell, uint32_t n_blobs, uint32_t wg, uint32_t t) {
  const uint32_t half = 1u << (log2_m - 1), lanes = half < FR_FK_LANES ? half : (uint32_t)FR_FK_LANES, stripes = FR_FK_LANES / lanes;
  const uint32_t sub = t % stripes;
  const uint64_t S = (uint64_t)wg * stripes + sub;
  const uint32_t live = S < ((uint64_t)n_blobs << log2_cell) ? 1u : 0u;
  return FrFkLane{sub, t / stripes, lanes, stripes, (uint32_t)(S >> log2_cell), (uint32_t)S & ((1u << log2_cell) - 1), live};
}
NBLS_FR_HD uint32_t fr_fk_workgroups(unsigned log2_m, unsigned log2_cell, uint32_t n_blobs) {
  const uint32_t half = 1u << (log2_m - 1), stripes = half < FR_FK_LANES ? FR_FK_LANES / half : 1u;
  return (uint32_t)((((uint64_t)n_blobs << log2_cell) + stripes - 1) / stripes);
}
NBLS_FR_HD uint32_t fr_fk_lds_words(unsigned log2_m) { const uint32_t M = 1u << log2_m; return FR_NL * (M < 2 * FR_FK_LANES ? 2 * FR_FK_LANES : M); }
// the lane's elements of its stripe: index t < n' is p_(j + c t), the upper half zero.  coef32: the call's n x N coefficients
NBLS_FR_HD void fr_fk_load(const uint8_t* coef32, unsigned log2_n, unsigned log2_cell, unsigned log2_m, const FrFkLane& L, uint32_t* a) {
  const uint32_t M = 1u << log2_m, W = M * L.stripes;
  const uint8_t* p = coef32 + (((uint64_t)L.blob * 32) << log2_n);
  for (uint32_t i = L.lane; i < M; i += L.lanes) {
    const Fr v = L.live && i < M / 2 ? fr_load_q(p + 32ull * (L.j + ((uint64_t)i << log2_cell))) : fr_zero();
    fr_ntt_put(a + L.sub, W, i * L.stripes, v);
  }
}
// fr_ntt_stage towards the values, on the lane's stripe
NBLS_FR_HD void fr_fk_stage(uint32_t* a, unsigned log2_m, unsigned log2_len, const Fr* sroots, const FrFkLane& L) {
  const uint32_t M = 1u << log2_m, W = M * L.stripes, len = 1u << log2_len;
  const bool unit = log2_len + 1 == log2_m;
  for (uint32_t b = L.lane; b < M / 2; b += L.lanes) {
    const uint32_t blk = b >> log2_len, lo = (blk << (log2_len + 1)) | (b & (len - 1)), hi = lo + len;
    const Fr u = fr_ntt_get(a + L.sub, W, lo * L.stripes), v = fr_ntt_get(a + L.sub, W, hi * L.stripes);
    const Fr t = unit ? v : fr_mul(v, sroots[2 * blk]);
    fr_ntt_put(a + L.sub, W, lo * L.stripes, fr_add(u, t));
    fr_ntt_put(a + L.sub, W, hi * L.stripes, fr_sub(u, t));
  }
}
// the lane's elements as big-endian scalars into pass A's array: out32[((blob M + i) c + j) * 32]
NBLS_FR_HD void fr_fk_store(const uint32_t* a, unsigned log2_cell, unsigned log2_m, const FrFkLane& L, uint8_t* out32) {
  const uint32_t M = 1u << log2_m, W = M * L.stripes;
  if (!L.live) return;
  for (uint32_t i = L.lane; i < M; i += L.lanes)
    fr_store_q(fr_ntt_get(a + L.sub, W, i * L.stripes), out32 + 32ull * (((((uint64_t)L.blob << log2_m) + i) << log2_cell) + L.j));
}
// scalar idx of the handle's one MSM: group (i, j) = idx / (n' - 1), term e = idx % (n' - 1) -> w_i^e, plain (the points are gathered to match: tau^(j + c (n' - 2 - e)))
NBLS_FR_HD Fr fr_fk_power(const Fr* sroots, unsigned log2_cell, unsigned log2_m, uint32_t idx) {
  const uint32_t terms = (1u << (log2_m - 1)) - 1, g = idx / terms, e = idx - g * terms;
  return fr_from_mont(fr_pow_index(sroots[g >> log2_cell], e, 12));
}
// B[k][i], plain.  With r = s_k / w_i:  sum_{u < n'} r^u = prod_{b < log2 n'} (1 + r^(2^b)), less the term r^(n' - 1) = r^n' / r;  w_i^(-(n' - 1)) = w_i^(-n') w_i.
// isroots: the table of the inverse roots, entry i = 1 / w_i.  n' = 1: the sum is empty and the entry zero
NBLS_FR_HD Fr fr_fk_matrix_entry(const Fr* sroots, const Fr* isroots, unsigned log2_m, uint32_t k, uint32_t i) {
  const Fr one = fr_one(), w = sroots[i], wi = isroots[i], r = fr_mul(sroots[k], wi), ri = fr_mul(isroots[k], w);
  Fr prod = one, rp = r, wp = wi;
  for (unsigned b = 0; b + 1 < log2_m; b++) { prod = fr_mul(prod, fr_add(one, rp)); rp = fr_sqr(rp); wp = fr_sqr(wp); }
  const Fr sum = fr_sub(prod, fr_mul(rp, ri));
  return fr_from_mont(fr_mul(fr_mul(sum, fr_mul(wp, w)), fr_inv_pow2(log2_m)));
}

// ---- The interpolation of cells (verify_cell_kzg_proof_batch of EIP-7594; kzg_cell_interp_kernel and nbls_sim_kzg_cell_interp).  Cell k holds the values of p on the coset
// h_k <omega_c> in bit-reversed order, h_k = g^rev(k), g = omega_2N; its interpolation polynomial has the coefficients
//   a_(k,i) = h_k^(-i) / c * (the way back of the network above, size c, on the cell's values)_i.
// c = 2^log2_cell <= 64 lanes own one cell: lane i holds element i between the stages and coefficient i after them, so a cell never leaves the registers of one wavefront.  A
// stage pairs lane i with lane i ^ len (the caller brings the partner's value: a cross-lane read on the device, an array on the simulator): the lane whose bit `len` is clear
// keeps lo + hi, the other (lo - hi) / zeta with the table of the inverse roots of size c -- fr_ntt_stage's butterfly with both halves computed on every lane and one
// selected.  Elements stay plain, the tables and factors are in Montgomery form.
NBLS_FR_HD Fr fr_cell_stage(const Fr& mine, const Fr& theirs, uint32_t i, unsigned log2_len, unsigned log2_cell, const Fr* iroots) {
  const uint32_t up = (uint32_t)0 - ((i >> log2_len) & 1);   // this lane holds the butterfly's upper element
  const Fr u = fr_select(up, theirs, mine), v = fr_select(up, mine, theirs);
  const Fr d = fr_sub(u, v);
  const Fr dz = log2_len + 1 == log2_cell ? d : fr_mul(d, iroots[2 * (i >> (log2_len + 1))]);   // (the one block of the last stage has zeta = 1)
  return fr_select(up, dz, fr_add(u, v));
}
// what coefficient i is multiplied by after the stages: (1 / h_k)^i / c, from the table's entry 1 / h_k (log2_cell bits of the index: no inversion, no long exponent)
NBLS_FR_HD Fr fr_cell_factor(const Fr& hinv, uint32_t i, unsigned log2_cell) { return fr_mul(fr_pow_index(hinv, i, log2_cell), fr_inv_pow2(log2_cell)); }
// entry k of the table of the M = 2^log2_m inverse shifts of (log2_n, log2_cell), log2_m = log2_n + 1 - log2_cell:  1 / h_k = g^(2 N - rev(k)), an exponent of 14 bits at most
NBLS_FR_HD Fr fr_cell_ishift_entry(const Fr& g, unsigned log2_n, unsigned log2_m, uint32_t k) { return fr_pow_index(g, (2u << log2_n) - fr_bitrev(k, log2_m), 14); }
// The lanes of a launch: workgroups of FR_CELL_LANES lanes, lane groups of c lanes side by side, group q of the launch on the cells q, q + groups, ..  The rows mode gives every
// cell a group of its own; the sum mode lets a group walk FR_CELL_WALK cells (fewer workgroups, hence fewer partial rows, while the device stays filled at the sizes that matter)
enum { FR_CELL_LANES = 256, FR_CELL_WALK = 4, FR_CELL_MAX_WG = 1024 };
NBLS_FR_HD uint32_t fr_cell_workgroups(uint32_t n_cells, unsigned log2_cell, bool sum) {
  const uint64_t per_wg = (uint64_t)(FR_CELL_LANES >> log2_cell) * (sum ? FR_CELL_WALK : 1), wg = (n_cells + per_wg - 1) / per_wg;
  return (uint32_t)(sum && wg > FR_CELL_MAX_WG ? FR_CELL_MAX_WG : wg);
}
// One cell on one lane, after the cross-lane part (bad: all ones when an element of the cell is >= r; v: the lane's value after the stages, of the cell's elements with a
// refused cell's replaced by zero): -> the lane's coefficient a_(k,i), zero for a cell that is out (pre != 0, refused, or past the end: `out` all ones)
NBLS_FR_HD Fr fr_cell_coeff(const Fr& v, const Fr& hinv, uint32_t i, unsigned log2_cell, uint32_t out) {
  return fr_select(out, fr_zero(), fr_mul(v, fr_cell_factor(hinv, i, log2_cell)));
}
// the cell's status: what came in (a decoder's refusal), else NBLS_ST_NON_CANONICAL for an element >= r, else 0
NBLS_FR_HD int fr_cell_status(int pre, uint32_t bad) { return pre ? pre : (int)(bad & 21); }

// ---- The recovery of a blob from at least half of its cells (recover_cells_and_kzg_proofs of EIP-7594; kzg_recover_z_kernel, kzg_recover_kernel and nbls_sim_kzg_recover).
// With M = 2 N / c cells, Z(x) = Zs(x^c), Zs(y) = prod over the missing k of (y - s_k), vanishes exactly on the missing cells and is CONSTANT on every cell: Zs(s_k) on cell k
// of H u gH, Zs(7^c s_j) on block j < M / 2 of the coset 7 H (the c elements c j .. c j + c of its bit-reversed order).  Nobody needs Z's coefficients: a blob takes the M
// values Zs(s_k) and the M / 2 inverses 1 / Zs(7^c s_j) -- never zero: 7 generates the multiplicative group, so 7^c s_j is no M-th root of unity.  The route, in transforms
// of size N only (a row of 2 N elements does not fit the compute unit's LDS), with E the given values and zero where a cell is missing:
//   (P Z)(x) = A(x) + x^N B(x), deg A, B < N (exact: deg P Z < N + (M / 2) c = 2 N);   S = A + B = to coefficients of (E Z on H);   D = A - B = the same of (E Z on gH), shift g;
//   T = A + 7^N B = S (1 + 7^N) / 2 + D (1 - 7^N) / 2;   (P Z on 7 H) = to values of T, shift 7;   block j times 1 / Zs(7^c s_j);   P = to coefficients, shift 7.
// P has degree < N, so its N values on 7 H determine it.  Then the cells are P's values on H and on gH, and every given cell is compared with them: with more than half of the
// cells the input can contradict itself, the division is then not exact, and the blob is refused (NBLS_ST_INCONSISTENT) instead of answered route-dependently.
// The index set is checked before anything is weighted (fr_recover_slots, on the host): at least M / 2 entries, every index < M, none twice.  Its result is the blob's slot
// map: slot[k] = the entry (of the staged cells) that holds cell k, or FR_RECOVER_NONE.  Elements stay plain, the Z values, tables and constants are in Montgomery form.
enum : uint32_t { FR_RECOVER_NONE = 0xffffffffu };
struct FrRecoverConsts { Fr g, ginv, seven, seveninv, kp, km, c7; };   // omega_2N, 1 / g, 7, 1 / 7, (1 + 7^N) / 2, (1 - 7^N) / 2, 7^c: the same for every blob of a call, made once on the host
NBLS_FR_HD FrRecoverConsts fr_recover_consts(unsigned log2_n, unsigned log2_cell) {
  FrRecoverConsts k;
  Fr seven = fr_zero(); seven.l[0] = 7;
  k.seven = fr_mul(seven, fr_r2());
  k.g = fr_omega(log2_n + 1);
  k.ginv = fr_inv(k.g); k.seveninv = fr_inv(k.seven);
  Fr p = k.seven;
  for (unsigned i = 0; i < log2_n; i++) p = fr_sqr(p);
  const Fr half = fr_inv_pow2(1);
  k.kp = fr_mul(fr_add(fr_one(), p), half); k.km = fr_mul(fr_sub(fr_one(), p), half);
  k.c7 = k.seven;
  for (unsigned i = 0; i < log2_cell; i++) k.c7 = fr_sqr(k.c7);
  return k;
}
// the slot map of one blob from its `count` indices, whose entries are first, first + 1, ..: returns 0, or 22 (NBLS_ST_BAD_CELLS) with an all-empty map
NBLS_FR_HD int fr_recover_slots(const uint32_t* idx, uint32_t first, uint64_t count, unsigned log2_m, uint32_t* slot) {
  const uint32_t M = 1u << log2_m;
  for (uint32_t k = 0; k < M; k++) slot[k] = FR_RECOVER_NONE;
  bool ok = count >= M / 2 && count <= M;
  for (uint64_t e = 0; ok && e < count; e++) {
    const uint32_t k = idx[e];
    if (k >= M || slot[k] != FR_RECOVER_NONE) ok = false; else slot[k] = first + (uint32_t)e;
  }
  if (ok) return 0;
  for (uint32_t k = 0; k < M; k++) slot[k] = FR_RECOVER_NONE;
  return 22;
}
// Z value v of a blob, one lane each: v < M: Zs(s_v) (zero where cell v is missing itself);  M <= v < 3 M / 2: 1 / Zs(7^c s_(v - M)), ONE inversion per block of c elements.
// sroots: the table of the M roots; the walk over k is the same on every lane
NBLS_FR_HD Fr fr_recover_z(const Fr* sroots, const uint32_t* slot, unsigned log2_m, uint32_t v, const Fr& c7) {
  const uint32_t M = 1u << log2_m;
  const bool block = v >= M;
  const Fr y = block ? fr_mul(c7, sroots[v - M]) : sroots[v];
  Fr acc = fr_one();
  for (uint32_t k = 0; k < M; k++) if (slot[k] == FR_RECOVER_NONE) acc = fr_mul(acc, fr_sub(y, sroots[k]));
  return block ? fr_inv(acc) : acc;
}
// the lane's elements t, t + lanes, .. of half `half` of the extension (0: on H, 1: on gH), each times its cell's Zs(s_k), zero where the cell is missing, into `a` (NULL:
// the canonical check alone); returns all ones when a given element is >= r.  cells: the staged entries of c elements each
NBLS_FR_HD uint32_t fr_recover_load(const uint8_t* cells, const uint32_t* slot, const Fr* zv, unsigned log2_n, unsigned log2_cell, uint32_t half, uint32_t lane, uint32_t lanes,
                                    uint32_t* a) {
  const uint32_t N = 1u << log2_n, c = 1u << log2_cell;
  uint32_t bad = 0;
  for (uint32_t i = lane; i < N; i += lanes) {
    const uint32_t x = half * N + i, k = x >> log2_cell, e = slot[k];
    Fr v = fr_zero();
    if (e != FR_RECOVER_NONE) {
      v = fr_load_q(cells + (((uint64_t)e << log2_cell) + (x & (c - 1))) * 32);
      bad |= fr_ge_r_mask(v);
      if (a) v = fr_mul(v, zv[k]);
    }
    if (a) fr_ntt_put(a, N, i, v);
  }
  return bad;
}
// the lane's elements: a = D in, S from s32 (32 bytes big-endian each) -> T_i 7^i = (S_i kp + D_i km) 7^i, ready for the stages towards the values on 7 H
NBLS_FR_HD void fr_recover_combine(uint32_t* a, const uint8_t* s32, uint32_t N, uint32_t lane, uint32_t lanes, unsigned log2_lanes, const FrRecoverConsts& k) {
  Fr pw = fr_pow_index(k.seven, lane, log2_lanes), step = k.seven;
  for (unsigned b = 0; b < log2_lanes; b++) step = fr_sqr(step);
  for (uint32_t i = lane; i < N; i += lanes) {
    const Fr t = fr_add(fr_mul(fr_load_q(s32 + 32ull * i), k.kp), fr_mul(fr_ntt_get(a, N, i), k.km));
    fr_ntt_put(a, N, i, fr_mul(t, pw));
    pw = fr_mul(pw, step);
  }
}
// the lane's elements of the values on 7 H, each times its block's inverse zinv[i / c]
NBLS_FR_HD void fr_recover_divide(uint32_t* a, const Fr* zinv, uint32_t N, unsigned log2_cell, uint32_t lane, uint32_t lanes) {
  for (uint32_t i = lane; i < N; i += lanes) fr_ntt_put(a, N, i, fr_mul(fr_ntt_get(a, N, i), zinv[i >> log2_cell]));
}
// the lane's elements of `a` = the recomputed half `half` against the given cells: all ones when one differs
NBLS_FR_HD uint32_t fr_recover_compare(const uint32_t* a, const uint8_t* cells, const uint32_t* slot, unsigned log2_n, unsigned log2_cell, uint32_t half, uint32_t lane,
                                       uint32_t lanes) {
  const uint32_t N = 1u << log2_n, c = 1u << log2_cell;
  uint32_t diff = 0;
  for (uint32_t i = lane; i < N; i += lanes) {
    const uint32_t x = half * N + i, e = slot[x >> log2_cell];
    if (e == FR_RECOVER_NONE) continue;
    const Fr v = fr_load_q(cells + (((uint64_t)e << log2_cell) + (x & (c - 1))) * 32), w = fr_ntt_get(a, N, i);
#pragma unroll
    for (int l = 0; l < FR_NL; l++) diff |= v.l[l] ^ w.l[l];
  }
  return diff ? 0xffffffffu : 0u;
}

// ---- The weighted sums of Groth16 public inputs (g16_input_sums_kernel, g16_sum_kernel and nbls_sim_g16_input_sums).  n proofs with m inputs each, the matrix row-major by
// proof (row i = the m inputs of proof i, 32 bytes big-endian each, 16-byte aligned), one weight w_i < 2^64 per row:
//   S_0 = sum_i w_i,   S_j = sum_i w_i x_(i,j),  j = 1 .. m,   over the rows that are in: pre[i] == 0 and every element of the row < r.
// The m + 1 columns of the result are walked by lanes: column 0 reads nothing (its element is 1), column c >= 1 reads element c - 1 of the row, so a wavefront's 64 lanes load
// 64 consecutive elements.  A workgroup of G16_LANES lanes is G16_GROUPS wavefronts on ONE tile of G16_TILE columns and on the rows q, q + groups, .. of its G16_GROUPS
// row groups (q = the workgroup's number among those of its tile * G16_GROUPS + wavefront; groups = G16_GROUPS * the launch's workgroups per tile: G16_ROWS_WG rows a workgroup until G16_MAX_WG of them
// are reached, more rows each from there on, so that the partial rows stay few).  Sixteen wavefronts a workgroup, four rows each: a row's loads wait for memory once per row,
// and with four wavefronts of sixteen rows the kernel took 28 us at 8192 x 16 and 88 us at 8192 x 328, the latency of sixteen dependent rounds.
// A row is in or out as a whole, so the wavefront looks at ALL its elements before it adds one: with m + 1 <= G16_TILE -- one tile -- every element is loaded once and checked
// where it is used; with more tiles the wavefront walks the row's other tiles for the check alone (the tiles of a row run side by side and meet in the cache; the check is eight
// subtractions an element against ~40 multiply-adds for the product).  Tile 0 writes the row's status.
// The products are NOT reduced one by one: w x < 2^64 * 2^256 = 2^320 is added into an accumulator of G16_ACC_NL limbs, 16 multiply-adds a row where a Montgomery product
// takes 136 (and the weight stays the two plain words it came as: there is no Montgomery form to bring it to), and a lane reduces ONCE, after its last row (g16_reduce).  The
// bound on the rows per reduction stands next to the accumulator's width below.  Fr addition is exact, so neither the split into workgroups nor the tree's order changes a byte.
enum { G16_TILE = 64, G16_GROUPS = 16, G16_LANES = G16_TILE * G16_GROUPS, G16_ROWS_WG = 64, G16_MAX_WG = 1024, G16_ACC_NL = 11 };
static const uint64_t G16_MAX_ELEMS = (uint64_t)1 << 24;   // n * m of one call; a lane adds at most one product per row of the call, and n <= n * m
struct G16Acc { uint32_t l[G16_ACC_NL]; };
static_assert(G16_MAX_ELEMS <= ((uint64_t)1 << (32 * G16_ACC_NL - 320)), "rows per reduction: 2^32 products below 2^320 stay below 2^352, the accumulator's eleven limbs");
NBLS_FR_HD uint32_t g16_tiles(uint32_t m) { return m / G16_TILE + 1; }   // ceil((m + 1) / G16_TILE)
NBLS_FR_HD uint32_t g16_workgroups(uint32_t n) { const uint32_t w = (n + G16_ROWS_WG - 1) / G16_ROWS_WG; return w > G16_MAX_WG ? (uint32_t)G16_MAX_WG : w; }
NBLS_FR_HD G16Acc g16_acc_zero() { G16Acc a; for (int i = 0; i < G16_ACC_NL; i++) a.l[i] = 0; return a; }
// acc += x * (whi 2^32 + wlo): two rows of operand scanning, the carry walked to the accumulator's top
NBLS_FR_HD void g16_mac(G16Acc& acc, const Fr& x, uint32_t wlo, uint32_t whi) {
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint32_t w = k ? whi : wlo;
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < FR_NL; j++) { c += (uint64_t)x.l[j] * w + acc.l[j + k]; acc.l[j + k] = (uint32_t)c; c >>= 32; }
#pragma unroll
    for (int j = FR_NL + k; j < G16_ACC_NL; j++) { c += acc.l[j]; acc.l[j] = (uint32_t)c; c >>= 32; }
  }
}
// the accumulator mod r, plain: lo + hi 2^256 with lo = the low eight limbs (lo R^2 / R = lo R, then out of Montgomery form) and hi < 2^96 (hi R^2 / R = hi 2^256)
NBLS_FR_HD Fr g16_reduce(const G16Acc& acc) {
  Fr lo, hi = fr_zero();
#pragma unroll
  for (int i = 0; i < FR_NL; i++) lo.l[i] = acc.l[i];
#pragma unroll
  for (int i = FR_NL; i < G16_ACC_NL; i++) hi.l[i - FR_NL] = acc.l[i];
  return fr_add(fr_from_mont(fr_mul(lo, fr_r2())), fr_mul(hi, fr_r2()));
}
// One row on one lane: the lane's own element -- column tile * G16_TILE + lane of the result: 1 for column 0, zero past column m -- and in *bad all ones when an element of
// the row that this lane looked at is >= r (the wavefront ORs the lanes).  Lanes past the row's end read nothing
NBLS_FR_HD Fr g16_row_lane(const uint8_t* row32, uint32_t m, uint32_t tiles, uint32_t tile, uint32_t lane, uint32_t* bad) {
  Fr x = fr_zero(); uint32_t b = 0;
  for (uint32_t tt = 0; tt < tiles; tt++) {
    const uint32_t c = tt * G16_TILE + lane;
    if (c < 1 || c > m) continue;
    const Fr v = fr_load_q(row32 + 32ull * (c - 1));
    b |= fr_ge_r_mask(v);
    if (tt == tile) x = v;
  }
  if (tile == 0 && lane == 0) x.l[0] = 1;
  *bad = b;
  return x;
}
// the row's product into the lane's accumulator: the weight's two words (w32: 32 bytes big-endian, < 2^64) under the row's mask (all ones: the row is out)
NBLS_FR_HD void g16_row_add(G16Acc& acc, const Fr& x, const uint8_t* w32, uint32_t out) {
  const Fr w = fr_load_q(w32);
  g16_mac(acc, x, w.l[0] & ~out, w.l[1] & ~out);
}
// the row's status: what came in, else NBLS_ST_NON_CANONICAL for an element >= r, else 0
NBLS_FR_HD int g16_row_status(int pre, uint32_t bad) { return pre ? pre : (int)(bad & 21); }

}  // namespace nbls
