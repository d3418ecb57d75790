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
NBLS_FR_HD uint32_t fr_group_of(const uint32_t* off, uint32_t ngroups, uint32_t k) {
  uint32_t lo = 0, hi = ngroups;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}
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

}  // namespace nbls
