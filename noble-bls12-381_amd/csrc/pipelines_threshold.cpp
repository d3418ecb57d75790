// pipelines_threshold.cpp -- the scalar field Fr on the device (reference math.ts:295-386) and the recombination of threshold shares: from t-of-n shares sigma_k = [f(x_k)]H(m)
// (or public-key shares [f(x_k)]G1) of a polynomial f the group's signature [f(0)]H(m) = sum_k [lambda_k]sigma_k with the Lagrange coefficients at zero
//   lambda_k = prod_{j != k} x_j / (x_j - x_k)
// for many groups in one call.  One chain on the call's stream, as verify_multiple_pipeline builds its own: the inputs travel as one copy from the page-locked block, nothing is
// decided on the host before the single read-back.
//   H2D copy -> shares: dev_decompress (PointG2.fromSignature / PointG1.fromHex rules)
//            -> identifiers: Montgomery form -> fr_lagrange_kernel -> canonical scalars (fr_kernels.hip)
//            -> [lambda_k]share_k (dev_point_mul, stopped at its projective points; the shares are in the subgroup after decoding and the coefficients are public, so G2 takes the
//               psi-split ladders) -> one sum per group (segment_sums, shared with the multi-verify calls) -> affine -> P_G*_COMPRESS -> status kernel -> D2H copy
// Scratch slots: SB_STAGED and SB_THR_* (nbls_internal.h, M_THR_OWN); the decoder and the ladder run on the main slots (DEC_MAIN, M_LADDER) one after the other.
#include "nbls_internal.h"
#include <algorithm>

static const size_t THR_MAX_SHARES = (size_t)1 << 24, THR_MAX_GROUP = (size_t)1 << 16;   // u32 ids and ranks, at most 16 rounds of the segmented sum

// what the three group calls refuse before any device work; fills in the number of shares and the largest group
static int check_groups(size_t n_groups, const uint32_t* off, size_t* n, size_t* maxgroup) {
  if (!n_groups || !off || n_groups > THR_MAX_SHARES || !strict_groups(n_groups, off, n, maxgroup)) return NBLS_EINVAL;
  return *n > THR_MAX_SHARES || *maxgroup > THR_MAX_GROUP ? NBLS_EINVAL : NBLS_OK;
}

// the coefficients of n identifiers (wire bytes, device) in n_groups groups (d_off: relative offsets, device) on `s` -> *L32: n canonical scalars (at dst when the caller has a
// place for them, else in the slot); *bad_group: one word per group
static int dev_lagrange(nbls_ctx* ctx, size_t n, size_t n_groups, const uint32_t* d_off, const uint8_t* d_ids, uint8_t* dst, uint8_t** L32, uint32_t** bad_group, hipStream_t s) {
  uint8_t* F; int r;
  if ((r = need(ctx, SB_THR_SCALARS, n * (32 + 32 + 4 + 32) + n_groups * 4, &F))) return r;
  uint8_t *X = F, *L = X + n * 32, *slot = L + n * 32, *out = dst ? dst : slot;
  uint32_t *group_of = (uint32_t*)(slot + n * 32), *bad = group_of + n;
  LAUNCHCHK(nbls_fr_lagrange_launch((unsigned)n, (unsigned)n_groups, d_off, d_ids, X, L, group_of, bad, out, s));
  *L32 = out; *bad_group = bad;
  return NBLS_OK;
}

static int combine_pipeline(nbls_ctx* ctx, bool g2, size_t n_groups, const uint32_t* off, size_t n, size_t maxgroup, const uint8_t* ids32, const uint8_t* shares, uint8_t* out,
                            int8_t* status) {
  const size_t e = g2 ? 96 : 48, a = 2 * e, p = (g2 ? 6 : 3) * RAW;
  // the staged block: identifiers | shares | offsets (relative); what is read back: compressed sums | statuses
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_ids = io.bytes(ids32 + (size_t)off[0] * 32, n * 32), o_sh = io.bytes(shares + (size_t)off[0] * e, n * e), o_off = io.rel(off, n_groups), back = n_groups * e + n_groups;
  uint8_t *c, *SH, *O; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_THR_SHARES, n * a + n, &SH)) || (r = need(ctx, SB_THR_OUT, n_groups * a + ((back + 15) & ~(size_t)15), &O)) ||
      (r = io.send(c, back)))
    return r;
  int8_t* ST = (int8_t*)(SH + n * a);
  uint8_t *AFF = O + ((back + 15) & ~(size_t)15), *OST = O + n_groups * e;
  const uint32_t* d_off = (const uint32_t*)(c + o_off);
  if ((r = dev_decompress(ctx, g2, n, c + o_sh, SH, ST, s))) return r;
  uint8_t *L32, *Pj; uint32_t* bad;
  if ((r = dev_lagrange(ctx, n, n_groups, d_off, c + o_ids, nullptr, &L32, &bad, s))) return r;
  // the ladders.  G2: the psi-split forms of sign -- up to sac_max items the sign-aligned one, which reads raw projective points (made here, in the slot sign's hash chain leaves
  // them in); a share that did not decode yields some point or other, which segment_sums replaces by the identity
  const void* pts = SH; size_t stride = a;
  if (g2 && g2_ladder_takes_projective(ctx, n)) {
    uint8_t* PR;
    if ((r = need(ctx, SB_WORK_B, n * p, &PR)) || (r = run(ctx, P_G2_TO_PROJ, n, {B(1, SH, a), B(3, PR, p)}, s))) return r;
    pts = PR; stride = p;
  }
  if ((r = dev_point_mul(ctx, g2, n, pts, stride, L32, nullptr, nullptr, s, false, g2, nullptr, &Pj))) return r;
  SegSums o;
  if ((r = segment_sums(ctx, g2, SEG_THR, n, n_groups, d_off, nullptr, Pj, ST, maxgroup, AFF, &o, s))) return r;
  if ((r = run(ctx, g2 ? P_G2_COMPRESS : P_G1_COMPRESS, n_groups, {B(0, AFF, a), B(2, O, e)}, s))) return r;
  LAUNCHCHK(nbls_fr_combine_status_launch((unsigned)n_groups, (unsigned)e, bad, o.first, o.st, o.zero, O, OST, s));
  return io.fetch_to(O, out, n_groups * e, status, n_groups);
}

static int combine_shares(nbls_ctx* ctx, bool g2, size_t n_groups, const uint32_t* off, const uint8_t* ids32, const uint8_t* shares, uint8_t* out, int8_t* status) {
  WHOLE_CALL(ctx);
  size_t n = 0, maxgroup = 0;
  if (!ctx || !ids32 || !shares || !out || check_groups(n_groups, off, &n, &maxgroup)) return NBLS_EINVAL;
  return combine_pipeline(ctx, g2, n_groups, off, n, maxgroup, ids32, shares, out, status);
}
EXPORT int nbls_g2_combine_shares(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* ids32, const uint8_t* shares96, uint8_t* out96, int8_t* status) {
  return combine_shares(ctx, true, n_groups, group_offsets, ids32, shares96, out96, status);
}
EXPORT int nbls_g1_combine_shares(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* ids32, const uint8_t* shares48, uint8_t* out48, int8_t* status) {
  return combine_shares(ctx, false, n_groups, group_offsets, ids32, shares48, out48, status);
}

EXPORT int nbls_lagrange_at_zero(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* ids32, uint8_t* out32, int8_t* status) {
  WHOLE_CALL(ctx);
  size_t n = 0, maxgroup = 0;
  if (!ctx || !ids32 || !out32 || check_groups(n_groups, group_offsets, &n, &maxgroup)) return NBLS_EINVAL;
  // the staged block: identifiers | offsets (relative); what is read back: coefficients | statuses
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_ids = io.bytes(ids32 + (size_t)group_offsets[0] * 32, n * 32), o_off = io.rel(group_offsets, n_groups), back = n * 32 + n_groups;
  uint8_t *c, *O, *L32; uint32_t* bad; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_THR_OUT, back, &O)) || (r = io.send(c, back))) return r;
  if ((r = dev_lagrange(ctx, n, n_groups, (const uint32_t*)(c + o_off), c + o_ids, O, &L32, &bad, s))) return r;
  LAUNCHCHK(nbls_fr_group_status_launch((unsigned)n_groups, bad, O + n * 32, s));
  return io.fetch_to(O, out32, n * 32, status, n_groups);
}

EXPORT int nbls_fr_op_batch(nbls_ctx* ctx, int op, size_t n, const uint8_t* a32, const uint8_t* b32, uint8_t* out32, int8_t* status) {
  const bool unary = op == NBLS_FROP_NEG || op == NBLS_FROP_SQR || op == NBLS_FROP_INV;
  if (!ctx || op < NBLS_FROP_ADD || op > NBLS_FROP_POW || n > THR_MAX_SHARES || (n && (!a32 || !out32 || (!unary && !b32)))) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  // the staged block: first operands | second operands (binary operations); what is read back: results | statuses
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_a = io.bytes(a32, n * 32), o_b = io.bytes(b32, unary ? 0 : n * 32), back = n * 32 + n;
  uint8_t *c, *O; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_THR_OUT, back, &O)) || (r = io.send(c, back))) return r;
  LAUNCHCHK(nbls_fr_op_launch((unsigned)n, op, c + o_a, unary ? nullptr : c + o_b, O, O + n * 32, s));
  return io.fetch_to(O, out32, n * 32, status, n);
}
