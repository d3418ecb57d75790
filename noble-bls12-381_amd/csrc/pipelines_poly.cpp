// pipelines_poly.cpp -- commitment polynomials evaluated in the exponent: from the published coefficients A_j = [a_j]G of a DKG / Feldman VSS the public keys of the shares,
//   pk_k = F(x_k) = sum_j [x_k^j] A_j,
// for many polynomials (groups) and many identifiers per polynomial in one call.  It closes the threshold flow of pipelines_threshold.cpp: commitment -> share keys ->
// verify_multiple_shared over the partial signatures -> combine_shares -> verify under A_0.  One chain on the call's stream, nothing decided on the host before the single read-back:
//   H2D copy -> coefficients: dev_decompress (PointG1.fromHex / PointG2.fromSignature rules) -> raw projective, the identity in place of what did not decode or is zero, the first
//               bad position of every group (agg_kernels.hip, as segment_sums labels its segments)
//            -> per slab of identifiers: Horner's rule, one item per identifier: acc <- A_(T-1), then acc <- [x]acc + A_j for j = T - 2 .. 0 (programs.h ExtraProg: the 16-bit form
//               when every identifier of the call is below 2^16 as given, else the 256-bit form), the step's coefficient of every item laid out by poly_coef_kernel (a group with
//               fewer than T coefficients meets the identity in its missing high steps: a no-op on an identity accumulator) -> affine -> P_G*_COMPRESS
//            -> status kernel -> D2H copy
// Scratch slots: SB_STAGED and SB_POLY_* (nbls_internal.h, M_POLY_OWN); the decoder runs on the main slots (DEC_MAIN) before anything of a slab exists.
#include "nbls_internal.h"
#include <algorithm>

static const size_t POLY_MAX_COEFS = (size_t)1 << 24, POLY_MAX_GROUP = (size_t)1 << 16, POLY_MAX_IDS = (size_t)1 << 22;
static const size_t POLY_SLAB_DEFAULT = (size_t)1 << 18;   // identifiers per slab: 2^18 x (accumulator, norm, inverse, affine point, step coefficient) = 160 MB in G1, 285 MB in G2

static int poly_pipeline(nbls_ctx* ctx, bool g2, size_t n_groups, const uint32_t* coff, size_t C, size_t T, const uint8_t* coefs, const uint32_t* ioff, size_t M, const uint8_t* ids32,
                         uint8_t* out, int8_t* status) {
  const size_t e = g2 ? 96 : 48, a = 2 * e, p = (g2 ? 6 : 3) * RAW;
  const uint8_t* ids = ids32 + (size_t)ioff[0] * 32;
  const bool low16 = scalars_bit_length(M, ids) <= 16;
  const ExtraProg xp = g2 ? (low16 ? XP_POLY_G2_16 : XP_POLY_G2_256) : (low16 ? XP_POLY_G1_16 : XP_POLY_G1_256);
  const size_t slab = std::min(M, ctx->poly_slab ? ctx->poly_slab : POLY_SLAB_DEFAULT);
  // the staged block: coefficients | identifiers | coefficient offsets | identifier offsets (both relative); what is read back: compressed points | statuses
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_cf = io.bytes(coefs + (size_t)coff[0] * e, C * e), o_ids = io.bytes(ids, M * 32), o_coff = io.rel(coff, n_groups), o_ioff = io.rel(ioff, n_groups), back = M * e + M;
  uint8_t *c, *CF, *LB, *AC, *SP, *O; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_POLY_COEFS, C * (a + p) + C, &CF)) || (r = need(ctx, SB_POLY_LABELS, (2 * C + n_groups + M) * 4 + C, &LB)) ||
      (r = need(ctx, SB_POLY_ACC, slab * (p + 2 * RAW + a), &AC)) || (r = need(ctx, SB_POLY_STEP, slab * p, &SP)) || (r = need(ctx, SB_POLY_OUT, ((back + 15) & ~(size_t)15) + M, &O)) ||
      (r = upload_extra(ctx, xp)) || (r = io.send(c, back)))
    return r;
  uint8_t *AFF = CF, *PR = AFF + C * a; int8_t* ST = (int8_t*)(PR + C * p);
  uint32_t *set_id = (uint32_t*)LB, *rank = set_id + C, *first = rank + C, *group_of = first + n_groups; int8_t* GST = (int8_t*)(group_of + M);
  uint8_t *ACC = AC, *N = ACC + slab * p, *NI = N + slab * RAW, *AFF2 = NI + slab * RAW;
  uint8_t *OST = O + M * e, *Z = O + ((back + 15) & ~(size_t)15);
  const uint8_t* d_ids = c + o_ids;
  const uint32_t *d_coff = (const uint32_t*)(c + o_coff), *d_ioff = (const uint32_t*)(c + o_ioff);
  if ((r = dev_decompress(ctx, g2, C, c + o_cf, AFF, ST, s))) return r;
  if ((r = run(ctx, g2 ? P_G2_TO_PROJ : P_G1_TO_PROJ, C, {B(g2 ? 1 : 0, AFF, a), B(3, PR, p)}, s))) return r;
  // every coefficient's group and status, every group's first position with a status >= 2; then the identity where the status is not 0 (in place)
  LAUNCHCHK(nbls_agg_keys_launch((unsigned)C, (unsigned)n_groups, d_coff, nullptr, ST, set_id, rank, GST, first, s));
  const uint8_t* ident = g2 ? ctx->ident_g2 : ctx->ident_g1;
  LAUNCHCHK(nbls_agg_points_launch(C, (unsigned)p, nullptr, GST, ident, PR, PR, s));
  LAUNCHCHK(nbls_poly_group_launch((unsigned)M, (unsigned)n_groups, d_ioff, group_of, s));
  const DevProgram& step = ctx->extra[xp];
  for (size_t k0 = 0; k0 < M; k0 += slab) {
    const size_t ms = std::min(slab, M - k0);
    LAUNCHCHK(nbls_poly_coef_launch(ms, (unsigned)p, (unsigned)(T - 1), group_of + k0, d_coff, ident, PR, ACC, s));
    for (size_t j = T - 1; j-- > 0;) {
      // one polynomial in the call: every item meets the same coefficient, read in place (stride 0)
      if (n_groups > 1) LAUNCHCHK(nbls_poly_coef_launch(ms, (unsigned)p, (unsigned)j, group_of + k0, d_coff, ident, PR, SP, s));
      if ((r = run_dev(ctx, step, -1, ms, {B(2, d_ids + k0 * 32, 32), B(3, ACC, p), n_groups > 1 ? B(4, SP, p) : B(4, PR + j * p, 0)}, s, nullptr, nullptr))) return r;
    }
    if ((r = to_affine(ctx, g2, ms, ACC, N, NI, AFF2, Z + k0, s))) return r;
    if ((r = run(ctx, g2 ? P_G2_COMPRESS : P_G1_COMPRESS, ms, {B(0, AFF2, a), B(2, O + k0 * e, e)}, s))) return r;
  }
  LAUNCHCHK(nbls_poly_status_launch((unsigned)M, (unsigned)e, group_of, first, GST, Z, O, OST, s));
  return io.fetch_to(O, out, M * e, status, M);
}

static int poly_eval(nbls_ctx* ctx, bool g2, size_t n_groups, const uint32_t* coff, const uint8_t* coefs, const uint32_t* ioff, const uint8_t* ids32, uint8_t* out, int8_t* status) {
  WHOLE_CALL(ctx);
  size_t C = 0, T = 0, M = 0, maxids = 0;
  if (!ctx || !coff || !coefs || !ioff || !ids32 || !out || !n_groups || n_groups > POLY_MAX_IDS || !strict_groups(n_groups, coff, &C, &T) || !strict_groups(n_groups, ioff, &M, &maxids) ||
      T > POLY_MAX_GROUP || C > POLY_MAX_COEFS || M > POLY_MAX_IDS)
    return NBLS_EINVAL;
  return poly_pipeline(ctx, g2, n_groups, coff, C, T, coefs, ioff, M, ids32, out, status);
}
EXPORT int nbls_g1_poly_eval(nbls_ctx* ctx, size_t n_groups, const uint32_t* coef_offsets, const uint8_t* coefs48, const uint32_t* id_offsets, const uint8_t* ids32, uint8_t* out48,
                             int8_t* status) {
  return poly_eval(ctx, false, n_groups, coef_offsets, coefs48, id_offsets, ids32, out48, status);
}
EXPORT int nbls_g2_poly_eval(nbls_ctx* ctx, size_t n_groups, const uint32_t* coef_offsets, const uint8_t* coefs96, const uint32_t* id_offsets, const uint8_t* ids32, uint8_t* out96,
                             int8_t* status) {
  return poly_eval(ctx, true, n_groups, coef_offsets, coefs96, id_offsets, ids32, out96, status);
}
