// pipelines_groth16.cpp -- batched Groth16 verification on BLS12-381 (include/nbls.h has the contract).  The key holds alpha in G1, beta, gamma, delta in G2 and IC_0 .. IC_m in
// G1; proof i = (A_i, B_i, C_i) with inputs x_i1 .. x_im holds when, with L_i = IC_0 + sum_j [x_ij]IC_j,
//   e(A_i, B_i) * e(L_i, -gamma) * e(C_i, -delta) * e(alpha, -beta) = 1.
// n proofs are checked together with the secret weights r_i of nbls_verify_multiple (rlc_weights.h):
//   prod_i e([r_i]A_i, B_i) * e(sum_j [S_j]IC_j, -gamma) * e(sum_i [r_i]C_i, -delta) * e([S_0]alpha, -beta) = 1,   S_0 = sum_i r_i,  S_j = sum_i r_i x_ij mod r
// (the signs on the fixed G2 points, whose line tables the handle keeps: no point is negated on the device).  One chain on the context's stream:
//   H2D copy -> g16_split_kernel: A | C into one array, B into another -> weights -> dev_decompress of the 2 n G1 points and of the n G2 points (subgroup checks included)
//            -> g16_pre_kernel: what the decoders say -> g16_input_sums_kernel / g16_sum_kernel: the canonical check of every input, the m + 1 scalars S_j, the statuses before
//               any pairing -> g16_items_kernel: a proof that is out gets fixed points and the scalar zero
//            -> [r_i]A_i by P_G1_MUL64, to affine -> sum [r_i]C_i: a 64-bit MSM -> sum [S_j]IC_j: a 256-bit MSM over m + 1 points -> [S_0]alpha: one ladder
//            -> n Miller loops with the decoded B_i, three against the handle's tables -> product -> final exponentiation -> compared with one -> D2H copy
// Nothing is decided on the host before that read-back: the verdict, the three zero flags and the n statuses come back together.  The combined check accepts when every status
// is 0, none of the three combined points is the zero point (the generator stands in for it in the Miller loop while the flag decides) and the result is one.
// Where it does not accept and the caller asked for statuses, the per-proof pass judges every proof with the first equation, in chunks of whole proofs under the batched MSM's
// bounds: L_i = msm_rows_dev against the handle's converted points (the rows are the staged inputs themselves) plus IC_0 by one complete addition -- a zero L_i is a factor of
// one --, millerLoop(A_i, B_i), two Miller loops against the shared tables with table_stride = 0, the one value of millerLoop(alpha, table of -beta), one batched final
// exponentiation, rlc_is_one.  nbls_groth16_prepare_inputs is the L_i of that pass, compressed.
// This file owns the chain up to the three combined points and the chunk loop's Miller values.  The seed, the read-back header with its verdict (verifier_frame.h), the
// combined check's tail, the close of a chunk and the read-back of the final statuses are the weighted verifiers' shared helpers (kzg_common.cpp); KzgFrame itself is not
// used: there is no tau point and no line table to build per call.
// Scratch slots: SB_STAGED and SB_G16_* (nbls_internal.h, M_G16_OWN); the decoders and the ladder run on the main slots, the MSMs on MSM_RLC's, the batched MSM on SB_MSMB_*.
#include "nbls_internal.h"
#include "fr_exec.h"
#include <algorithm>

static const size_t G16_MAX_PROOFS = MSMB_MAX_GROUPS, G16_MAX_INPUTS = (size_t)1 << 16;

EXPORT void nbls_groth16_vk_destroy(nbls_groth16_vk* vk) {
  if (!vk) return;
  handle_free(vk->device, {vk->mem});
  delete vk;
}
EXPORT int nbls_groth16_vk_inputs(const nbls_groth16_vk* vk, size_t* m) {
  if (!vk || !m) return NBLS_EINVAL;
  *m = vk->m;
  return NBLS_OK;
}
// the handle's block filled: alpha and the IC points decoded in place, the three G2 points decoded, read back, negated on the host and sent again, their line tables, the
// converted IC points and IC_0 raw projective.  status: m + 5 entries in the header's order
static int g16_vk_build(nbls_ctx* ctx, nbls_groth16_vk* vk, const uint8_t* alpha48, const uint8_t* const g2_96[3], const uint8_t* ic48, int8_t* status) {
  const size_t m = vk->m, np = m + 2, p = 3 * RAW;
  std::vector<uint8_t> h48(np * 48), h96(3 * 96), g2(3 * 192), neg(3 * 192);
  std::vector<int8_t> st(np + 3);
  memcpy(h48.data(), alpha48, 48); memcpy(h48.data() + 48, ic48, (m + 1) * 48);
  for (int k = 0; k < 3; k++) memcpy(h96.data() + 96 * k, g2_96[k], 96);
  LOCKED(ctx);
  HostIO io{ctx};
  void *d48 = io.alloc(np * 48), *d96 = io.alloc(3 * 96), *dg2 = io.alloc(3 * 192), *dst = io.alloc(np + 3);
  if (!d48 || !d96 || !dg2 || !dst) return NBLS_EHIP;
  size_t sz = 0;
  const size_t a_pts = carve(&sz, np * 96), a_neg = carve(&sz, 3 * 192), a_tb = carve(&sz, 3 * LINE_BYTES), a_conv = carve(&sz, (m + 1) * 2 * p), a_proj = carve(&sz, p);
  HIPCHK(hipMalloc(&vk->mem, sz));   // (freed by the caller's nbls_groth16_vk_destroy on every error return)
  vk->alpha96 = vk->mem + a_pts; vk->ic96 = vk->alpha96 + 96; vk->g2neg = vk->mem + a_neg; vk->tables = vk->mem + a_tb; vk->ic_conv = vk->mem + a_conv; vk->ic0_proj = vk->mem + a_proj;
  int r;
  HIPCHK(hipMemcpyAsync(d48, h48.data(), np * 48, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d96, h96.data(), 3 * 96, hipMemcpyHostToDevice, s));
  if ((r = dev_decompress(ctx, false, np, d48, vk->alpha96, dst, s)) || (r = dev_decompress(ctx, true, 3, d96, dg2, (uint8_t*)dst + np, s))) return r;
  HIPCHK(hipMemcpyAsync(st.data(), dst, np + 3, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(g2.data(), dg2, 3 * 192, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  bool bad = false;
  for (size_t k = 0; k < np + 3; k++) bad = bad || st[k] != 0;   // 1: a zero point, which no real key contains
  if (status) {
    status[0] = st[0];
    for (int k = 0; k < 3; k++) status[1 + k] = st[np + k];
    memcpy(status + 4, st.data() + 1, m + 1);
  }
  if (bad) return NBLS_EDECODE;
  for (int k = 0; k < 3; k++) g2_wire_negate(g2.data() + 192 * k, neg.data() + 192 * k);
  HIPCHK(hipMemcpyAsync(vk->g2neg, neg.data(), 3 * 192, hipMemcpyHostToDevice, s));
  if ((r = run(ctx, P_LINES_Q, 3, {B(1, vk->g2neg, 192), B(3, vk->tables, LINE_BYTES)}, s)) || (r = run(ctx, P_G1_MSM_PREP, m + 1, {B(0, vk->ic96, 96), B(3, vk->ic_conv, 2 * p)}, s)) ||
      (r = run(ctx, P_G1_TO_PROJ, 1, {B(0, vk->ic96, 96), B(3, vk->ic0_proj, p)}, s)))
    return r;
  HIPCHK(hipStreamSynchronize(s));   // (neg is read by the copy until here; an error return waits in ~HostIO)
  return NBLS_OK;
}
EXPORT int nbls_groth16_vk_create(nbls_ctx* ctx, size_t m, const uint8_t* alpha_g1_48, const uint8_t* beta_g2_96, const uint8_t* gamma_g2_96, const uint8_t* delta_g2_96,
                                  const uint8_t* ic48, int8_t* status, nbls_groth16_vk** out) {
  WHOLE_CALL(ctx);
  if (out) *out = nullptr;
  if (!ctx || !m || m > G16_MAX_INPUTS || !alpha_g1_48 || !beta_g2_96 || !gamma_g2_96 || !delta_g2_96 || !ic48 || !out) return NBLS_EINVAL;
  const uint8_t* const g2[3] = {beta_g2_96, gamma_g2_96, delta_g2_96};
  return handle_create(ctx, out, nbls_groth16_vk_destroy, [&](nbls_groth16_vk* vk) { vk->m = m; return g16_vk_build(ctx, vk, alpha_g1_48, g2, ic48, status); });
}

EXPORT int nbls_groth16_input_sums(nbls_ctx* ctx, size_t n, size_t m, const uint8_t* inputs32, const uint8_t* weights32, const int8_t* pre, uint8_t* out32, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !n || !m || !inputs32 || !weights32 || !out32 || n > G16_MAX_ELEMS || m > G16_MAX_ELEMS || n * m > G16_MAX_ELEMS) return NBLS_EINVAL;
  for (size_t i = 0; i < n; i++) for (int k = 0; k < 24; k++) if (weights32[32 * i + k]) return NBLS_EINVAL;   // a weight >= 2^64
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_in = io.bytes(inputs32, n * m * 32), o_w = io.bytes(weights32, n * 32), o_pre = io.bytes(pre, pre ? n : 0), sums = (m + 1) * 32;
  size_t sz = 0;
  const size_t a_part = carve(&sz, (size_t)g16_workgroups((uint32_t)n) * sums), a_out = carve(&sz, sums + n);
  uint8_t *c, *SC; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_G16_SCALARS, sz, &SC)) || (r = io.send(c, sums + n))) return r;
  uint8_t* O = SC + a_out;
  LAUNCHCHK(nbls_g16_input_sums_launch((unsigned)n, (unsigned)m, c + o_in, c + o_w, pre ? c + o_pre : nullptr, SC + a_part, O, O + sums, s));
  return io.fetch_to(O, out32, sums, status, n);
}

// proofs per pass of the batched MSM: whole proofs under its bounds, fewer where the tuning key says so
static size_t g16_chunk(const nbls_ctx* ctx, size_t n, size_t m) {
  size_t per = std::min({n, MSMB_MAX_ITEMS / m, MSMB_MAX_GROUPS});
  if (ctx->g16_chunk && ctx->g16_chunk < per) per = ctx->g16_chunk;
  return per;
}
// One chunk's L_i: the buffers of `per` proofs, carved into the caller's block.  aff / zf: the row sums and their zero flags; pj, nn, ni: raw projective, norms, inverses;
// l / lz: L_i affine and its zero flag
struct G16Rows { size_t aff, zf, pj, nn, ni, l, lz; };
static G16Rows g16_rows_carve(size_t per, size_t* off) {
  G16Rows a;
  a.aff = carve(off, per * 96); a.zf = carve(off, per); a.pj = carve(off, per * 3 * RAW); a.nn = carve(off, per * RAW); a.ni = carve(off, per * RAW); a.l = carve(off, per * 96); a.lz = carve(off, per);
  return a;
}
// L_i = IC_0 + sum_j [x_ij]IC_j for the cnt rows at rows32 (device memory; a row that is out holds zeros): the rows form of the batched MSM against IC_1 .. IC_m, the identity
// where a sum is the zero point, one complete addition with IC_0, affine again with L_i's own zero flag
static int g16_l_points(nbls_ctx* ctx, const nbls_groth16_vk* vk, const MsmbPlan& pl, size_t cnt, const uint8_t* rows32, uint8_t* block, const G16Rows& a, hipStream_t s) {
  const size_t p = 3 * RAW; int r;
  uint8_t *AFF = block + a.aff, *ZF = block + a.zf, *PJ = block + a.pj;
  if ((r = msm_rows_dev(ctx, pl, vk->ic_conv + 2 * p, rows32, AFF, ZF, s)) || (r = run(ctx, P_G1_TO_PROJ, cnt, {B(0, AFF, 96), B(3, PJ, p)}, s))) return r;
  LAUNCHCHK(nbls_agg_points_launch(cnt, (unsigned)p, nullptr, ZF, ctx->ident_g1, PJ, PJ, s));
  if ((r = run(ctx, P_G1_ADD_AB, cnt, {B(3, PJ, p), B(4, vk->ic0_proj, 0), B(5, PJ, p)}, s))) return r;
  return to_affine(ctx, false, cnt, PJ, block + a.nn, block + a.ni, block + a.l, block + a.lz, s);
}

EXPORT int nbls_groth16_prepare_inputs(nbls_ctx* ctx, const nbls_groth16_vk* vk, size_t n, const uint8_t* inputs32, uint8_t* out48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !vk || !n || !inputs32 || !out48 || vk->device != ctx->device || n > G16_MAX_PROOFS || n * vk->m > G16_MAX_ELEMS) return NBLS_EINVAL;
  const size_t m = vk->m, per = g16_chunk(ctx, n, m), tail = n % per, sums = (m + 1) * 32, back = n * 48 + n;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_in = io.bytes(inputs32, n * m * 32);
  size_t sz_sc = 0, sz_it = 0;
  const size_t a_w = carve(&sz_sc, n * 32), a_part = carve(&sz_sc, (size_t)g16_workgroups((uint32_t)n) * sums), a_S = carve(&sz_sc, sums), a_pre = carve(&sz_sc, n);
  const G16Rows a = g16_rows_carve(per, &sz_it);
  MsmbPlan pl_full, pl_tail;
  uint8_t *c, *SC, *O, *IT; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_G16_SCALARS, sz_sc, &SC)) || (r = need(ctx, SB_G16_OUT, back, &O)) || (r = need(ctx, SB_G16_ITEMS, sz_it, &IT)) ||
      (r = msm_rows_dev_plan(ctx, m, per, &pl_full)) || (tail && (r = msm_rows_dev_plan(ctx, m, tail, &pl_tail))) || (r = io.send(c, back)))
    return r;
  uint8_t *W = SC + a_w, *PRE = SC + a_pre, *ROWS = c + o_in;
  // the rows' statuses: the folding kernel with all-zero weights (its sums are not read)
  HIPCHK(hipMemsetAsync(W, 0, n * 32, s));
  LAUNCHCHK(nbls_g16_input_sums_launch((unsigned)n, (unsigned)m, ROWS, W, nullptr, SC + a_part, SC + a_S, PRE, s));
  LAUNCHCHK(nbls_g16_rows_launch((unsigned)n, (unsigned)m, PRE, ROWS, s));
  for (size_t b0 = 0; b0 < n; b0 += per) {
    const size_t cnt = std::min(per, n - b0);
    if ((r = g16_l_points(ctx, vk, cnt == per ? pl_full : pl_tail, cnt, ROWS + b0 * m * 32, IT, a, s)) || (r = run(ctx, P_G1_COMPRESS, cnt, {B(0, IT + a.l, 96), B(2, O + b0 * 48, 48)}, s)))
      return r;
    LAUNCHCHK(nbls_g16_prepare_tail_launch((unsigned)cnt, IT + a.lz, PRE + b0, O + b0 * 48, O + n * 48 + b0, s));
  }
  return io.fetch_to(O, out48, n * 48, status, n);
}

struct G16In { const nbls_groth16_vk* vk; size_t n; const uint8_t *proofs, *inputs, *seed32; };

static int groth16_pipeline(nbls_ctx* ctx, const G16In& in, int* all_ok, int8_t* status) {
  const nbls_groth16_vk* vk = in.vk;
  const size_t n = in.n, m = vk->m, p = 3 * RAW, sums = (m + 1) * 32, back = back_bytes(n);
  uint8_t seed[32]; int r; bool more;
  if ((r = rlc_seed(in.seed32, seed))) return r;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  // the staged block: proofs | inputs | seed
  const size_t o_pf = io.bytes(in.proofs, n * 192), o_in = io.bytes(in.inputs, n * m * 32), o_seed = io.bytes(seed, 32);
  size_t sz_pt = 0, sz_sc = 0, sz_pr = 0;
  const size_t a_ac = carve(&sz_pt, 2 * n * 48), a_bc = carve(&sz_pt, n * 96), a_aff = carve(&sz_pt, 2 * n * 96), a_b = carve(&sz_pt, n * 192), a_dst = carve(&sz_pt, 3 * n), a_pj = carve(&sz_pt, n * p),
               a_nn = carve(&sz_pt, n * RAW), a_ni = carve(&sz_pt, n * RAW), a_ra = carve(&sz_pt, n * 96), a_rst = carve(&sz_pt, n);
  const size_t a_w = carve(&sz_sc, n * 32), a_s1 = carve(&sz_sc, n * 32), a_part = carve(&sz_sc, (size_t)g16_workgroups((uint32_t)n) * sums), a_S = carve(&sz_sc, sums), a_pre0 = carve(&sz_sc, n);
  const size_t a_pt3 = carve(&sz_pr, 3 * 96), a_res = carve(&sz_pr, 576);
  uint8_t *c, *PTS, *SC, *PR, *BK; const uint8_t* got;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_G16_POINTS, sz_pt, &PTS)) || (r = need(ctx, SB_G16_SCALARS, sz_sc, &SC)) || (r = need(ctx, SB_G16_PAIRS, sz_pr, &PR)) ||
      (r = need(ctx, SB_G16_OUT, back, &BK)) || (r = ensure_scratch(ctx, n + 3)) || (r = io.send(c, back)))
    return r;
  uint8_t *AC = PTS + a_ac, *BC = PTS + a_bc, *A = PTS + a_aff, *C = A + n * 96, *B2 = PTS + a_b, *DST = PTS + a_dst, *PJ = PTS + a_pj, *NN = PTS + a_nn, *NI = PTS + a_ni, *RA = PTS + a_ra, *RST = PTS + a_rst;
  uint8_t *W = SC + a_w, *S1 = SC + a_s1, *S = SC + a_S, *PRE0 = SC + a_pre0, *PT3 = PR + a_pt3, *RES = PR + a_res, *PRE = hdr_pre(BK), *ROWS = c + o_in;
  HIPCHK(hipMemsetAsync(BK, 0, HDR_BYTES, s));
  LAUNCHCHK(nbls_g16_split_launch((unsigned)n, c + o_pf, AC, BC, s));
  LAUNCHCHK(nbls_rlc_weights_launch((unsigned)n, c + o_seed, W, s));
  // PointG1.fromHex of A_0 .. A_(n-1), C_0 .. C_(n-1); PointG2.fromSignature of the B_i
  if ((r = dev_decompress(ctx, false, 2 * n, AC, A, DST, s)) || (r = dev_decompress(ctx, true, n, BC, B2, DST + 2 * n, s))) return r;
  LAUNCHCHK(nbls_g16_pre_launch((unsigned)n, DST, DST + 2 * n, DST + n, PRE0, s));
  LAUNCHCHK(nbls_g16_input_sums_launch((unsigned)n, (unsigned)m, ROWS, W, PRE0, SC + a_part, S, PRE, s));
  LAUNCHCHK(nbls_g16_items_launch((unsigned)n, PRE, W, ctx->gen_g1, vk->g2neg, A, C, B2, S1, s));
  // [r_i]A_i, affine (never the zero point: A_i is a point of the subgroup other than zero, 2^63 <= r_i < 2^64)
  if ((r = run(ctx, P_G1_MUL64, n, {B(0, A, 96), B(2, W, 32), B(3, PJ, p), B(4, NN, RAW)}, s)) || (r = to_affine(ctx, false, n, PJ, NN, NI, RA, RST, s, false))) return r;
  // [S_0]alpha | sum_j [S_j]IC_j | sum_i [r_i]C_i: the partners of -beta, -gamma, -delta, each with its zero flag in the header
  if ((r = dev_msm(ctx, false, n, C, S1, 64, PT3 + 192, g16_hdr_c_zero(BK), s, MSM_RLC)) || (r = dev_msm(ctx, false, m + 1, vk->ic96, S, 256, PT3 + 96, g16_hdr_ic_zero(BK), s, MSM_RLC)) ||
      (r = dev_point_mul(ctx, false, 1, vk->alpha96, 0, S, PT3, g16_hdr_alpha_zero(BK), s)))
    return r;
  size_t mm = 0;
  if ((r = miller_values(ctx, n, RA, B2, &mm, s)) || (r = combined_tail(ctx, 3, mm, PT3, hdr_flags(BK), vk->tables, RES, hdr_one(BK), s)) || (r = io.fetch(BK, back, &got))) return r;
  combined_result(g16_verdict(got, n), n, all_ok, status, &more);
  if (!more) return NBLS_OK;
  // ---- the per-proof pass, chunk after chunk.  F: millerLoop(A_i, B_i) | the loops of L_i | of C_i, cnt each; behind the largest chunk's the one value of millerLoop(alpha, -beta)
  const size_t per = g16_chunk(ctx, n, m), tail = n % per;
  size_t sz_it = 0;
  const G16Rows a = g16_rows_carve(per, &sz_it);
  const size_t a_e = carve(&sz_it, per * 576), a_v = carve(&sz_it, per), a_fs = carve(&sz_it, n);
  MsmbPlan pl_full, pl_tail; uint8_t* IT;
  if ((r = need(ctx, SB_G16_ITEMS, sz_it, &IT)) || (r = ensure_scratch(ctx, 3 * per + 1)) || (r = msm_rows_dev_plan(ctx, m, per, &pl_full)) || (tail && (r = msm_rows_dev_plan(ctx, m, tail, &pl_tail))))
    return r;
  ForkGuard guard;   // (armed until statuses_back)
  uint8_t *L = IT + a.l, *LZ = IT + a.lz, *E = IT + a_e, *V = IT + a_v, *FS = IT + a_fs, *FAB = ctx->F + 3 * per * F12;
  LAUNCHCHK(nbls_g16_rows_launch((unsigned)n, (unsigned)m, PRE, ROWS, s));
  if ((r = run(ctx, P_ACC_Q, 1, {B(0, vk->alpha96, 96), B(3, vk->tables, LINE_BYTES), B(5, FAB, F12)}, s))) return r;
  for (size_t b0 = 0; b0 < n; b0 += per) {
    const size_t cnt = std::min(per, n - b0);
    uint8_t *F0 = ctx->F, *F1 = F0 + cnt * F12, *F2 = F1 + cnt * F12;
    if ((r = g16_l_points(ctx, vk, cnt == per ? pl_full : pl_tail, cnt, ROWS + b0 * m * 32, IT, a, s))) return r;
    LAUNCHCHK(nbls_agg_fix_zero_launch((unsigned)cnt, LZ, ctx->gen_g1, L, nullptr, s));
    if ((r = run(ctx, ls_variant(ctx, P_MILLER_RAW, cnt), cnt, {B(0, A + b0 * 96, 96), B(1, B2 + b0 * 192, 192), B(3, F0, F12)}, s)) ||
        (r = run(ctx, P_ACC_Q, cnt, {B(0, L, 96), B(3, vk->tables + LINE_BYTES, 0), B(5, F1, F12)}, s)) ||
        (r = run(ctx, P_ACC_Q, cnt, {B(0, C + b0 * 96, 96), B(3, vk->tables + 2 * LINE_BYTES, 0), B(5, F2, F12)}, s)))
      return r;
    LAUNCHCHK(nbls_agg_points_launch(cnt, (unsigned)F12, nullptr, LZ, ctx->one12, F1, F1, s));   // a zero L_i: the factor one
    if ((r = run(ctx, P_MUL2S, cnt, {B(3, F0, F12), B(4, F1, F12), B(5, F0, F12)}, s)) || (r = run(ctx, P_MUL2S, cnt, {B(3, F0, F12), B(4, F2, F12), B(5, F0, F12)}, s)) ||
        (r = run(ctx, P_MUL2S, cnt, {B(3, F0, F12), B(4, FAB, 0), B(5, F0, F12)}, s)) || (r = items_is_one(ctx, cnt, E, V, s)))
      return r;
    LAUNCHCHK(nbls_g16_status_launch((unsigned)cnt, PRE + b0, V, FS + b0, s));
  }
  return statuses_back(ctx, s, FS, n, guard, all_ok, status);
}

EXPORT int nbls_groth16_verify(nbls_ctx* ctx, const nbls_groth16_vk* vk, size_t n, const uint8_t* proofs192, const uint8_t* inputs32, const uint8_t* seed32, int* all_ok, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !vk || !n || !proofs192 || !inputs32 || !all_ok || vk->device != ctx->device || n > G16_MAX_PROOFS || n * vk->m > G16_MAX_ELEMS) return NBLS_EINVAL;
  return groth16_pipeline(ctx, {vk, n, proofs192, inputs32, seed32}, all_ok, status);
}
