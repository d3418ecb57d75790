// pipelines_kzg_verify_cells.cpp -- the verifier's side of PeerDAS (EIP-7594, polynomial-commitments-sampling.md: verify_cell_kzg_proof_batch) against the monomial basis kept on
// the device (nbls_kzg_monomial).  With N elements per blob, c = 2^log2_cell per cell, g = omega_2N: cell k of a blob with polynomial p holds v_j = p(h_k omega_c^rev(j)),
// h_k = g^rev(k); I_k, of degree < c, interpolates it; s_k = h_k^c = entry k of the table of the 2 N / c roots.  The cell holds with proof pi_k and commitment C exactly when
//   e(pi_k, [tau^c]G2) = e(C - [I_k(tau)]G1 + [s_k]pi_k, G2).
// n cells are checked together with the secret weights r_k of nbls_verify_multiple (rlc_weights.h), indexed by the cell's position in the call:
//   e(A, [tau^c]G2) * e(B, -G2) = 1,   A = sum_k [r_k]pi_k,   B = sum_k [r_k]C_ci[k] - sum_(i<c) [S_i][tau^i]G1 + sum_k [r_k s_k]pi_k,   S_i = sum_k r_k a_(k,i) mod r
// (the sign on the fixed G2 point, as in kzg_pipeline).  This is the specification's verify_cell_kzg_proof_batch_impl with secret weights in place of its Fiat-Shamir powers,
// the choice nbls_kzg_verify_proofs made before.  One chain on the context's stream:
//   H2D copy -> [tau^c]G2: PointG2.fromSignature; its line table and -G2's (P_LINES_Q) -> weights -> dev_decompress of the n_commitments + n_cells G1 points (every commitment once)
//            -> kzg_cell_pre_kernel: what the decoders say about every cell -> kzg_cell_interp_kernel in its sum mode: the canonical check, the interpolation of every cell in
//               the registers of c lanes, weighted and summed; kzg_cell_sum_kernel: the c scalars -S_i.  No coefficient of a cell goes to memory
//            -> kzg_cell_items_kernel: the scalars, the commitment of every cell gathered
//            -> A: the 64-bit MSM over the proofs; B: a 64-bit MSM over the gathered commitments + a 256-bit MSM over the proofs + msm_rows_dev with ONE row of c scalars against
//               the handle's first c points, joined by two complete additions -> two Miller loops -> product -> final exponentiation -> compared with one (kzg_combined_tail)
//            -> D2H copy; acceptance by kzg_pipeline's rule (A = B = O accepts, exactly one of them zero rejects)
// Where the combined check does not accept and the caller asked for statuses, the per-cell pass judges every cell with the equation above: the kernel's rows mode writes
// -a_(k,.) into the rows of msm_rows_dev (n rows of c points), one ladder for [s_k]pi_k, the gathered C, and kzg_item_tail.
// Scratch slots: SB_STAGED and SB_KZGV_* (nbls_internal.h, M_KZGV_OWN); the decoder and the ladder run on the main slots, the MSMs on MSM_RLC's, the batched MSM on SB_MSMB_*.
#include "nbls_internal.h"
#include "fr_exec.h"
#include <algorithm>

static const size_t KZGV_MAX_CELLS = (size_t)1 << 20, KZGV_MAX_SCALARS = (size_t)1 << 22;   // one pass of the batched MSM, which the per-cell pass needs: rows, scalars
static const size_t KZGV_MAX_COMMITMENTS = (size_t)1 << 22;

static size_t carve(size_t* off, size_t bytes) { const size_t o = *off; *off = o + ((bytes + 63) & ~(size_t)63); return o; }

// the table of the 2 N / c inverse shifts of (log2_n, log2_cell): made on first use, freed with the context
static int cell_ishifts(nbls_ctx* ctx, unsigned log2_n, unsigned log2_cell, hipStream_t s, const uint8_t** table) {
  uint8_t*& slot = ctx->kzg_cell_ishifts[log2_n][log2_cell];
  if (!slot) {
    const unsigned lm = log2_n + 1 - log2_cell;
    uint8_t* t = nullptr;
    HIPCHK(hipMalloc(&t, (size_t)32 << lm));
    const int e = nbls_kzg_cell_ishifts_launch(log2_n, lm, t, s);
    if (e) { hipFree(t); ctx->last_hip = e; return NBLS_EHIP; }
    slot = t;
  }
  *table = slot;
  return NBLS_OK;
}

struct VerifyCellsIn {
  const nbls_kzg_monomial* mono; unsigned log2_cell; size_t n_commitments; const uint8_t* c48; size_t n; const uint32_t *ci, *cell_index; const uint8_t *cells, *p48, *tau96, *seed32;
};

static int verify_cells_pipeline(nbls_ctx* ctx, const VerifyCellsIn& in, int* all_ok, int8_t* status) {
  const unsigned L = in.mono->log2_n, lc = in.log2_cell, lm = L + 1 - lc;
  const size_t n = in.n, nc = in.n_commitments, cc = (size_t)1 << lc, p = 3 * RAW;
  uint8_t seed[32];
  if (in.seed32) memcpy(seed, in.seed32, 32);
  else { const int e = os_seed(seed); if (e) return e; }
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  // the staged block: commitments | proofs (one array of compressed points) | the two index arrays | cells | [tau^c]G2 | -G2 | seed
  const size_t o_cp = io.bytes(in.c48, nc * 48), o_pf = io.bytes(in.p48, n * 48), o_ci = io.bytes(in.ci, n * 4), o_ki = io.bytes(in.cell_index, n * 4), o_cells = io.bytes(in.cells, n * cc * 32),
               o_tau = io.bytes(in.tau96, 96), o_ng2 = io.bytes(neg_g2_wire(), 192), o_seed = io.bytes(seed, 32);
  if (o_pf != o_cp + nc * 48) return NBLS_EINVAL;   // (48 is a multiple of the parts' alignment)
  const size_t parts = fr_cell_workgroups((uint32_t)n, lc, true);
  size_t sz_pt = 0, sz_sc = 0, sz_pr = 0;
  const size_t a_aff = carve(&sz_pt, (nc + n) * 96), a_gath = carve(&sz_pt, n * 96), a_dst = carve(&sz_pt, nc + n), a_gst = carve(&sz_pt, n);
  const size_t a_w = carve(&sz_sc, n * 32), a_s1 = carve(&sz_sc, n * 32), a_s2 = carve(&sz_sc, n * 32), a_s3 = carve(&sz_sc, n * 32), a_zs = carve(&sz_sc, n * 32),
               a_part = carve(&sz_sc, parts * cc * 32), a_srow = carve(&sz_sc, cc * 32), a_pre0 = carve(&sz_sc, n);
  const size_t a_g2 = carve(&sz_pr, 2 * 192), a_tb = carve(&sz_pr, 2 * LINE_BYTES), a_pt2 = carve(&sz_pr, 2 * 96), a_res = carve(&sz_pr, 576), a_b3 = carve(&sz_pr, 3 * 96), a_bst = carve(&sz_pr, 3),
               a_bj = carve(&sz_pr, 3 * p), a_bn = carve(&sz_pr, 2 * RAW);
  // what is read back: the product is one | A is the zero point | B is | the decoder status of [tau^c]G2 | (12 unused) | the n statuses before any pairing
  const size_t back = 16 + n;
  MsmbPlan pl_one;
  uint8_t *c, *PTS, *SC, *PR, *BK; const uint8_t *sroots, *iroots = nullptr, *ishifts, *got; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGV_POINTS, sz_pt, &PTS)) || (r = need(ctx, SB_KZGV_SCALARS, sz_sc, &SC)) || (r = need(ctx, SB_KZGV_PAIRS, sz_pr, &PR)) ||
      (r = need(ctx, SB_KZGV_OUT, back, &BK)) || (r = ensure_scratch(ctx, 2)) || (r = msm_rows_dev_plan(ctx, cc, 1, &pl_one)) || (r = kzg_roots(ctx, lm, s, &sroots)) ||
      (lc && (r = kzg_inv_roots(ctx, lc, s, &iroots))) || (r = cell_ishifts(ctx, L, lc, s, &ishifts)) || (r = io.send(c, back)))
    return r;
  uint8_t *AFF = PTS + a_aff, *PF = AFF + nc * 96, *GATH = PTS + a_gath, *DST = PTS + a_dst, *GST = PTS + a_gst;
  uint8_t *W = SC + a_w, *S1 = SC + a_s1, *S2 = SC + a_s2, *S3 = SC + a_s3, *ZS = SC + a_zs, *PART = SC + a_part, *SROW = SC + a_srow, *PRE0 = SC + a_pre0;
  uint8_t *G2P = PR + a_g2, *TB = PR + a_tb, *PT2 = PR + a_pt2, *RES = PR + a_res, *PRE = BK + 16, *B3 = PR + a_b3, *BST = PR + a_bst, *BJ = PR + a_bj, *BN = PR + a_bn;
  const uint32_t *d_ci = (const uint32_t*)(c + o_ci), *d_ki = (const uint32_t*)(c + o_ki);
  HIPCHK(hipMemsetAsync(BK, 0, 16, s));
  // [tau^c]G2 by PointG2.fromSignature's rules (its status is judged after the read-back: nothing is decided on the host before), then the two line tables
  if ((r = dev_decompress(ctx, true, 1, c + o_tau, G2P, BK + 3, s))) return r;
  HIPCHK(hipMemcpyAsync(G2P + 192, c + o_ng2, 192, hipMemcpyDeviceToDevice, s));
  if ((r = run(ctx, P_LINES_Q, 2, {B(1, G2P, 192), B(3, TB, LINE_BYTES)}, s))) return r;
  LAUNCHCHK(nbls_rlc_weights_launch((unsigned)n, c + o_seed, W, s));
  if ((r = dev_decompress(ctx, false, nc + n, c + o_cp, AFF, DST, s))) return r;
  LAUNCHCHK(nbls_kzg_cell_pre_launch((unsigned)n, DST, DST + nc, d_ci, PRE0, s));
  LAUNCHCHK(nbls_kzg_cell_interp_launch(lc, (unsigned)n, 1, c + o_cells, d_ki, PRE0, W, iroots, ishifts, nullptr, PART, SROW, PRE, s));
  LAUNCHCHK(nbls_kzg_cell_items_launch((unsigned)n, DST, DST + nc, d_ci, d_ki, PRE, W, sroots, ctx->gen_g1, AFF, PF, GATH, GST, S1, S2, S3, ZS, s));
  if ((r = dev_msm(ctx, false, n, PF, S1, 64, PT2, BK + 1, s, MSM_RLC))) return r;
  // B = sum_k [r_k]C_ci[k] | sum_k [r_k s_k]pi_k | -sum_i [S_i][tau^i]G1: affine points with a status each (1 = the zero point), joined by kzg_combined_tail
  if ((r = dev_msm(ctx, false, n, GATH, S2, 64, B3, BST, s, MSM_RLC)) || (r = dev_msm(ctx, false, n, PF, S3, 256, B3 + 96, BST + 1, s, MSM_RLC)) ||
      (r = msm_rows_dev(ctx, pl_one, in.mono->pts, SROW, B3 + 192, BST + 2, s)) || (r = kzg_combined_tail(ctx, {B3, BST, BJ, BN, PT2, TB, RES, BK}, s)))
    return r;
  if ((r = io.fetch(BK, back, &got))) return r;
  if (got[3] != 0) return NBLS_EDECODE;   // [tau^c]G2 does not decode, or is the zero point
  const bool one = got[0] != 0, za = got[1] == 1, zb = got[2] == 1;
  bool clean = true;
  for (size_t i = 0; i < n && clean; i++) clean = got[16 + i] == 0;
  if (clean && ((za && zb) || (!za && !zb && one))) {
    *all_ok = 1;
    if (status) memset(status, 0, n);
    return NBLS_OK;
  }
  *all_ok = 0;
  if (!status) return NBLS_OK;   // fast reject: no per-cell work
  // ---- the per-cell pass: X_k = -[I_k(tau)]G1 | [s_k]pi_k | C_ci[k]
  size_t sz_it = 0;
  KzgItemTail t;
  const size_t b_rows = carve(&sz_it, n * cc * 32), b_t = kzg_item_tail_carve(n, &sz_it, &t);
  MsmbPlan pl_rows;
  uint8_t* IT;
  if ((r = need(ctx, SB_KZGV_ITEMS, sz_it, &IT)) || (r = ensure_scratch(ctx, 2 * n)) || (r = msm_rows_dev_plan(ctx, cc, n, &pl_rows))) return r;
  uint8_t *ROWS = IT + b_rows, *P3 = IT + b_t + t.p3, *ST3 = IT + b_t + t.st3, *FS = IT + b_t + t.fs;
  ForkGuard guard;   // nothing is forked here: the guard is used for its wait alone, as in kzg_pipeline
  LAUNCHCHK(nbls_kzg_cell_interp_launch(lc, (unsigned)n, 0, c + o_cells, d_ki, PRE, nullptr, iroots, ishifts, ROWS, nullptr, nullptr, nullptr, s));
  if ((r = msm_rows_dev(ctx, pl_rows, in.mono->pts, ROWS, P3, ST3, s)) || (r = dev_point_mul(ctx, false, n, PF, 96, ZS, P3 + n * 96, ST3 + n, s))) return r;
  HIPCHK(hipMemcpyAsync(P3 + 2 * n * 96, GATH, n * 96, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(ST3 + 2 * n, GST, n, hipMemcpyDeviceToDevice, s));
  if ((r = kzg_item_tail(ctx, n, t, IT + b_t, PF, TB, PRE, DST + nc, s)) || (r = read_back(ctx, s, FS, n, &got))) return r;
  guard.armed = false;
  memcpy(status, got, n);
  int all = 1;
  for (size_t i = 0; i < n; i++) if (got[i]) all = 0;
  *all_ok = all;
  return NBLS_OK;
}

EXPORT int nbls_kzg_verify_cells(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n_commitments, const uint8_t* commitments48, size_t n_cells,
                                 const uint32_t* commitment_index, const uint32_t* cell_index, const uint8_t* cells, const uint8_t* proofs48, const uint8_t* tau_c_g2_96,
                                 const uint8_t* seed32, int* all_ok, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !monomial || !commitments48 || !commitment_index || !cell_index || !cells || !proofs48 || !tau_c_g2_96 || !all_ok || !n_cells || !n_commitments ||
      monomial->device != ctx->device || log2_cell > 6 || log2_cell > monomial->log2_n || monomial->log2_n + 1 - log2_cell > 12 || n_cells > KZGV_MAX_CELLS ||
      (n_cells << log2_cell) > KZGV_MAX_SCALARS || n_commitments > KZGV_MAX_COMMITMENTS)
    return NBLS_EINVAL;
  const size_t M = (size_t)2 << (monomial->log2_n - log2_cell);
  for (size_t k = 0; k < n_cells; k++) if (cell_index[k] >= M || commitment_index[k] >= n_commitments) return NBLS_EINVAL;
  return verify_cells_pipeline(ctx, {monomial, log2_cell, n_commitments, commitments48, n_cells, commitment_index, cell_index, cells, proofs48, tau_c_g2_96, seed32}, all_ok, status);
}
