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
//               the handle's first c points, joined by two complete additions -> two Miller loops -> product -> final exponentiation -> compared with one (KzgFrame::decide)
//            -> D2H copy; acceptance by the frame's rule, which kzg_pipeline shares (verifier_frame.h: A = B = O accepts, exactly one of them zero rejects)
// Where the combined check does not accept and the caller asked for statuses, the per-cell pass judges every cell with the equation above: the kernel's rows mode writes
// -a_(k,.) into the rows of msm_rows_dev (n rows of c points), one ladder for [s_k]pi_k, the gathered C, and the frame's per-item tail (KzgFrame::items_close).
// Scratch slots: SB_STAGED and SB_KZGV_* (nbls_internal.h, M_KZGV_OWN); the decoder and the ladder run on the main slots, the MSMs on MSM_RLC's, the batched MSM on SB_MSMB_*.
#include "nbls_internal.h"
#include "fr_exec.h"
#include <algorithm>

static const size_t KZGV_MAX_COMMITMENTS = (size_t)1 << 22;

struct VerifyCellsIn {
  const nbls_kzg_monomial* mono; unsigned log2_cell; size_t n_commitments; const uint8_t* c48; size_t n; const uint32_t *ci, *cell_index; const uint8_t *cells, *p48, *tau96, *seed32;
};

static int verify_cells_pipeline(nbls_ctx* ctx, const VerifyCellsIn& in, int* all_ok, int8_t* status) {
  const unsigned L = in.mono->log2_n, lc = in.log2_cell, lm = L + 1 - lc;
  const size_t n = in.n, nc = in.n_commitments, cc = (size_t)1 << lc;
  uint8_t seed[32]; int r; bool more;
  if ((r = rlc_seed(in.seed32, seed))) return r;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  KzgFrame fr(ctx, io, s, n, SB_KZGV_PAIRS, SB_KZGV_OUT, SB_KZGV_ITEMS);
  // the staged block: commitments | proofs (one array of compressed points) | the two index arrays | cells | [tau^c]G2 | -G2 | seed
  const size_t o_cp = io.bytes(in.c48, nc * 48), o_pf = io.bytes(in.p48, n * 48), o_ci = io.bytes(in.ci, n * 4), o_ki = io.bytes(in.cell_index, n * 4), o_cells = io.bytes(in.cells, n * cc * 32);
  fr.stage(in.tau96, seed);
  if (o_pf != o_cp + nc * 48) return NBLS_EINVAL;   // (48 is a multiple of the parts' alignment)
  const size_t parts = fr_cell_workgroups((uint32_t)n, lc, true);
  size_t sz_pt = 0, sz_sc = 0;
  const size_t a_aff = carve(&sz_pt, (nc + n) * 96), a_gath = carve(&sz_pt, n * 96), a_dst = carve(&sz_pt, nc + n), a_gst = carve(&sz_pt, n);
  const size_t a_w = carve(&sz_sc, n * 32), a_s1 = carve(&sz_sc, n * 32), a_s2 = carve(&sz_sc, n * 32), a_s3 = carve(&sz_sc, n * 32), a_zs = carve(&sz_sc, n * 32),
               a_part = carve(&sz_sc, parts * cc * 32), a_srow = carve(&sz_sc, cc * 32), a_pre0 = carve(&sz_sc, n);
  MsmbPlan pl_one, pl_rows;
  uint8_t *c, *PTS, *SC, *ROWS; const uint8_t *sroots, *iroots = nullptr, *ishifts;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGV_POINTS, sz_pt, &PTS)) || (r = need(ctx, SB_KZGV_SCALARS, sz_sc, &SC)) || (r = fr.take()) ||
      (r = msm_rows_dev_plan(ctx, cc, 1, &pl_one)) || (r = kzg_table(ctx, KZG_ROOTS, lm, 0, s, &sroots)) || (lc && (r = kzg_table(ctx, KZG_INV_ROOTS, lc, 0, s, &iroots))) ||
      (r = kzg_table(ctx, KZG_CELL_ISHIFTS, L, lc, s, &ishifts)) || (r = io.send(c, back_bytes(n))))
    return r;
  uint8_t *AFF = PTS + a_aff, *PF = AFF + nc * 96, *GATH = PTS + a_gath, *DST = PTS + a_dst, *GST = PTS + a_gst;
  uint8_t *W = SC + a_w, *S1 = SC + a_s1, *S2 = SC + a_s2, *S3 = SC + a_s3, *ZS = SC + a_zs, *PART = SC + a_part, *SROW = SC + a_srow, *PRE0 = SC + a_pre0;
  const uint32_t *d_ci = (const uint32_t*)(c + o_ci), *d_ki = (const uint32_t*)(c + o_ki);
  if ((r = fr.open(c, W)) || (r = dev_decompress(ctx, false, nc + n, c + o_cp, AFF, DST, s))) return r;
  LAUNCHCHK(nbls_kzg_cell_pre_launch((unsigned)n, DST, DST + nc, d_ci, PRE0, s));
  LAUNCHCHK(nbls_kzg_cell_interp_launch(lc, (unsigned)n, 1, c + o_cells, d_ki, PRE0, W, iroots, ishifts, nullptr, PART, SROW, fr.PRE, s));
  LAUNCHCHK(nbls_kzg_cell_items_launch((unsigned)n, DST, DST + nc, d_ci, d_ki, fr.PRE, W, sroots, ctx->gen_g1, AFF, PF, GATH, GST, S1, S2, S3, ZS, s));
  if ((r = dev_msm(ctx, false, n, PF, S1, 64, fr.PT2, fr.A_ZERO, s, MSM_RLC))) return r;
  // B = sum_k [r_k]C_ci[k] | sum_k [r_k s_k]pi_k | -sum_i [S_i][tau^i]G1: affine points with a status each (1 = the zero point), joined by the frame's combined check
  if ((r = dev_msm(ctx, false, n, GATH, S2, 64, fr.B3, fr.BST, s, MSM_RLC)) || (r = dev_msm(ctx, false, n, PF, S3, 256, fr.B3 + 96, fr.BST + 1, s, MSM_RLC)) ||
      (r = msm_rows_dev(ctx, pl_one, in.mono->pts, SROW, fr.B3 + 192, fr.BST + 2, s)) || (r = fr.decide(all_ok, status, &more)) || !more)
    return r;
  // ---- the per-cell pass: X_k = -[I_k(tau)]G1 | [s_k]pi_k | C_ci[k]
  if ((r = fr.items_begin(n * cc * 32, &ROWS, &pl_rows, cc))) return r;
  uint8_t *P3 = fr.P3, *ST3 = fr.ST3;
  LAUNCHCHK(nbls_kzg_cell_interp_launch(lc, (unsigned)n, 0, c + o_cells, d_ki, fr.PRE, nullptr, iroots, ishifts, ROWS, nullptr, nullptr, nullptr, s));
  if ((r = msm_rows_dev(ctx, pl_rows, in.mono->pts, ROWS, P3, ST3, s)) || (r = dev_point_mul(ctx, false, n, PF, 96, ZS, P3 + n * 96, ST3 + n, s))) return r;
  HIPCHK(hipMemcpyAsync(P3 + 2 * n * 96, GATH, n * 96, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(ST3 + 2 * n, GST, n, hipMemcpyDeviceToDevice, s));
  return fr.items_close(PF, DST + nc, all_ok, status);
}

EXPORT int nbls_kzg_verify_cells(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n_commitments, const uint8_t* commitments48, size_t n_cells,
                                 const uint32_t* commitment_index, const uint32_t* cell_index, const uint8_t* cells, const uint8_t* proofs48, const uint8_t* tau_c_g2_96,
                                 const uint8_t* seed32, int* all_ok, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !monomial || !commitments48 || !commitment_index || !cell_index || !cells || !proofs48 || !tau_c_g2_96 || !all_ok || !n_cells || !n_commitments ||
      monomial->device != ctx->device || log2_cell > 6 || log2_cell > monomial->log2_n || monomial->log2_n + 1 - log2_cell > 12 || n_cells > MSMB_MAX_GROUPS ||
      (n_cells << log2_cell) > MSMB_MAX_ITEMS || n_commitments > KZGV_MAX_COMMITMENTS)   // (one pass of the batched MSM, which the per-cell pass needs: rows, scalars)
    return NBLS_EINVAL;
  const size_t M = (size_t)2 << (monomial->log2_n - log2_cell);
  for (size_t k = 0; k < n_cells; k++) if (cell_index[k] >= M || commitment_index[k] >= n_commitments) return NBLS_EINVAL;
  return verify_cells_pipeline(ctx, {monomial, log2_cell, n_commitments, commitments48, n_cells, commitment_index, cell_index, cells, proofs48, tau_c_g2_96, seed32}, all_ok, status);
}
