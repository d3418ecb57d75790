// pipelines_kzg_cells.cpp -- the transform between the two forms of a polynomial over Fr (nbls_fr_ntt) and what PeerDAS (EIP-7594, polynomial-commitments-sampling.md) builds on
// it: compute_cells and compute_cells_and_kzg_proofs for many blobs, against the monomial basis [tau^i]G1 kept on the device (nbls_kzg_monomial).  With N = 2^log2_n elements
// per blob, c = 2^log2_cell per cell, g = omega_2N and p the blob's polynomial:
//   the extension in bit-reversed order over 2 N is   ext[i] = blob[i],  ext[N + i] = p(g w_i)   -- one coset evaluation of size N, never a transform of size 2 N;
//   cell k = ext[c k .. c k + c), its points h_k omega_c^rev(j) with h_k = g^rev(k), its vanishing polynomial X^c - s_k with s_k = h_k^c = entry k of the table of 2 N / c roots;
//   its proof = sum_i [q_i] [tau^i]G1 for the floor quotient q of p by X^c - s_k in coefficient form.
// One chain on the context's stream:
//   H2D copy -> kzg_ntt_kernel in its cells mode: the canonical check, the blob's bytes, the coefficients (kept in device memory for the proofs), the coset values
//            -> proofs, chunk after chunk of whole blobs (the batched MSM takes 2^22 scalars and 2^20 rows a pass: 8 mainnet blobs): kzg_cell_rows_kernel writes the 2 N / c
//               quotient rows of every blob as big-endian scalars -> kzg_proof_tail (kzg_common.cpp): msm_rows_dev against the converted basis -> P_G1_COMPRESS ->
//               kzg_prove_tail_kernel.  The handle nbls_kzg_monomial and the tables of roots are kzg_common.cpp's as well
//            -> D2H copy: cells | proofs | statuses
// Scratch slots: SB_STAGED and SB_KZGC_* (nbls_internal.h, M_KZGC_OWN); the MSM on SB_MSMB_*.
#include "nbls_internal.h"
// (fr_omega runs on the host here: its exponent's shift asks for an unrolling that the host pass declines, which is all the warning says)
#pragma clang diagnostic ignored "-Wpass-failed"
#include "fr_exec.h"
#include <algorithm>

EXPORT int nbls_fr_ntt(nbls_ctx* ctx, unsigned log2_n, int dir, size_t n, const uint8_t* in32, const uint8_t* shift32, uint8_t* out32, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > 12 || (dir != NBLS_NTT_TO_COEFFS && dir != NBLS_NTT_TO_EVALS) || (n && (!in32 || !out32)) || n > (KZG_MAX_ELEMS >> log2_n)) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t qb = (n * 32) << log2_n, o_in = io.bytes(in32, qb), o_sh = io.bytes(shift32, shift32 ? n * 32 : 0), back = qb + n;
  uint8_t *c, *O; const uint8_t *roots, *iroots; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGC_OUT, back, &O)) || (r = kzg_table(ctx, KZG_ROOTS, log2_n, 0, s, &roots)) || (r = kzg_table(ctx, KZG_INV_ROOTS, log2_n, 0, s, &iroots)) ||
      (r = io.send(c, back)))
    return r;
  LAUNCHCHK(nbls_kzg_ntt_launch(log2_n, dir == NBLS_NTT_TO_COEFFS ? FR_NTT_TO_COEFFS : FR_NTT_TO_EVALS, (unsigned)n, c + o_in, shift32 ? c + o_sh : nullptr, 32, roots, iroots, O, nullptr,
                                O + qb, s));
  return io.fetch_to(O, out32, qb, status, n);
}

// mono == NULL: nbls_kzg_compute_cells (out_proofs unused)
struct CellsIn { unsigned log2_n, log2_cell; size_t n; const uint8_t* blobs; const nbls_kzg_monomial* mono; uint8_t *out_cells, *out_proofs; };

static int cells_pipeline(nbls_ctx* ctx, const CellsIn& in, int8_t* status) {
  const unsigned L = in.log2_n, lc = in.log2_cell;
  const size_t n = in.n, N = (size_t)1 << L, M = (2 * N) >> lc, qb = n * N * 32;   // M: the cells, and the quotient rows, of one blob
  const bool proofs = in.mono != nullptr;
  uint8_t g32[32];
  fr_to_bytes(fr_omega(L + 1), g32);   // g = omega_2N, the shift of the coset
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_blob = io.bytes(in.blobs, qb), o_g = io.bytes(g32, 32);
  // blobs per pass: as many whole blobs as the batched MSM takes, or fewer where the tuning key says so
  size_t per = proofs ? std::min({n, (MSMB_MAX_ITEMS >> L) / M, MSMB_MAX_GROUPS / M}) : n;
  if (proofs && ctx->cells_chunk && ctx->cells_chunk < per) per = ctx->cells_chunk;
  const size_t tail = n % per;
  // what is read back: the cells | the compressed proofs | the blobs' statuses; behind it one pass's affine sums, zero flags and closing statuses
  const size_t b_pf = 2 * qb, b_st = b_pf + (proofs ? n * M * 48 : 0), back = b_st + n;
  size_t sz_out = 0, sz_rows = 0;
  const size_t a_bk = carve(&sz_out, back), a_aff = carve(&sz_out, proofs ? per * M * 96 : 0), a_zf = carve(&sz_out, proofs ? per * M : 0), a_cst = carve(&sz_out, proofs ? per * M : 0);
  const size_t a_q = carve(&sz_rows, proofs ? per * M * N * 32 : 0), a_rst = carve(&sz_rows, proofs ? per * M : 0);
  MsmbPlan pl_full, pl_tail;   // (the larger plan first: the smaller then finds both of the MSM's slots large enough and takes the same pointers)
  uint8_t *c, *OUT, *COEF = nullptr, *ROWS = nullptr; const uint8_t *roots, *iroots, *sroots = nullptr, *got; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGC_OUT, sz_out, &OUT)) || (proofs && (r = need(ctx, SB_KZGC_COEFS, qb, &COEF))) ||
      (proofs && (r = need(ctx, SB_KZGC_ROWS, sz_rows, &ROWS))) || (proofs && (r = msm_rows_dev_plan(ctx, N, per * M, &pl_full))) ||
      (proofs && tail && (r = msm_rows_dev_plan(ctx, N, tail * M, &pl_tail))) || (r = kzg_table(ctx, KZG_ROOTS, L, 0, s, &roots)) || (r = kzg_table(ctx, KZG_INV_ROOTS, L, 0, s, &iroots)) ||
      (proofs && (r = kzg_table(ctx, KZG_ROOTS, L + 1 - lc, 0, s, &sroots))) || (r = io.send(c, back)))
    return r;
  uint8_t *BK = OUT + a_bk, *AFF = OUT + a_aff, *ZF = OUT + a_zf, *CST = OUT + a_cst, *Q = ROWS + a_q, *RST = ROWS + a_rst;
  LAUNCHCHK(nbls_kzg_ntt_launch(L, FR_NTT_CELLS, (unsigned)n, c + o_blob, c + o_g, 0, roots, iroots, BK, COEF, BK + b_st, s));
  for (size_t b0 = 0; proofs && b0 < n; b0 += per) {
    const size_t nb = std::min(per, n - b0);
    uint8_t* P = BK + b_pf + b0 * M * 48;
    LAUNCHCHK(nbls_kzg_cell_rows_launch(L, lc, (unsigned)nb, COEF + b0 * N * 32, sroots, BK + b_st + b0, Q, RST, s));
    if ((r = kzg_proof_tail(ctx, nb == per ? pl_full : pl_tail, in.mono->pts, Q, AFF, ZF, RST, nullptr, P, CST, s))) return r;
  }
  if ((r = io.fetch(BK, back, &got))) return r;
  memcpy(in.out_cells, got, 2 * qb);
  if (proofs) memcpy(in.out_proofs, got + b_pf, n * M * 48);
  if (status) memcpy(status, got + b_st, n);
  return NBLS_OK;
}

EXPORT int nbls_kzg_compute_cells(nbls_ctx* ctx, unsigned log2_n, unsigned log2_cell, size_t n, const uint8_t* blobs, uint8_t* out_cells, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > 12 || log2_cell > log2_n || (n && (!blobs || !out_cells)) || n > (KZG_MAX_ELEMS >> log2_n)) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  return cells_pipeline(ctx, {log2_n, log2_cell, n, blobs, nullptr, out_cells, nullptr}, status);
}

EXPORT int nbls_kzg_compute_cells_and_proofs(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n, const uint8_t* blobs, uint8_t* out_cells,
                                             uint8_t* out_proofs48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !monomial || !blobs || !out_cells || !out_proofs48 || !n || monomial->device != ctx->device || log2_cell > monomial->log2_n) return NBLS_EINVAL;
  const unsigned L = monomial->log2_n;
  // one blob alone must fit a pass of the batched MSM: (2 N / c) rows of N scalars
  if (((size_t)2 << (2 * L - log2_cell)) > MSMB_MAX_ITEMS || n > (KZG_MAX_ELEMS >> L)) return NBLS_EINVAL;
  return cells_pipeline(ctx, {L, log2_cell, n, blobs, monomial, out_cells, out_proofs48}, status);
}
