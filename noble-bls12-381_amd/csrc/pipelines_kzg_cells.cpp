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
// nbls_kzg_recover_cells / _and_proofs (recover_cells_and_kzg_proofs) are the same chain behind another front end: from at least half of every blob's cells to the same
// coefficients buffer, by size-N transforms only (fr_exec.h has the route), then the same proofs loop.
// The *_fk20 calls are the same chain again with another proofs loop (FK20; fr_exec.h has the identities, the handle nbls_kzg_fk20 is kzg_common.cpp's): per chunk of whole
// blobs (256 mainnet blobs) kzg_fk20_scalars_kernel writes the transforms of the coefficients' stripes as pass A's scalars -> msm_map_dev against the handle's points: M
// groups of c terms a blob, the sums left projective with their endomorphism images -> msm_map_dev with those sums as points and the handle's matrix as scalars: M groups of
// M terms a blob -> kzg_proof_close.  n' = N / c = 1: no pass, every proof of an accepted blob is the zero point.
// Scratch slots: SB_STAGED and SB_KZGC_* (nbls_internal.h, M_KZGC_OWN), the recovery's Z values on SB_KZGR_Z (M_KZGR_OWN), the FK20 loop's on SB_KZGF_* (M_KZGF_OWN); the MSM on SB_MSMB_*.
#include "nbls_internal.h"
// (fr_omega runs on the host here: its exponent's shift asks for an unrolling that the host pass declines, which is all the warning says)
#pragma clang diagnostic ignored "-Wpass-failed"
#include "fr_exec.h"
#include <algorithm>
#include <vector>

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

// ---- Transforms of up to 2^24 elements a polynomial (fr_exec.h has the split into global stages and tails).  The plan of a call: t = the tails' log size, P = the stages
// a launch runs at most, both the context's (NBLS_TUNE_NTT_TAIL_BITS / _PASS_BITS) or fr_exec.h's defaults
static unsigned ntt_tail_bits(const nbls_ctx* ctx) { return ctx->ntt_tail_bits ? ctx->ntt_tail_bits : FR_NTTL_DEFAULT_TAIL; }
// what both entry points refuse before any device work (the buffers are theirs to look at)
static bool ntt_large_args(const nbls_ctx* ctx, unsigned log2_n, int dir, size_t n) {
  return ctx && log2_n >= 1 && log2_n <= FR_NTTL_MAX_LOG2 && (dir == NBLS_NTT_TO_COEFFS || dir == NBLS_NTT_TO_EVALS) && n <= (KZG_MAX_ELEMS >> log2_n) &&
         (log2_n <= ntt_tail_bits(ctx) || log2_n - ntt_tail_bits(ctx) <= 12);
}
// n polynomials on the device, in -> out (equal, or disjoint; 16-byte aligned), on s.  Up to the tails' size: kzg_ntt_kernel as nbls_fr_ntt launches it.  Above: the flags
// cleared, then the runs and the tails in the direction's order -- the first launch reads `in`, every later one works in place on `out`
static int fr_ntt_large_dev(nbls_ctx* ctx, unsigned L, int dir, size_t n, const uint8_t* in, const uint8_t* shift, uint8_t* out, int8_t* status, hipStream_t s) {
  const unsigned t = ntt_tail_bits(ctx), P = ctx->ntt_pass_bits ? ctx->ntt_pass_bits : FR_NTTL_DEFAULT_PASS;
  const bool inverse = dir == NBLS_NTT_TO_COEFFS;
  const uint8_t *roots, *iroots, *table; int r;
  if (L <= t) {
    if ((r = kzg_table(ctx, KZG_ROOTS, L, 0, s, &roots)) || (r = kzg_table(ctx, KZG_INV_ROOTS, L, 0, s, &iroots))) return r;
    LAUNCHCHK(nbls_kzg_ntt_launch(L, inverse ? FR_NTT_TO_COEFFS : FR_NTT_TO_EVALS, (unsigned)n, in, shift, 32, roots, iroots, out, nullptr, status, s));
    return NBLS_OK;
  }
  const unsigned K = L - t, runs = fr_nttl_runs(K, P);
  const size_t fb = (n * 4 + 31) & ~(size_t)31;
  uint8_t* F;
  if ((r = need(ctx, SB_NTTL_FLAGS, fb + n * 32, &F)) || (r = kzg_table(ctx, KZG_ROOTS, t, 0, s, &roots)) || (r = kzg_table(ctx, KZG_INV_ROOTS, t, 0, s, &iroots)) ||
      (r = kzg_table(ctx, inverse ? KZG_INV_ROOTS : KZG_ROOTS, K, 0, s, &table)))
    return r;
  uint8_t* SINV = F + fb;
  const Fr omega = fr_omega(L), w = inverse ? fr_inv(omega) : omega;
  HIPCHK(hipMemsetAsync(F, 0, fb, s));
  auto tails = [&](const uint8_t* src) { return nbls_kzg_ntt_tail_launch(t, K, inverse, (unsigned)n, w.l, src, out, shift, SINV, roots, iroots, F, status, s); };
  auto run = [&](unsigned i, const uint8_t* src) {
    const FrNttRun R = fr_nttl_run(L, K, P, i);
    const bool first = R.j0 == 0;   // the run that has stage 0: the caller's shift on the way to the values, its inverse and the status on the way back
    return nbls_kzg_ntt_pass_launch(&R, inverse, (unsigned)n, src, out, first && !inverse ? shift : nullptr, first && inverse && shift ? SINV : nullptr, table, F,
                                    first && inverse ? status : nullptr, s);
  };
  if (inverse) {
    LAUNCHCHK(tails(in));
    for (unsigned i = runs; i-- > 0;) LAUNCHCHK(run(i, out));
  } else {
    for (unsigned i = 0; i < runs; i++) LAUNCHCHK(run(i, i ? out : in));
    LAUNCHCHK(tails(out));
  }
  return NBLS_OK;
}
EXPORT int nbls_fr_ntt_large(nbls_ctx* ctx, unsigned log2_n, int dir, size_t n, const uint8_t* in32, const uint8_t* shift32, uint8_t* out32, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ntt_large_args(ctx, log2_n, dir, n) || (n && (!in32 || !out32))) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t qb = (n * 32) << log2_n, o_in = io.bytes(in32, qb), o_sh = io.bytes(shift32, shift32 ? n * 32 : 0), back = qb + n;
  uint8_t *c, *O; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGC_OUT, back, &O)) || (r = io.send(c, back)) ||
      (r = fr_ntt_large_dev(ctx, log2_n, dir, n, c + o_in, shift32 ? c + o_sh : nullptr, O, (int8_t*)(O + qb), s)))
    return r;
  return io.fetch_to(O, out32, qb, status, n);
}
EXPORT int nbls_fr_ntt_dev(nbls_ctx* ctx, unsigned log2_n, int dir, size_t n, const void* d_in32, const void* d_shift32, void* d_out32, void* d_status, void* stream) {
  if (!ntt_large_args(ctx, log2_n, dir, n) || (n && (!d_in32 || !d_out32))) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  const uintptr_t a = (uintptr_t)d_in32, b = (uintptr_t)d_out32, qb = ((uintptr_t)n * 32) << log2_n;
  if (((a | b) & 15) || (a != b && a < b + qb && b < a + qb)) return NBLS_EINVAL;
  DEV_ENTER(ctx, stream);
  return fr_ntt_large_dev(ctx, log2_n, dir, n, (const uint8_t*)d_in32, (const uint8_t*)d_shift32, (uint8_t*)d_out32, (int8_t*)d_status, s);
}

// mono == NULL and fk == NULL: nbls_kzg_compute_cells (out_proofs unused).  fk != NULL: the FK20 proofs loop.  rec != NULL: the recovery front end -- the blobs come from subsets of their cells (blobs unused)
struct RecoverIn { const uint32_t *offsets, *index; const uint8_t* cells; };
struct CellsIn { unsigned log2_n, log2_cell; size_t n; const uint8_t* blobs; const nbls_kzg_monomial* mono; uint8_t *out_cells, *out_proofs; const RecoverIn* rec; const nbls_kzg_fk20* fk = nullptr; };

// Two front ends to one coefficients buffer, one proofs loop behind them.  From whole blobs: kzg_ntt_kernel's cells mode.  From cells (rec): the index sets are checked here,
// on the host, before the copy -- a refused blob (NBLS_ST_BAD_CELLS) sends an empty slot map and none of its cells --, then kzg_recover_z_kernel and kzg_recover_kernel leave the
// same three things the cells mode leaves: the 2 N elements of every blob, its coefficients, its status.  The Z values live on SB_KZGR_Z (M_KZGR_OWN)
static int cells_pipeline(nbls_ctx* ctx, const CellsIn& in, int8_t* status) {
  const unsigned L = in.log2_n, lc = in.log2_cell, lm = L + 1 - lc;
  const size_t n = in.n, N = (size_t)1 << L, M = (2 * N) >> lc, qb = n * N * 32;   // M: the cells, and the quotient rows, of one blob
  const nbls_kzg_fk20* fk = in.fk;
  const bool proofs = in.mono != nullptr || fk, passes = fk && M > 2;   // (M = 2: n' = 1)
  const RecoverIn* rec = in.rec;
  uint8_t g32[32];
  fr_to_bytes(fr_omega(L + 1), g32);   // g = omega_2N, the shift of the coset
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  size_t o_blob = 0, o_g = 0, o_cells = 0, o_slot = 0, o_pre = 0, o_k = 0;
  std::vector<uint32_t> slot; std::vector<int8_t> pre; FrRecoverConsts kc;
  if (rec) {
    const size_t cb = (size_t)32 << lc;
    slot.resize(n * M); pre.resize(n);
    kc = fr_recover_consts(L, lc);
    uint32_t at = 0;   // (entries staged so far: at most n M, the cells of 2^24 elements of blobs)
    for (size_t i = 0; i < n; i++) {
      const size_t first = rec->offsets[i], cnt = rec->offsets[i + 1] - first;
      if ((pre[i] = (int8_t)fr_recover_slots(rec->index ? rec->index + first : nullptr, at, cnt, lm, &slot[i * M]))) continue;
      const size_t o = io.bytes(rec->cells + first * cb, cnt * cb);   // (whole cells: the parts follow one another without a gap)
      if (!at) o_cells = o;
      at += (uint32_t)cnt;
    }
    o_slot = io.bytes(slot.data(), slot.size() * 4); o_pre = io.bytes(pre.data(), n); o_k = io.bytes(&kc, sizeof kc);
  } else {
    o_blob = io.bytes(in.blobs, qb); o_g = io.bytes(g32, 32);
  }
  // blobs per pass: as many whole blobs as the batched MSM takes, or fewer where the tuning key says so
  // (the FK20 loop: 2 N scalars a blob in pass A, M^2 in pass B, M groups in both)
  size_t per = fk ? std::min({n, MSMB_MAX_ITEMS / (2 * N), MSMB_MAX_ITEMS / (M * M), MSMB_MAX_GROUPS / M}) : proofs ? std::min({n, (MSMB_MAX_ITEMS >> L) / M, MSMB_MAX_GROUPS / M}) : n;
  if (proofs && ctx->cells_chunk && ctx->cells_chunk < per) per = ctx->cells_chunk;
  const size_t tail = n % per;
  // what is read back: the cells | the compressed proofs | the blobs' statuses; behind it one pass's affine sums, zero flags and closing statuses
  const size_t b_pf = 2 * qb, b_st = b_pf + (proofs ? n * M * 48 : 0), back = b_st + n;
  size_t sz_out = 0, sz_rows = 0;
  const size_t a_bk = carve(&sz_out, back), a_aff = carve(&sz_out, proofs ? per * M * 96 : 0), a_zf = carve(&sz_out, proofs ? per * M : 0), a_cst = carve(&sz_out, proofs ? per * M : 0);
  const size_t a_q = carve(&sz_rows, !proofs ? 0 : fk ? per * 2 * N * 32 : per * M * N * 32), a_rst = carve(&sz_rows, proofs ? per * M : 0);
  const size_t sz_yh = passes ? per * M * 6 * RAW : 0, cs = (size_t)1 << lc;
  // the plans of a pass of `blobs` blobs: the rows (a), or pass A (a) and pass B (b).  (The larger pass first: the smaller then finds both of the MSM's slots large enough)
  MsmbPlan pl_full, pl_tail, plb_full, plb_tail;
  auto plans = [&](size_t blobs, MsmbPlan* a, MsmbPlan* b) -> int {
    if (!fk) return msm_rows_dev_plan(ctx, N, blobs * M, a);
    if (!passes) return NBLS_OK;
    const int e = msm_map_dev_plan(ctx, cs, cs * M, 0, 0, blobs * M, a);
    return e ? e : msm_map_dev_plan(ctx, M, M, M * M, M * M, blobs * M, b);
  };
  uint8_t* YH = nullptr;
  uint8_t *c, *OUT, *COEF = nullptr, *ROWS = nullptr, *ZV = nullptr; const uint8_t *roots, *iroots, *sroots = nullptr, *got; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGC_OUT, sz_out, &OUT)) || ((proofs || rec) && (r = need(ctx, SB_KZGC_COEFS, qb, &COEF))) ||
      (rec && (r = need(ctx, SB_KZGR_Z, n * (M + M / 2) * sizeof(Fr), &ZV))) ||
      (proofs && (r = need(ctx, fk ? SB_KZGF_SCALARS : SB_KZGC_ROWS, sz_rows, &ROWS))) || (passes && (r = need(ctx, SB_KZGF_POINTS, sz_yh, &YH))) ||
      (proofs && (r = plans(per, &pl_full, &plb_full))) || (proofs && tail && (r = plans(tail, &pl_tail, &plb_tail))) || (r = kzg_table(ctx, KZG_ROOTS, L, 0, s, &roots)) || (r = kzg_table(ctx, KZG_INV_ROOTS, L, 0, s, &iroots)) ||
      ((proofs || rec) && (r = kzg_table(ctx, KZG_ROOTS, lm, 0, s, &sroots))) || (r = io.send(c, back)))
    return r;
  if (passes) msm_map_plans_settle(ctx, {&pl_full, &plb_full, &pl_tail, &plb_tail});   // (four plans on the MSM's two slots: the last need() decided where they are)
  uint8_t *BK = OUT + a_bk, *AFF = OUT + a_aff, *ZF = OUT + a_zf, *CST = OUT + a_cst, *Q = ROWS + a_q, *RST = ROWS + a_rst;
  if (rec) LAUNCHCHK(nbls_kzg_recover_launch(L, lc, (unsigned)n, c + o_cells, (const uint32_t*)(c + o_slot), c + o_pre, sroots, c + o_k, roots, iroots, ZV, BK, COEF, BK + b_st, s));
  else LAUNCHCHK(nbls_kzg_ntt_launch(L, FR_NTT_CELLS, (unsigned)n, c + o_blob, c + o_g, 0, roots, iroots, BK, COEF, BK + b_st, s));
  for (size_t b0 = 0; proofs && b0 < n; b0 += per) {
    const size_t nb = std::min(per, n - b0);
    uint8_t* P = BK + b_pf + b0 * M * 48;
    if (fk) {
      LAUNCHCHK(nbls_kzg_fk20_row_status_launch(lm, (unsigned)nb, BK + b_st + b0, RST, s));
      if (passes) {
        LAUNCHCHK(nbls_kzg_fk20_scalars_launch(L, lc, (unsigned)nb, COEF + b0 * N * 32, sroots, Q, s));
        if ((r = msm_map_dev(ctx, nb == per ? pl_full : pl_tail, fk->xhat, Q, nullptr, nullptr, nullptr, YH, s)) ||
            (r = msm_map_dev(ctx, nb == per ? plb_full : plb_tail, YH, nullptr, fk->bsplit, AFF, ZF, nullptr, s)))
          return r;
      } else {   // every sum is empty: the zero point, whatever the blob holds
        HIPCHK(hipMemsetAsync(AFF, 0, nb * M * 96, s)); HIPCHK(hipMemsetAsync(ZF, 1, nb * M, s));
      }
      if ((r = kzg_proof_close(ctx, nb * M, AFF, ZF, RST, nullptr, P, CST, s))) return r;
      continue;
    }
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
  return cells_pipeline(ctx, {log2_n, log2_cell, n, blobs, nullptr, out_cells, nullptr, nullptr}, status);
}

EXPORT int nbls_kzg_compute_cells_and_proofs_fk20(nbls_ctx* ctx, const nbls_kzg_fk20* fk, size_t n, const uint8_t* blobs, uint8_t* out_cells, uint8_t* out_proofs48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !fk || !blobs || !out_cells || !out_proofs48 || !n || fk->device != ctx->device || n > (KZG_MAX_ELEMS >> fk->log2_n)) return NBLS_EINVAL;
  return cells_pipeline(ctx, {fk->log2_n, fk->log2_cell, n, blobs, nullptr, out_cells, out_proofs48, nullptr, fk}, status);
}

EXPORT int nbls_kzg_compute_cells_and_proofs(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n, const uint8_t* blobs, uint8_t* out_cells,
                                             uint8_t* out_proofs48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !monomial || !blobs || !out_cells || !out_proofs48 || !n || monomial->device != ctx->device || log2_cell > monomial->log2_n) return NBLS_EINVAL;
  const unsigned L = monomial->log2_n;
  // one blob alone must fit a pass of the batched MSM: (2 N / c) rows of N scalars
  if (((size_t)2 << (2 * L - log2_cell)) > MSMB_MAX_ITEMS || n > (KZG_MAX_ELEMS >> L)) return NBLS_EINVAL;
  return cells_pipeline(ctx, {L, log2_cell, n, blobs, monomial, out_cells, out_proofs48, nullptr}, status);
}

// what both recovery calls refuse before any device work (the header's list)
static bool recover_args_ok(unsigned log2_n, unsigned log2_cell, size_t n, const uint32_t* off, const uint32_t* index, const uint8_t* cells, const uint8_t* out_cells) {
  if (log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 12 || !off || !out_cells || off[0] != 0 || n > (KZG_MAX_ELEMS >> log2_n)) return false;
  for (size_t i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
  return !off[n] || (index && cells);
}
EXPORT int nbls_kzg_recover_cells(nbls_ctx* ctx, unsigned log2_n, unsigned log2_cell, size_t n, const uint32_t* cell_offsets, const uint32_t* cell_index, const uint8_t* cells,
                                  uint8_t* out_cells, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > 12 || log2_cell > log2_n || log2_n + 1 - log2_cell > 12) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  if (!recover_args_ok(log2_n, log2_cell, n, cell_offsets, cell_index, cells, out_cells)) return NBLS_EINVAL;
  const RecoverIn rec{cell_offsets, cell_index, cells};
  return cells_pipeline(ctx, {log2_n, log2_cell, n, nullptr, nullptr, out_cells, nullptr, &rec}, status);
}

EXPORT int nbls_kzg_recover_cells_and_proofs(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n, const uint32_t* cell_offsets,
                                             const uint32_t* cell_index, const uint8_t* cells, uint8_t* out_cells, uint8_t* out_proofs48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !monomial || !out_proofs48 || !n || monomial->device != ctx->device) return NBLS_EINVAL;
  const unsigned L = monomial->log2_n;
  // one blob alone must fit a pass of the batched MSM: (2 N / c) rows of N scalars
  if (!recover_args_ok(L, log2_cell, n, cell_offsets, cell_index, cells, out_cells) || ((size_t)2 << (2 * L - log2_cell)) > MSMB_MAX_ITEMS) return NBLS_EINVAL;
  const RecoverIn rec{cell_offsets, cell_index, cells};
  return cells_pipeline(ctx, {L, log2_cell, n, nullptr, monomial, out_cells, out_proofs48, &rec}, status);
}

EXPORT int nbls_kzg_recover_cells_and_proofs_fk20(nbls_ctx* ctx, const nbls_kzg_fk20* fk, size_t n, const uint32_t* cell_offsets, const uint32_t* cell_index, const uint8_t* cells,
                                                  uint8_t* out_cells, uint8_t* out_proofs48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !fk || !out_proofs48 || !n || fk->device != ctx->device) return NBLS_EINVAL;
  if (!recover_args_ok(fk->log2_n, fk->log2_cell, n, cell_offsets, cell_index, cells, out_cells)) return NBLS_EINVAL;   // (the handle exists: one blob fits a pass)
  const RecoverIn rec{cell_offsets, cell_index, cells};
  return cells_pipeline(ctx, {fk->log2_n, fk->log2_cell, n, nullptr, nullptr, out_cells, out_proofs48, &rec, fk}, status);
}
