// pipelines_kzg_prove.cpp -- the prover's side of KZG on BLS12-381 (EIP-4844: blob_to_kzg_commitment, compute_kzg_proof, compute_blob_kzg_proof), the quotient of an opening in
// evaluation form (nbls_fr_quotient_roots), against the device-resident setup (nbls_kzg_setup: the Lagrange basis decoded, checked and split ONCE by kzg_common.cpp, which
// has the handle).  With the basis points L_j = [L_j(tau)]G1 in bit-reversed order,
//   C_i = sum_j [f_ij] L_j,      pi_i = sum_j [q_ij] L_j,   q_ij = (f_ij - y_i) / (w_j - z_i)   (and compute_quotient_eval_within_domain's sum where z_i is a root).
// One chain on the context's stream:
//   H2D copy -> commitments: kzg_canon_kernel (a non-canonical blob is flagged and zeroed in place), the blob elements ARE the MSM's scalars
//            -> proofs: the challenges (blob proofs: hashed on host threads behind the copy, a second small copy) -> kzg_quotient_kernel: y_i, the canonical check, and the
//               quotient rows as 32-byte big-endian scalars
//            -> kzg_proof_tail (kzg_common.cpp; the commit leg and the proof leg close with it): msm_rows_dev (pipelines_msm.cpp), the scalars split along the
//               endomorphism, the slabs of the batched MSM against the setup's converted points, to-affine -> P_G1_COMPRESS -> kzg_prove_tail_kernel: statuses, 0xc0 00.. for a zero sum, all-zero bytes for a refused item -> D2H copy
// nbls_kzg_compute_blob_proofs without commitments runs the first chain on the staged blobs, reads the 48 n bytes back (the one synchronisation the challenge needs), hashes,
// and goes on with the second.  Scratch slots: SB_STAGED and SB_KZGP_* (nbls_internal.h, M_KZGP_OWN); the MSM on SB_MSMB_*.
#include "nbls_internal.h"
#include "fr_exec.h"
#include <algorithm>

EXPORT int nbls_fr_quotient_roots(nbls_ctx* ctx, unsigned log2_n, size_t n, const uint8_t* evals32, const uint8_t* z32, uint8_t* out_y32, uint8_t* out_q32, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > 12 || (n && (!evals32 || !z32 || !out_y32 || !out_q32)) || n > (KZG_MAX_ELEMS >> log2_n)) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  // what is read back: the values | the quotient rows | the statuses
  const size_t qb = (n * 32) << log2_n, o_ev = io.bytes(evals32, qb), o_z = io.bytes(z32, n * 32), back = n * 32 + qb + n;
  uint8_t *c, *O; const uint8_t *roots, *got; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGP_SCALARS, back, &O)) || (r = kzg_table(ctx, KZG_ROOTS, log2_n, 0, s, &roots)) || (r = io.send(c, back))) return r;
  LAUNCHCHK(nbls_kzg_quotient_launch(log2_n, (unsigned)n, c + o_ev, c + o_z, roots, O, O + n * 32, O + n * 32 + qb, s));
  if ((r = io.fetch(O, back, &got))) return r;
  memcpy(out_y32, got, n * 32); memcpy(out_q32, got + n * 32, qb);
  if (status) memcpy(status, got + n * 32 + qb, n);
  return NBLS_OK;
}

// mode 0: nbls_kzg_commit_blobs (out_p48 = the commitments); 1: nbls_kzg_compute_proofs (z32 from the caller); 2: nbls_kzg_compute_blob_proofs (c48 given, or NULL: committed
// first into out_c48)
struct ProveIn { int mode; size_t n; const uint8_t *blobs, *z32, *c48; uint8_t *out_c48, *out_p48, *out_y32; };

static int kzg_prove_pipeline(nbls_ctx* ctx, const nbls_kzg_setup* su, const ProveIn& in, int8_t* status) {
  const size_t n = in.n; const unsigned log2_n = su->log2_n;
  const size_t npts = (size_t)1 << log2_n, qb = (n * 32) << log2_n;
  const bool quot = in.mode != 0, commit = in.mode == 0 || (in.mode == 2 && !in.c48);
  std::vector<uint8_t> zhost;   // (declared in front of the staged block: it outlives the wait of that block's destructor)
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_blob = io.bytes(in.blobs, qb), o_z = io.bytes(in.z32, in.mode == 1 ? n * 32 : 0);
  size_t sz_sc = 0, sz_out = 0;
  const size_t a_q = carve(&sz_sc, quot ? qb : 0), a_z = carve(&sz_sc, in.mode == 2 ? n * 32 : 0), a_y = carve(&sz_sc, in.mode == 2 ? n * 32 : 0), a_qst = carve(&sz_sc, n), a_cst = carve(&sz_sc, n);
  // what is read back: the compressed sums | the values y_i (compute_proofs) | the statuses
  const size_t b_y = (n * 48 + 15) & ~(size_t)15, b_st = b_y + (in.mode == 1 ? n * 32 : 0), back = b_st + n;
  const size_t a_aff = carve(&sz_out, n * 96), a_zf = carve(&sz_out, n), a_bk = carve(&sz_out, back);
  MsmbPlan pl;
  uint8_t *c, *SC, *OUT; const uint8_t *roots = nullptr, *got; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGP_SCALARS, sz_sc, &SC)) || (r = need(ctx, SB_KZGP_OUT, sz_out, &OUT)) ||
      (r = msm_rows_dev_plan(ctx, npts, n, &pl)) || (quot && (r = kzg_table(ctx, KZG_ROOTS, log2_n, 0, s, &roots))) || (r = io.send(c, std::max(back, n * 48))))
    return r;
  uint8_t *Q = SC + a_q, *Z = SC + a_z, *QST = SC + a_qst, *CST = SC + a_cst, *AFF = OUT + a_aff, *ZF = OUT + a_zf, *BK = OUT + a_bk;
  const uint8_t* c48 = in.c48;
  if (commit) {
    LAUNCHCHK(nbls_kzg_canon_launch(log2_n, (unsigned)n, c + o_blob, CST, s));
    if ((r = kzg_proof_tail(ctx, pl, su->pts, c + o_blob, AFF, ZF, CST, nullptr, BK, BK + b_st, s))) return r;
    if (quot) {   // the challenges need the commitments on the host
      if ((r = read_back(ctx, s, BK, n * 48, &got))) return r;
      memcpy(in.out_c48, got, n * 48);
      c48 = in.out_c48;
    }
  }
  if (quot) {
    const uint8_t* d_z = c + o_z;
    if (in.mode == 2) {   // the device is busy with the copy (given commitments): now the host hashes
      zhost.resize(n * 32);
      blob_challenges(log2_n, n, in.blobs, c48, zhost.data());
      HIPCHK(hipMemcpyAsync(Z, zhost.data(), n * 32, hipMemcpyHostToDevice, s));
      d_z = Z;
    }
    LAUNCHCHK(nbls_kzg_quotient_launch(log2_n, (unsigned)n, c + o_blob, d_z, roots, in.mode == 1 ? BK + b_y : SC + a_y, Q, QST, s));
    if ((r = kzg_proof_tail(ctx, pl, su->pts, Q, AFF, ZF, commit ? CST : nullptr, QST, BK, BK + b_st, s))) return r;
  }
  if ((r = io.fetch(BK, back, &got))) return r;
  memcpy(in.out_p48, got, n * 48);
  if (in.mode == 1) memcpy(in.out_y32, got + b_y, n * 32);
  if (status) memcpy(status, got + b_st, n);
  return NBLS_OK;
}

static bool prove_args_ok(const nbls_ctx* ctx, const nbls_kzg_setup* su, size_t n, const uint8_t* blobs) {
  return ctx && su && blobs && n && su->device == ctx->device && n <= (MSMB_MAX_ITEMS >> su->log2_n);   // one pass of the batched MSM
}
EXPORT int nbls_kzg_commit_blobs(nbls_ctx* ctx, const nbls_kzg_setup* setup, size_t n, const uint8_t* blobs, uint8_t* out_commitments48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!prove_args_ok(ctx, setup, n, blobs) || !out_commitments48) return NBLS_EINVAL;
  return kzg_prove_pipeline(ctx, setup, {0, n, blobs, nullptr, nullptr, nullptr, out_commitments48, nullptr}, status);
}
EXPORT int nbls_kzg_compute_proofs(nbls_ctx* ctx, const nbls_kzg_setup* setup, size_t n, const uint8_t* blobs, const uint8_t* z32, uint8_t* out_proofs48, uint8_t* out_y32,
                                   int8_t* status) {
  WHOLE_CALL(ctx);
  if (!prove_args_ok(ctx, setup, n, blobs) || !z32 || !out_proofs48 || !out_y32) return NBLS_EINVAL;
  return kzg_prove_pipeline(ctx, setup, {1, n, blobs, z32, nullptr, nullptr, out_proofs48, out_y32}, status);
}
EXPORT int nbls_kzg_compute_blob_proofs(nbls_ctx* ctx, const nbls_kzg_setup* setup, size_t n, const uint8_t* blobs, const uint8_t* commitments48, uint8_t* out_commitments48,
                                        uint8_t* out_proofs48, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!prove_args_ok(ctx, setup, n, blobs) || !out_proofs48 || (!commitments48 && !out_commitments48)) return NBLS_EINVAL;
  const int r = kzg_prove_pipeline(ctx, setup, {2, n, blobs, nullptr, commitments48, out_commitments48, out_proofs48, nullptr}, status);
  if (!r && commitments48 && out_commitments48) memcpy(out_commitments48, commitments48, n * 48);
  return r;
}
