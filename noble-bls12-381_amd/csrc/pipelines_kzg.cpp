// pipelines_kzg.cpp -- KZG verification on BLS12-381 (EIP-4844: verify_kzg_proof_batch, verify_blob_kzg_proof_batch) and the evaluation of polynomials given by their values on
// the roots of unity.  A tuple (C, z, y, pi) holds when e(pi, [tau]G2) = e(C + [z]pi - [y]G1, G2); n tuples are checked together with the secret weights r_i of
// nbls_verify_multiple (rlc_weights.h):
//   e(A, [tau]G2) * e(B, -G2) = 1,   A = sum_i [r_i]pi_i,   B = sum_i [r_i]C_i + sum_i [r_i z_i]pi_i - [sum_i r_i y_i]G1
// (the issue's form with the sign moved from A to the fixed G2 point: no point is negated on the device).  One chain on the context's stream:
//   H2D copy -> [tau]G2: PointG2.fromSignature; its line table and -G2's (P_LINES_Q) -> weights -> dev_decompress of the 2 n G1 points (PointG1.fromHex, subgroup check included)
//            -> blobs only: the challenges z_i, hashed on host threads BEHIND the copy and the launches above, follow as a second small copy; y_i = p_i(z_i) (kzg_eval_kernel)
//            -> kzg_items_kernel / kzg_sum_kernel: statuses and scalars
//            -> A: the 64-bit MSM over the proofs; B: a 64-bit MSM over the commitments + a 256-bit MSM over the proofs + one fixed-base ladder, joined by two complete additions
//               (three sums of n points each: one sum of 2 n + 1 points would pass dev_msm's bound of 2^22 at half the contract's n)
//            -> two Miller loops against the two tables -> product -> final exponentiation -> compared with one -> D2H copy
// Zero points are valid (the zero polynomial's commitment, a constant polynomial's proof): a zero point gets a zero scalar and the generator's bytes, and when A or B is the zero
// point the generator stands in for it in the Miller loop while the flag decides: e(O, Q) = 1, so A = B = O accepts, exactly one of them zero rejects (e(P, Q) != 1 for P != O in
// the subgroup).  Where the combined check does not accept and the caller asked for statuses, the per-item pass judges every tuple: X_i = C_i + [z_i]pi_i - [y_i]G1 by two
// ladders and two complete additions, millerLoop(pi_i, table of [tau]G2) * millerLoop(X_i, table of -G2) with table_stride = 0, one batched final exponentiation, rlc_is_one.
// The staged [tau]G2 | -G2 | seed, the pairs block, the opening launches, the read-back with its verdict and the close of the per-item pass are KzgFrame's (kzg_common.cpp),
// shared with the cell verifier; the seed and the device helpers KzgFrame runs are shared with every weighted verifier; the rest of the chain is this file's.
// Scratch slots: SB_STAGED and SB_KZG_* (nbls_internal.h, M_KZG_OWN); the decoder and the ladders run on the main slots, the MSMs on MSM_RLC's (MSM_MAIN holds SB_STAGED).
#include "nbls_internal.h"
#include "fr_exec.h"
#include <algorithm>

static const size_t KZG_MAX_ITEMS = (size_t)1 << 22;   // dev_msm's bound: every sum of the chain has n points

EXPORT int nbls_fr_eval_roots(nbls_ctx* ctx, unsigned log2_n, size_t n, const uint8_t* evals32, const uint8_t* z32, uint8_t* out32, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > 12 || (n && (!evals32 || !z32 || !out32)) || n > (KZG_MAX_ELEMS >> log2_n)) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_ev = io.bytes(evals32, (n * 32) << log2_n), o_z = io.bytes(z32, n * 32), back = n * 33;
  uint8_t *c, *O; const uint8_t* roots; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZG_OUT, back, &O)) || (r = kzg_table(ctx, KZG_ROOTS, log2_n, 0, s, &roots)) || (r = io.send(c, back))) return r;
  LAUNCHCHK(nbls_kzg_eval_launch(log2_n, (unsigned)n, c + o_ev, c + o_z, roots, O, O + n * 32, s));
  return io.fetch_to(O, out32, n * 32, status, n);
}

// blobs == NULL: nbls_kzg_verify_proofs (z32, y32 from the caller); else nbls_kzg_verify_blobs (z32 = y32 = NULL: the challenges are hashed inside the pipeline, y_i evaluated on the device)
struct KzgIn { size_t n; unsigned log2_n; const uint8_t *blobs, *c48, *z32, *y32, *p48, *tau96, *seed32; };

static int kzg_pipeline(nbls_ctx* ctx, const KzgIn& in, int* all_ok, int8_t* status) {
  const size_t n = in.n;
  std::vector<uint8_t> zhost;   // (declared in front of the staged block: it outlives the wait of that block's destructor)
  uint8_t seed[32]; int r; bool more;
  if ((r = rlc_seed(in.seed32, seed))) return r;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  KzgFrame fr(ctx, io, s, n, SB_KZG_PAIRS, SB_KZG_OUT, SB_KZG_ITEMS);
  // the staged block: commitments | proofs (one array of 2 n compressed points) | z | y | [tau]G2 | -G2 | seed | blobs
  const size_t o_cp = io.bytes(in.c48, n * 48), o_pf = io.bytes(in.p48, n * 48), o_z = io.bytes(in.z32, in.z32 ? n * 32 : 0), o_y = io.bytes(in.y32, in.y32 ? n * 32 : 0);
  fr.stage(in.tau96, seed);
  const size_t o_blob = io.bytes(in.blobs, in.blobs ? (n * 32) << in.log2_n : 0);
  if (o_pf != o_cp + n * 48) return NBLS_EINVAL;   // (n * 48 is a multiple of the parts' alignment)
  size_t sz_pt = 0, sz_sc = 0, sz_it = 0;
  const size_t a_aff = carve(&sz_pt, (2 * n + 1) * 96), a_dst = carve(&sz_pt, 2 * n);
  const size_t a_w = carve(&sz_sc, n * 32), a_s1 = carve(&sz_sc, n * 32), a_s2 = carve(&sz_sc, (2 * n + 1) * 32), a_t = carve(&sz_sc, n * 32), a_y = carve(&sz_sc, n * 32), a_yst = carve(&sz_sc, n), a_z = carve(&sz_sc, n * 32);
  uint8_t *c, *PTS, *SC, *IT; const uint8_t* roots = nullptr;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZG_POINTS, sz_pt, &PTS)) || (r = need(ctx, SB_KZG_SCALARS, sz_sc, &SC)) || (r = fr.take()) ||
      (in.blobs && (r = kzg_table(ctx, KZG_ROOTS, in.log2_n, 0, s, &roots))) || (r = io.send(c, back_bytes(n))))
    return r;
  uint8_t *AFF = PTS + a_aff, *DST = PTS + a_dst, *W = SC + a_w, *S1 = SC + a_s1, *S2 = SC + a_s2, *T = SC + a_t, *Y = SC + a_y, *YST = SC + a_yst;
  const uint8_t *d_z = in.blobs ? SC + a_z : c + o_z, *d_y = in.blobs ? Y : c + o_y;
  if ((r = fr.open(c, W)) || (r = dev_decompress(ctx, false, 2 * n, c + o_cp, AFF, DST, s))) return r;
  if (in.blobs) {   // the device is busy with the copy and the decoders: now the host hashes
    zhost.resize(n * 32);
    blob_challenges(in.log2_n, n, in.blobs, in.c48, zhost.data());
    HIPCHK(hipMemcpyAsync(SC + a_z, zhost.data(), n * 32, hipMemcpyHostToDevice, s));
  }
  if (in.blobs) LAUNCHCHK(nbls_kzg_eval_launch(in.log2_n, (unsigned)n, c + o_blob, d_z, roots, Y, YST, s));
  LAUNCHCHK(nbls_kzg_items_launch((unsigned)n, DST, W, d_z, d_y, in.blobs ? YST : nullptr, ctx->gen_g1, AFF, S1, S2, T, fr.PRE, s));
  if ((r = dev_msm(ctx, false, n, AFF + n * 96, S1, 64, fr.PT2, fr.A_ZERO, s, MSM_RLC))) return r;
  // B = sum_i [r_i]C_i | sum_i [r_i z_i]pi_i | [-sum_i r_i y_i]G1: affine points with a status each (1 = the zero point), joined by the frame's combined check
  if ((r = dev_msm(ctx, false, n, AFF, S2, 64, fr.B3, fr.BST, s, MSM_RLC)) || (r = dev_msm(ctx, false, n, AFF + n * 96, S2 + n * 32, 256, fr.B3 + 96, fr.BST + 1, s, MSM_RLC)) ||
      (r = dev_point_mul(ctx, false, 1, ctx->gen_g1, 0, S2 + 2 * n * 32, fr.B3 + 192, fr.BST + 2, s)) || (r = fr.decide(all_ok, status, &more)) || !more)
    return r;
  // ---- the per-item pass
  const size_t b_zs = carve(&sz_it, n * 32), b_ny = carve(&sz_it, n * 32);
  if ((r = fr.items_begin(sz_it, &IT))) return r;
  uint8_t *ZS = IT + b_zs, *NY = IT + b_ny, *P3 = fr.P3, *ST3 = fr.ST3;
  LAUNCHCHK(nbls_kzg_item_scalars_launch((unsigned)n, fr.PRE, DST, d_z, d_y, ZS, NY, s));
  HIPCHK(hipMemcpyAsync(P3, AFF, n * 96, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(ST3, DST, n, hipMemcpyDeviceToDevice, s));
  // C_i | [z_i]pi_i | [-y_i]G1: the three summands of X_i
  if ((r = dev_point_mul(ctx, false, n, AFF + n * 96, 96, ZS, P3 + n * 96, ST3 + n, s)) || (r = dev_point_mul(ctx, false, n, ctx->gen_g1, 0, NY, P3 + 2 * n * 96, ST3 + 2 * n, s))) return r;
  return fr.items_close(AFF + n * 96, DST + n, all_ok, status);
}

EXPORT int nbls_kzg_verify_proofs(nbls_ctx* ctx, size_t n, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32, const uint8_t* proofs48, const uint8_t* tau_g2_96,
                                  const uint8_t* seed32, int* all_ok, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !n || n > KZG_MAX_ITEMS || !commitments48 || !z32 || !y32 || !proofs48 || !tau_g2_96 || !all_ok) return NBLS_EINVAL;
  return kzg_pipeline(ctx, {n, 0, nullptr, commitments48, z32, y32, proofs48, tau_g2_96, seed32}, all_ok, status);
}

EXPORT int nbls_kzg_verify_blobs(nbls_ctx* ctx, unsigned log2_n, size_t n, const uint8_t* blobs, const uint8_t* commitments48, const uint8_t* proofs48, const uint8_t* tau_g2_96,
                                 const uint8_t* seed32, int* all_ok, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > 12 || !n || n > KZG_MAX_ITEMS || n > (KZG_MAX_ELEMS >> log2_n) || !blobs || !commitments48 || !proofs48 || !tau_g2_96 || !all_ok) return NBLS_EINVAL;
  return kzg_pipeline(ctx, {n, log2_n, blobs, commitments48, nullptr, nullptr, proofs48, tau_g2_96, seed32}, all_ok, status);
}
