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
// Scratch slots: SB_STAGED and SB_KZG_* (nbls_internal.h, M_KZG_OWN); the decoder and the ladders run on the main slots, the MSMs on MSM_RLC's (MSM_MAIN holds SB_STAGED).
#include "nbls_internal.h"
#include "fr_exec.h"
#include <algorithm>

static const size_t KZG_MAX_ELEMS = (size_t)1 << 24;
static const size_t KZG_MAX_ITEMS = (size_t)1 << 22;   // dev_msm's bound: every sum of the chain has n points

// -G2 in affine wire bytes (x.c0 || x.c1 || p - y.c0 || p - y.c1), from the generator's standard coordinates
const uint8_t* neg_g2_wire() {
  static uint8_t w[192];
  static const bool once = [] {
    static const char* hex[5] = {
        "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8",
        "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e",
        "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801",
        "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be",
        "1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab"};
    uint8_t v[5][48];
    auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
    for (int k = 0; k < 5; k++) for (int i = 0; i < 48; i++) v[k][i] = (uint8_t)(nib(hex[k][2 * i]) << 4 | nib(hex[k][2 * i + 1]));
    memcpy(w, v[0], 48); memcpy(w + 48, v[1], 48);
    for (int k = 2; k < 4; k++) {
      int bw = 0;
      for (int i = 47; i >= 0; i--) { const int d = (int)v[4][i] - (int)v[k][i] - bw; w[48 * k + i] = (uint8_t)d; bw = d < 0; }
    }
    return true;
  }();
  (void)once;
  return w;
}

int kzg_roots(nbls_ctx* ctx, unsigned log2_n, hipStream_t s, const uint8_t** table) {
  if (!ctx->kzg_roots[log2_n]) {
    uint8_t* t = nullptr;
    HIPCHK(hipMalloc(&t, (size_t)32 << log2_n));
    const int e = nbls_kzg_roots_launch(log2_n, t, s);
    if (e) { hipFree(t); ctx->last_hip = e; return NBLS_EHIP; }
    ctx->kzg_roots[log2_n] = t;
  }
  *table = ctx->kzg_roots[log2_n];
  return NBLS_OK;
}
// the inverse roots, a permutation of the table above (made behind it on the same stream)
int kzg_inv_roots(nbls_ctx* ctx, unsigned log2_n, hipStream_t s, const uint8_t** table) {
  if (!ctx->kzg_inv_roots[log2_n]) {
    const uint8_t* roots; uint8_t* t = nullptr;
    const int r = kzg_roots(ctx, log2_n, s, &roots); if (r) return r;
    HIPCHK(hipMalloc(&t, (size_t)32 << log2_n));
    const int e = nbls_kzg_inv_roots_launch(log2_n, roots, t, s);
    if (e) { hipFree(t); ctx->last_hip = e; return NBLS_EHIP; }
    ctx->kzg_inv_roots[log2_n] = t;
  }
  *table = ctx->kzg_inv_roots[log2_n];
  return NBLS_OK;
}

EXPORT int nbls_fr_eval_roots(nbls_ctx* ctx, unsigned log2_n, size_t n, const uint8_t* evals32, const uint8_t* z32, uint8_t* out32, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > 12 || (n && (!evals32 || !z32 || !out32)) || n > (KZG_MAX_ELEMS >> log2_n)) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t o_ev = io.bytes(evals32, (n * 32) << log2_n), o_z = io.bytes(z32, n * 32), back = n * 33;
  uint8_t *c, *O; const uint8_t* roots; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZG_OUT, back, &O)) || (r = kzg_roots(ctx, log2_n, s, &roots)) || (r = io.send(c, back))) return r;
  LAUNCHCHK(nbls_kzg_eval_launch(log2_n, (unsigned)n, c + o_ev, c + o_z, roots, O, O + n * 32, s));
  return io.fetch_to(O, out32, n * 32, status, n);
}

// z = BE(SHA-256("FSBLOBVERIFY_V1_" || BE128(N) || blob || commitment)) mod r, canonical bytes
static void blob_challenge(unsigned log2_n, const uint8_t* blob, const uint8_t* commitment48, uint8_t* z32) {
  uint8_t head[32] = {'F', 'S', 'B', 'L', 'O', 'B', 'V', 'E', 'R', 'I', 'F', 'Y', '_', 'V', '1', '_'}, digest[32];
  const uint32_t N = 1u << log2_n;
  head[30] = (uint8_t)(N >> 8); head[31] = (uint8_t)N;
  Sha256 h;
  h.update(head, 32); h.update(blob, (size_t)32 << log2_n); h.update(commitment48, 48); h.final(digest);
  fr_to_bytes(fr_from_bytes(digest), z32);
}
// the challenges of n blobs on up to eight host threads (2 N + 2 dependent SHA-256 blocks per blob: no work for a GPU lane); thread t takes the blobs t, t + threads, ..
// A thread that cannot be started costs nothing but time: the calling thread does its share
void blob_challenges(unsigned log2_n, size_t n, const uint8_t* blobs, const uint8_t* c48, uint8_t* z32) {
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t nt = std::max<size_t>(1, std::min<size_t>({n, 8, hw ? hw : 1}));
  auto share = [=](size_t t) { for (size_t i = t; i < n; i += nt) blob_challenge(log2_n, blobs + ((i * 32) << log2_n), c48 + 48 * i, z32 + 32 * i); };
  std::vector<std::thread> th;
  std::vector<size_t> mine{0};
  for (size_t t = 1; t < nt; t++) {
    try { th.emplace_back(share, t); } catch (...) { mine.push_back(t); }
  }
  for (size_t t : mine) share(t);
  for (std::thread& x : th) x.join();
}

// blobs == NULL: nbls_kzg_verify_proofs (z32, y32 from the caller); else nbls_kzg_verify_blobs (z32 = y32 = NULL: the challenges are hashed inside the pipeline, y_i evaluated on the device)
struct KzgIn { size_t n; unsigned log2_n; const uint8_t *blobs, *c48, *z32, *y32, *p48, *tau96, *seed32; };

static size_t carve(size_t* off, size_t bytes) { const size_t o = *off; *off = o + ((bytes + 63) & ~(size_t)63); return o; }

// From the three parts of B (affine points with a status each, 1 = the zero point) to the verdict of the combined check, shared with verify_cells_pipeline: raw projective,
// the identity where the status says so, two complete additions, affine again with B's own zero flag (BK[2]; A and its flag BK[1] are in place), the generator for a zero A or
// B, two Miller loops against the two tables, product, final exponentiation, BK[0] = the result is one
int kzg_combined_tail(nbls_ctx* ctx, const KzgCombined& k, hipStream_t s) {
  const size_t p = 3 * RAW; int r;
  if ((r = run(ctx, P_G1_TO_PROJ, 3, {B(0, k.B3, 96), B(3, k.BJ, p)}, s))) return r;
  LAUNCHCHK(nbls_agg_points_launch(3, (unsigned)p, nullptr, k.BST, ctx->ident_g1, k.BJ, k.BJ, s));
  if ((r = run(ctx, P_G1_ADD_AB, 1, {B(3, k.BJ, p), B(4, k.BJ + p, p), B(5, k.BJ, p)}, s)) || (r = run(ctx, P_G1_ADD_AB, 1, {B(3, k.BJ, p), B(4, k.BJ + 2 * p, p), B(5, k.BJ, p)}, s)) ||
      (r = to_affine(ctx, false, 1, k.BJ, k.BN, k.BN + RAW, k.PT2 + 96, k.BK + 2, s)))
    return r;
  LAUNCHCHK(nbls_agg_fix_zero_launch(2, k.BK + 1, ctx->gen_g1, k.PT2, nullptr, s));
  uint8_t* res = ctx->F;
  if ((r = run(ctx, P_ACC_Q, 2, {B(0, k.PT2, 96), B(3, k.TB, LINE_BYTES), B(5, ctx->F, F12)}, s)) || (r = reduce_product(ctx, 2, &res, s)) || (r = finish_single(ctx, Window(), res, 1, k.RES, s))) return r;
  LAUNCHCHK(nbls_rlc_is_one_launch(1, k.RES, k.BK, s));
  return NBLS_OK;
}
// The per-item tail, shared likewise.  kzg_item_tail_carve: its buffers as offsets from the block's own start (*off: the caller's carving, moved past the block; returns where
// the block starts).  kzg_item_tail: block = that start; the caller has written the three summands of every X_i to p3 (3 n affine points, summand after summand) and their
// statuses to st3 (non-zero: the identity) -> X_i by two complete additions, millerLoop(pi_i, table 0) * millerLoop(X_i, table 1) with table_stride = 0, one batched final
// exponentiation, compared with one on the device, kzg_item_status_kernel's rule -> the n statuses at fs.  The caller has run ensure_scratch(ctx, 2 n)
size_t kzg_item_tail_carve(size_t n, size_t* off, KzgItemTail* t) {
  const size_t p = 3 * RAW, start = *off;
  size_t o = 0;
  t->p3 = carve(&o, 3 * n * 96); t->st3 = carve(&o, 3 * n); t->proj = carve(&o, 3 * n * p); t->n = carve(&o, n * RAW); t->ni = carve(&o, n * RAW); t->x = carve(&o, n * 96);
  t->e = carve(&o, n * 576); t->v = carve(&o, n); t->xz = carve(&o, n); t->fs = carve(&o, n);
  *off = start + o;
  return start;
}
int kzg_item_tail(nbls_ctx* ctx, size_t n, const KzgItemTail& t, uint8_t* block, const uint8_t* proofs96, const uint8_t* tables, const uint8_t* pre, const uint8_t* proof_st, hipStream_t s) {
  const size_t p = 3 * RAW; int r;
  uint8_t *P3 = block + t.p3, *ST3 = block + t.st3, *PJ = block + t.proj, *N = block + t.n, *NI = block + t.ni, *X = block + t.x, *E = block + t.e, *V = block + t.v, *XZ = block + t.xz,
          *FS = block + t.fs;
  // the summands as raw projective points, the identity where the status says so (a zero commitment, a zero product, an item that is out), then two complete additions
  if ((r = run(ctx, P_G1_TO_PROJ, 3 * n, {B(0, P3, 96), B(3, PJ, p)}, s))) return r;
  LAUNCHCHK(nbls_agg_points_launch(3 * n, (unsigned)p, nullptr, ST3, ctx->ident_g1, PJ, PJ, s));
  if ((r = run(ctx, P_G1_ADD_AB, n, {B(3, PJ, p), B(4, PJ + n * p, p), B(5, PJ, p)}, s)) || (r = run(ctx, P_G1_ADD_AB, n, {B(3, PJ, p), B(4, PJ + 2 * n * p, p), B(5, PJ, p)}, s)) ||
      (r = to_affine(ctx, false, n, PJ, N, NI, X, XZ, s)))
    return r;
  LAUNCHCHK(nbls_agg_fix_zero_launch((unsigned)n, XZ, ctx->gen_g1, X, nullptr, s));
  if ((r = run(ctx, P_ACC_Q, n, {B(0, proofs96, 96), B(3, tables, 0), B(5, ctx->F, F12)}, s)) || (r = run(ctx, P_ACC_Q, n, {B(0, X, 96), B(3, tables + LINE_BYTES, 0), B(5, ctx->F + n * F12, F12)}, s)) ||
      (r = run(ctx, P_MUL2S, n, {B(3, ctx->F, F12), B(4, ctx->F + n * F12, F12), B(5, ctx->F, F12)}, s)) || (r = run(ctx, P_NORM_RAW, n, {B(3, ctx->F, F12), B(4, ctx->N, RAW)}, s)) ||
      (r = final_exp_pipeline(ctx, Window(), n, ctx->F, E, s)))
    return r;
  LAUNCHCHK(nbls_rlc_is_one_launch((unsigned)n, E, V, s));
  LAUNCHCHK(nbls_kzg_item_status_launch((unsigned)n, pre, proof_st, XZ, V, FS, s));
  return NBLS_OK;
}

static int kzg_pipeline(nbls_ctx* ctx, const KzgIn& in, int* all_ok, int8_t* status) {
  const size_t n = in.n, p = 3 * RAW;
  std::vector<uint8_t> zhost;   // (declared in front of the staged block: it outlives the wait of that block's destructor)
  uint8_t seed[32];
  if (in.seed32) memcpy(seed, in.seed32, 32);
  else { const int e = os_seed(seed); if (e) return e; }
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  // the staged block: commitments | proofs (one array of 2 n compressed points) | z | y | [tau]G2 | -G2 | seed | blobs
  const size_t o_cp = io.bytes(in.c48, n * 48), o_pf = io.bytes(in.p48, n * 48), o_z = io.bytes(in.z32, in.z32 ? n * 32 : 0), o_y = io.bytes(in.y32, in.y32 ? n * 32 : 0),
               o_tau = io.bytes(in.tau96, 96), o_ng2 = io.bytes(neg_g2_wire(), 192), o_seed = io.bytes(seed, 32), o_blob = io.bytes(in.blobs, in.blobs ? (n * 32) << in.log2_n : 0);
  if (o_pf != o_cp + n * 48) return NBLS_EINVAL;   // (n * 48 is a multiple of the parts' alignment)
  size_t sz_pt = 0, sz_sc = 0, sz_pr = 0;
  const size_t a_aff = carve(&sz_pt, (2 * n + 1) * 96), a_dst = carve(&sz_pt, 2 * n);
  const size_t a_w = carve(&sz_sc, n * 32), a_s1 = carve(&sz_sc, n * 32), a_s2 = carve(&sz_sc, (2 * n + 1) * 32), a_t = carve(&sz_sc, n * 32), a_y = carve(&sz_sc, n * 32), a_yst = carve(&sz_sc, n), a_z = carve(&sz_sc, n * 32);
  const size_t a_g2 = carve(&sz_pr, 2 * 192), a_tb = carve(&sz_pr, 2 * LINE_BYTES), a_pt2 = carve(&sz_pr, 2 * 96), a_res = carve(&sz_pr, 576), a_b3 = carve(&sz_pr, 3 * 96), a_bst = carve(&sz_pr, 3), a_bj = carve(&sz_pr, 3 * p), a_bn = carve(&sz_pr, 2 * RAW);
  // what is read back: the product is one | A is the zero point | B is | the decoder status of [tau]G2 | (12 unused) | the n statuses before any pairing
  const size_t back = 16 + n;
  uint8_t *c, *PTS, *SC, *PR, *BK; const uint8_t *roots = nullptr, *got; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZG_POINTS, sz_pt, &PTS)) || (r = need(ctx, SB_KZG_SCALARS, sz_sc, &SC)) || (r = need(ctx, SB_KZG_PAIRS, sz_pr, &PR)) ||
      (r = need(ctx, SB_KZG_OUT, back, &BK)) || (r = ensure_scratch(ctx, 2)) || (in.blobs && (r = kzg_roots(ctx, in.log2_n, s, &roots))) || (r = io.send(c, back)))
    return r;
  uint8_t *AFF = PTS + a_aff, *DST = PTS + a_dst, *W = SC + a_w, *S1 = SC + a_s1, *S2 = SC + a_s2, *T = SC + a_t, *Y = SC + a_y, *YST = SC + a_yst;
  uint8_t *G2P = PR + a_g2, *TB = PR + a_tb, *PT2 = PR + a_pt2, *RES = PR + a_res, *PRE = BK + 16, *B3 = PR + a_b3, *BST = PR + a_bst, *BJ = PR + a_bj, *BN = PR + a_bn;
  const uint8_t *d_z = in.blobs ? SC + a_z : c + o_z, *d_y = in.blobs ? Y : c + o_y;
  HIPCHK(hipMemsetAsync(BK, 0, 16, s));
  // [tau]G2 by PointG2.fromSignature's rules (its status is judged after the read-back: nothing is decided on the host before), then the two line tables
  if ((r = dev_decompress(ctx, true, 1, c + o_tau, G2P, BK + 3, s))) return r;
  HIPCHK(hipMemcpyAsync(G2P + 192, c + o_ng2, 192, hipMemcpyDeviceToDevice, s));
  if ((r = run(ctx, P_LINES_Q, 2, {B(1, G2P, 192), B(3, TB, LINE_BYTES)}, s))) return r;
  LAUNCHCHK(nbls_rlc_weights_launch((unsigned)n, c + o_seed, W, s));
  if ((r = dev_decompress(ctx, false, 2 * n, c + o_cp, AFF, DST, s))) return r;
  if (in.blobs) {   // the device is busy with the copy and the decoders: now the host hashes
    zhost.resize(n * 32);
    blob_challenges(in.log2_n, n, in.blobs, in.c48, zhost.data());
    HIPCHK(hipMemcpyAsync(SC + a_z, zhost.data(), n * 32, hipMemcpyHostToDevice, s));
  }
  if (in.blobs) LAUNCHCHK(nbls_kzg_eval_launch(in.log2_n, (unsigned)n, c + o_blob, d_z, roots, Y, YST, s));
  LAUNCHCHK(nbls_kzg_items_launch((unsigned)n, DST, W, d_z, d_y, in.blobs ? YST : nullptr, ctx->gen_g1, AFF, S1, S2, T, PRE, s));
  if ((r = dev_msm(ctx, false, n, AFF + n * 96, S1, 64, PT2, BK + 1, s, MSM_RLC))) return r;
  // B = sum_i [r_i]C_i | sum_i [r_i z_i]pi_i | [-sum_i r_i y_i]G1: affine points with a status each (1 = the zero point) -> raw projective, the identity where the status says so,
  // two complete additions, affine again with B's own zero flag
  if ((r = dev_msm(ctx, false, n, AFF, S2, 64, B3, BST, s, MSM_RLC)) || (r = dev_msm(ctx, false, n, AFF + n * 96, S2 + n * 32, 256, B3 + 96, BST + 1, s, MSM_RLC)) ||
      (r = dev_point_mul(ctx, false, 1, ctx->gen_g1, 0, S2 + 2 * n * 32, B3 + 192, BST + 2, s)) || (r = kzg_combined_tail(ctx, {B3, BST, BJ, BN, PT2, TB, RES, BK}, s)))
    return r;
  if ((r = io.fetch(BK, back, &got))) return r;
  if (got[3] != 0) return NBLS_EDECODE;   // [tau]G2 does not decode, or is the zero point
  const bool one = got[0] != 0, za = got[1] == 1, zb = got[2] == 1;
  bool clean = true;
  for (size_t i = 0; i < n && clean; i++) clean = got[16 + i] == 0;
  if (clean && ((za && zb) || (!za && !zb && one))) {
    *all_ok = 1;
    if (status) memset(status, 0, n);
    return NBLS_OK;
  }
  *all_ok = 0;
  if (!status) return NBLS_OK;   // fast reject: no per-item work
  // ---- the per-item pass
  size_t sz_it = 0;
  KzgItemTail t;
  const size_t b_zs = carve(&sz_it, n * 32), b_ny = carve(&sz_it, n * 32), b_t = kzg_item_tail_carve(n, &sz_it, &t);
  uint8_t* IT;
  if ((r = need(ctx, SB_KZG_ITEMS, sz_it, &IT)) || (r = ensure_scratch(ctx, 2 * n))) return r;
  uint8_t *ZS = IT + b_zs, *NY = IT + b_ny, *P3 = IT + b_t + t.p3, *ST3 = IT + b_t + t.st3, *FS = IT + b_t + t.fs;
  ForkGuard guard;   // nothing is forked here: the guard is used for its wait alone.  fetch() has disarmed the staged block, and an error return below must not leave this chain running on slots the next call regrows
  LAUNCHCHK(nbls_kzg_item_scalars_launch((unsigned)n, PRE, DST, d_z, d_y, ZS, NY, s));
  HIPCHK(hipMemcpyAsync(P3, AFF, n * 96, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(ST3, DST, n, hipMemcpyDeviceToDevice, s));
  // C_i | [z_i]pi_i | [-y_i]G1: the three summands of X_i
  if ((r = dev_point_mul(ctx, false, n, AFF + n * 96, 96, ZS, P3 + n * 96, ST3 + n, s)) || (r = dev_point_mul(ctx, false, n, ctx->gen_g1, 0, NY, P3 + 2 * n * 96, ST3 + 2 * n, s)) ||
      (r = kzg_item_tail(ctx, n, t, IT + b_t, AFF + n * 96, TB, PRE, DST + n, s)))
    return r;
  if ((r = read_back(ctx, s, FS, n, &got))) return r;
  guard.armed = false;
  memcpy(status, got, n);
  int all = 1;
  for (size_t i = 0; i < n; i++) if (got[i]) all = 0;
  *all_ok = all;
  return NBLS_OK;
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
