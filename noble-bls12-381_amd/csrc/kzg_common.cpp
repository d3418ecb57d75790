// kzg_common.cpp -- what the four KZG chains share (nbls_internal.h, the KZG section): -G2 and the blob challenges, the context's device tables, the two basis handles and the
// handle of the FK20 cell proofs, the prover's closing stage, and the KZG verifiers' frame (KzgFrame) around the combined check and the per-item pass, which kzg_pipeline and
// verify_cells_pipeline both run.  It also owns the device helpers of every weighted verifier -- sum3_affine, combined_tail, items_is_one, statuses_back -- which KzgFrame,
// groth16_pipeline and verify_multiple_pipeline's per-set pass run; the header those write into and the verdicts are verifier_frame.h's.
#include "nbls_internal.h"
#include "fr_exec.h"
#include <algorithm>

// -G2 in affine wire bytes: g2_wire_negate of the generator's standard coordinates x.c0, x.c1, y.c0, y.c1
const uint8_t* neg_g2_wire() {
  static uint8_t w[192];
  static const bool once = [] {
    static const char* hex = "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
                             "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                             "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801"
                             "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be";
    uint8_t g[192];
    auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
    for (int i = 0; i < 192; i++) g[i] = (uint8_t)(nib(hex[2 * i]) << 4 | nib(hex[2 * i + 1]));
    g2_wire_negate(g, w);
    return true;
  }();
  (void)once;
  return w;
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

int kzg_table(nbls_ctx* ctx, KzgTable kind, unsigned log2_n, unsigned log2_cell, hipStream_t s, const uint8_t** table) {
  const bool cells = kind == KZG_CELL_ISHIFTS;
  uint8_t*& slot = ctx->kzg_tables[cells ? 26 + 7 * log2_n + log2_cell : 13 * kind + log2_n];
  if (!slot) {
    const unsigned lm = cells ? log2_n + 1 - log2_cell : log2_n;   // the table has 2^lm entries
    const uint8_t* roots = nullptr; uint8_t* t = nullptr; int r;
    if (kind == KZG_INV_ROOTS && (r = kzg_table(ctx, KZG_ROOTS, log2_n, 0, s, &roots))) return r;
    HIPCHK(hipMalloc(&t, (size_t)32 << lm));
    const int e = cells ? nbls_kzg_cell_ishifts_launch(log2_n, lm, t, s) : roots ? nbls_kzg_inv_roots_launch(log2_n, roots, t, s) : nbls_kzg_roots_launch(log2_n, t, s);
    if (e) { hipFree(t); ctx->last_hip = e; return NBLS_EHIP; }
    slot = t;
  }
  *table = slot;
  return NBLS_OK;
}

// ---- the basis handles.  What the two create calls share: 2^log2_n compressed points decoded, subgroup-checked and converted into a device block of the context's device
// (*pts, the caller frees it); NBLS_EDECODE (and no block) where an entry does not decode or is the zero point; status (may be NULL) as the create calls state it
static int kzg_basis_decode(nbls_ctx* ctx, unsigned log2_n, const uint8_t* points48, int8_t* status, uint8_t** pts) {
  const size_t n = (size_t)1 << log2_n, p = 3 * RAW;
  std::vector<int8_t> st(n);
  LOCKED(ctx);
  HostIO io{ctx};
  void *d = io.alloc(n * 48), *a = io.alloc(n * 96), *dst = io.alloc(n);
  if (!d || !a || !dst) return NBLS_EHIP;
  uint8_t* mem = nullptr;
  if (hipMalloc(&mem, n * 2 * p) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); return NBLS_EHIP; }
  int r = NBLS_OK;
  hipError_t e = hipMemcpyAsync(d, points48, n * 48, hipMemcpyHostToDevice, s);
  // (an entry that does not decode goes through the conversion as whatever bytes the decoder left: the table is then discarded)
  if (e == hipSuccess && !(r = dev_decompress(ctx, false, n, d, a, dst, s)) && !(r = run(ctx, P_G1_MSM_PREP, n, {B(0, a, 96), B(3, mem, 2 * p)}, s))) {
    e = hipMemcpyAsync(st.data(), dst, n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) { ctx->last_hip = (int)e; r = NBLS_EHIP; }
  if (!r) {
    if (status) memcpy(status, st.data(), n);
    for (size_t j = 0; j < n; j++) if (st[j]) r = NBLS_EDECODE;   // 1: a zero point, which no real setup contains
  }
  if (r) { (void)hipStreamSynchronize(s); hipFree(mem); return r; }
  *pts = mem;
  return NBLS_OK;
}
// H: the public handle type, which adds nothing to KzgBasis but its name
template <class H> static void kzg_basis_destroy(H* h) {
  if (!h) return;
  handle_free(h->device, {h->pts});
  delete h;
}
template <class H> static int kzg_basis_create(nbls_ctx* ctx, unsigned log2_n, const uint8_t* points48, int8_t* status, H** out) {
  WHOLE_CALL(ctx);
  if (out) *out = nullptr;
  if (!ctx || log2_n < 1 || log2_n > 12 || !points48 || !out) return NBLS_EINVAL;
  return handle_create(ctx, out, kzg_basis_destroy<H>, [&](H* h) { h->log2_n = log2_n; return kzg_basis_decode(ctx, log2_n, points48, status, &h->pts); });
}
static int kzg_basis_log2n(const KzgBasis* h, unsigned* log2_n) {
  if (!h || !log2_n) return NBLS_EINVAL;
  *log2_n = h->log2_n;
  return NBLS_OK;
}
EXPORT int nbls_kzg_setup_create(nbls_ctx* ctx, unsigned log2_n, const uint8_t* lagrange48, int8_t* status, nbls_kzg_setup** out) { return kzg_basis_create(ctx, log2_n, lagrange48, status, out); }
EXPORT void nbls_kzg_setup_destroy(nbls_kzg_setup* su) { kzg_basis_destroy(su); }
EXPORT int nbls_kzg_setup_log2n(const nbls_kzg_setup* su, unsigned* log2_n) { return kzg_basis_log2n(su, log2_n); }
EXPORT int nbls_kzg_monomial_create(nbls_ctx* ctx, unsigned log2_n, const uint8_t* monomial48, int8_t* status, nbls_kzg_monomial** out) { return kzg_basis_create(ctx, log2_n, monomial48, status, out); }
EXPORT void nbls_kzg_monomial_destroy(nbls_kzg_monomial* m) { kzg_basis_destroy(m); }
EXPORT int nbls_kzg_monomial_log2n(const nbls_kzg_monomial* m, unsigned* log2_n) { return kzg_basis_log2n(m, log2_n); }

int kzg_proof_tail(nbls_ctx* ctx, const MsmbPlan& pl, const uint8_t* basis_pts, const uint8_t* rows, uint8_t* aff96, uint8_t* zero, const uint8_t* st_a, const uint8_t* st_b,
                   uint8_t* out48, uint8_t* status, hipStream_t s) {
  int r;
  if ((r = msm_rows_dev(ctx, pl, basis_pts, rows, aff96, zero, s))) return r;
  return kzg_proof_close(ctx, pl.n_groups, aff96, zero, st_a, st_b, out48, status, s);
}
int kzg_proof_close(nbls_ctx* ctx, size_t n, const uint8_t* aff96, const uint8_t* zero, const uint8_t* st_a, const uint8_t* st_b, uint8_t* out48, uint8_t* status, hipStream_t s) {
  int r;
  if ((r = run(ctx, P_G1_COMPRESS, n, {B(0, aff96, 96), B(2, out48, 48)}, s))) return r;
  LAUNCHCHK(nbls_kzg_prove_tail_launch((unsigned)n, zero, st_a, st_b, out48, status, s));
  return NBLS_OK;
}

// ---- the handle of the FK20 cell proofs (include/nbls.h has the contract, fr_exec.h the identities).  On the device throughout: the monomial basis gathered into the order of
// the one MSM's terms, the powers of the roots as its scalars, c M groups of n' - 1 terms in one pass, its sums kept projective with their endomorphism images; the matrix B
// from a kernel, split once.  The temporaries are the call's (HostIO); the MSM runs on the batched MSM's two slots
static int fk20_build(nbls_ctx* ctx, const nbls_kzg_monomial* mono, nbls_kzg_fk20* h) {
  const unsigned L = h->log2_n, lc = h->log2_cell, lm = L + 1 - lc;
  const size_t c = (size_t)1 << lc, M = (size_t)1 << lm, terms = M / 2 - 1, p = 3 * RAW, groups = c * M;
  LOCKED(ctx);
  HostIO io{ctx};
  // gathered point q = j (n' - 1) + e is tau^(j + c (n' - 2 - e)): the scalar index modulo c (n' - 1) then names its point
  std::vector<uint32_t> idx(c * terms);
  for (size_t j = 0; j < c; j++) for (size_t e = 0; e < terms; e++) idx[j * terms + e] = (uint32_t)(j + c * (terms - 1 - e));
  void *d_idx = io.alloc(idx.size() * 4), *Q = io.alloc(idx.size() * 2 * p), *K = io.alloc(groups * terms * 32), *Bm = io.alloc(M * M * 32);
  if (!d_idx || !Q || !K || !Bm) return NBLS_EHIP;
  const uint8_t *sroots, *isroots; MsmbPlan pl; int r;
  HIPCHK(hipMalloc(&h->xhat, groups * 2 * p));
  HIPCHK(hipMalloc(&h->bsplit, M * M * 64));
  HIPCHK(hipMemcpyAsync(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s));
  if ((r = kzg_table(ctx, KZG_ROOTS, lm, 0, s, &sroots)) || (r = kzg_table(ctx, KZG_INV_ROOTS, lm, 0, s, &isroots)) || (r = msm_map_dev_plan(ctx, terms, c * terms, 0, 0, groups, &pl)))
    return r;
  LAUNCHCHK(nbls_msm_gather_launch(idx.size(), (unsigned)(2 * p), (const uint32_t*)d_idx, mono->pts, Q, s));
  LAUNCHCHK(nbls_kzg_fk20_powers_launch(L, lc, sroots, K, s));
  LAUNCHCHK(nbls_kzg_fk20_matrix_launch(lm, sroots, isroots, Bm, s));
  if ((r = msm_split_scalars(ctx, M * M, (const uint8_t*)Bm, h->bsplit, s)) || (r = msm_map_dev(ctx, pl, (const uint8_t*)Q, (const uint8_t*)K, nullptr, nullptr, nullptr, h->xhat, s)))
    return r;
  HIPCHK(hipStreamSynchronize(s));   // (idx is read by the copy until here; an error return waits in ~HostIO)
  return NBLS_OK;
}
EXPORT int nbls_kzg_fk20_create(nbls_ctx* ctx, const nbls_kzg_monomial* mono, unsigned log2_cell, nbls_kzg_fk20** out) {
  WHOLE_CALL(ctx);
  if (out) *out = nullptr;
  if (!ctx || !mono || !out || mono->device != ctx->device || log2_cell > mono->log2_n) return NBLS_EINVAL;
  const unsigned L = mono->log2_n;
  // the M groups of M terms of one blob's second pass fit a pass of the batched MSM wherever the handle's own MSM does: (2 N / c) N scalars
  if (L + 1 - log2_cell > 12 || ((size_t)2 << (2 * L - log2_cell)) > MSMB_MAX_ITEMS) return NBLS_EINVAL;
  return handle_create(ctx, out, nbls_kzg_fk20_destroy, [&](nbls_kzg_fk20* h) {
    h->log2_n = L; h->log2_cell = log2_cell;
    return log2_cell == L ? NBLS_OK : fk20_build(ctx, mono, h);   // n' = 1: no sum has a term, every proof is the zero point
  });
}
EXPORT void nbls_kzg_fk20_destroy(nbls_kzg_fk20* h) {
  if (!h) return;
  handle_free(h->device, {h->xhat, h->bsplit});
  delete h;
}
EXPORT int nbls_kzg_fk20_params(const nbls_kzg_fk20* h, unsigned* log2_n, unsigned* log2_cell) {
  if (!h || !log2_n || !log2_cell) return NBLS_EINVAL;
  *log2_n = h->log2_n; *log2_cell = h->log2_cell;
  return NBLS_OK;
}

// ---- the device helpers of the weighted verifiers (nbls_internal.h states what each does)
int sum3_affine(nbls_ctx* ctx, size_t n, const uint8_t* p3, const uint8_t* st3, uint8_t* pj, uint8_t* nn, uint8_t* ni, uint8_t* out96, uint8_t* zero, hipStream_t s) {
  const size_t p = 3 * RAW; int r;
  if ((r = run(ctx, P_G1_TO_PROJ, 3 * n, {B(0, p3, 96), B(3, pj, p)}, s))) return r;
  LAUNCHCHK(nbls_agg_points_launch(3 * n, (unsigned)p, nullptr, st3, ctx->ident_g1, pj, pj, s));
  if ((r = run(ctx, P_G1_ADD_AB, n, {B(3, pj, p), B(4, pj + n * p, p), B(5, pj, p)}, s)) || (r = run(ctx, P_G1_ADD_AB, n, {B(3, pj, p), B(4, pj + 2 * n * p, p), B(5, pj, p)}, s))) return r;
  return to_affine(ctx, false, n, pj, nn, ni, out96, zero, s);
}
int combined_tail(nbls_ctx* ctx, size_t k, size_t mm, uint8_t* pts96, uint8_t* zero, const uint8_t* tables, uint8_t* res576, uint8_t* one, hipStream_t s) {
  int r;
  LAUNCHCHK(nbls_agg_fix_zero_launch((unsigned)k, zero, ctx->gen_g1, pts96, nullptr, s));
  uint8_t* res = ctx->F;
  if ((r = run(ctx, P_ACC_Q, k, {B(0, pts96, 96), B(3, tables, LINE_BYTES), B(5, ctx->F + mm * F12, F12)}, s)) || (r = reduce_product(ctx, mm + k, &res, s)) ||
      (r = finish_single(ctx, Window(), res, 1, res576, s)))
    return r;
  LAUNCHCHK(nbls_rlc_is_one_launch(1, res576, one, s));
  return NBLS_OK;
}
int items_is_one(nbls_ctx* ctx, size_t cnt, uint8_t* e576, uint8_t* v, hipStream_t s) {
  int r;
  if ((r = run(ctx, P_NORM_RAW, cnt, {B(3, ctx->F, F12), B(4, ctx->N, RAW)}, s)) || (r = final_exp_pipeline(ctx, Window(), cnt, ctx->F, e576, s))) return r;
  LAUNCHCHK(nbls_rlc_is_one_launch((unsigned)cnt, e576, v, s));
  return NBLS_OK;
}
int statuses_back(nbls_ctx* ctx, hipStream_t s, const uint8_t* fs, size_t n, ForkGuard& guard, int* all_ok, int8_t* status) {
  const uint8_t* got;
  const int r = read_back(ctx, s, fs, n, &got); if (r) return r;
  guard.armed = false;
  memcpy(status, got, n);
  *all_ok = std::all_of(got, got + n, [](uint8_t st) { return st == 0; });
  return NBLS_OK;
}

// ---- the KZG verifiers' frame
// The per-item tail.  block = the start kzg_item_tail_carve returned; the caller has written the three summands of every X_i to p3 (3 n affine points, summand after summand)
// and their statuses to st3 (non-zero: the identity: a zero commitment, a zero product, an item that is out) -> X_i = their sum, millerLoop(pi_i, table 0) *
// millerLoop(X_i, table 1) with table_stride = 0, one batched final exponentiation, compared with one on the device, kzg_item_status_kernel's rule -> the n statuses at fs.
// The caller has run ensure_scratch(ctx, 2 n)
static int kzg_item_tail(nbls_ctx* ctx, size_t n, const KzgItemTail& t, uint8_t* block, const uint8_t* proofs96, const uint8_t* tables, const uint8_t* pre, const uint8_t* proof_st, hipStream_t s) {
  int r;
  uint8_t *X = block + t.x, *V = block + t.v, *XZ = block + t.xz;
  if ((r = sum3_affine(ctx, n, block + t.p3, block + t.st3, block + t.proj, block + t.n, block + t.ni, X, XZ, s))) return r;
  LAUNCHCHK(nbls_agg_fix_zero_launch((unsigned)n, XZ, ctx->gen_g1, X, nullptr, s));
  if ((r = run(ctx, P_ACC_Q, n, {B(0, proofs96, 96), B(3, tables, 0), B(5, ctx->F, F12)}, s)) || (r = run(ctx, P_ACC_Q, n, {B(0, X, 96), B(3, tables + LINE_BYTES, 0), B(5, ctx->F + n * F12, F12)}, s)) ||
      (r = run(ctx, P_MUL2S, n, {B(3, ctx->F, F12), B(4, ctx->F + n * F12, F12), B(5, ctx->F, F12)}, s)) || (r = items_is_one(ctx, n, block + t.e, V, s)))
    return r;
  LAUNCHCHK(nbls_kzg_item_status_launch((unsigned)n, pre, proof_st, XZ, V, block + t.fs, s));
  return NBLS_OK;
}

KzgFrame::KzgFrame(nbls_ctx* c, Staged& st, hipStream_t stream, size_t items, Slot pairs, Slot out, Slot per_item)
    : ctx(c), io(st), s(stream), n(items), sb_pairs(pairs), sb_out(out), sb_items(per_item), a(kzg_pairs_carve()) {}
void KzgFrame::stage(const uint8_t* tau96, const uint8_t* seed) { o_tau = io.bytes(tau96, 96); o_ng2 = io.bytes(neg_g2_wire(), 192); o_seed = io.bytes(seed, 32); }
int KzgFrame::take() {
  int r;
  if ((r = need(ctx, sb_pairs, a.bytes, &PR)) || (r = need(ctx, sb_out, back_bytes(n), &BK)) || (r = ensure_scratch(ctx, 2))) return r;
  TB = PR + a.tb; PT2 = PR + a.pt2; B3 = PR + a.b3; BST = PR + a.bst; A_ZERO = kzg_hdr_a_zero(BK); PRE = hdr_pre(BK);
  return NBLS_OK;
}
int KzgFrame::open(uint8_t* c, uint8_t* W) {
  uint8_t* G2P = PR + a.g2; int r;
  HIPCHK(hipMemsetAsync(BK, 0, HDR_BYTES, s));
  // the G2 point by PointG2.fromSignature's rules (its status is judged after the read-back: nothing is decided on the host before), then the two line tables
  if ((r = dev_decompress(ctx, true, 1, c + o_tau, G2P, kzg_hdr_g2_status(BK), s))) return r;
  HIPCHK(hipMemcpyAsync(G2P + 192, c + o_ng2, 192, hipMemcpyDeviceToDevice, s));
  if ((r = run(ctx, P_LINES_Q, 2, {B(1, G2P, 192), B(3, TB, LINE_BYTES)}, s))) return r;
  LAUNCHCHK(nbls_rlc_weights_launch((unsigned)n, c + o_seed, W, s));
  return NBLS_OK;
}
// B = the sum of its three parts with B's own zero flag (A and its flag are in place), then the combined check of the two points against the two tables
int KzgFrame::decide(int* all_ok, int8_t* status, bool* more) {
  const uint8_t* got; int r;
  uint8_t* BN = PR + a.bn;
  if ((r = sum3_affine(ctx, 1, B3, BST, PR + a.bj, BN, BN + RAW, PT2 + 96, kzg_hdr_b_zero(BK), s)) || (r = combined_tail(ctx, 2, 0, PT2, A_ZERO, TB, PR + a.res, hdr_one(BK), s)) ||
      (r = io.fetch(BK, back_bytes(n), &got)))
    return r;
  const KzgVerdict v = kzg_verdict(got, n);
  if (v == KZG_BAD_G2) return NBLS_EDECODE;
  combined_result(v == KZG_ACCEPT, n, all_ok, status, more);
  return NBLS_OK;
}
int KzgFrame::items_begin(size_t front, uint8_t** FRONT, MsmbPlan* rows_plan, size_t row_pts) {
  size_t sz = 0; uint8_t* IT; int r;
  const size_t b_front = carve(&sz, front), b_t = kzg_item_tail_carve(n, &sz, &t);
  if ((r = need(ctx, sb_items, sz, &IT)) || (r = ensure_scratch(ctx, 2 * n)) || (rows_plan && (r = msm_rows_dev_plan(ctx, row_pts, n, rows_plan)))) return r;
  *FRONT = IT + b_front; TAIL = IT + b_t; P3 = TAIL + t.p3; ST3 = TAIL + t.st3;
  guard.armed = true;   // (until statuses_back)
  return NBLS_OK;
}
int KzgFrame::items_close(const uint8_t* proofs96, const uint8_t* proof_st, int* all_ok, int8_t* status) {
  const int r = kzg_item_tail(ctx, n, t, TAIL, proofs96, TB, PRE, proof_st, s); if (r) return r;
  return statuses_back(ctx, s, TAIL + t.fs, n, guard, all_ok, status);
}
