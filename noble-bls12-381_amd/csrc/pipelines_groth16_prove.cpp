// pipelines_groth16_prove.cpp -- the Groth16 prover on BLS12-381 (include/nbls.h has the contract, g16p_exec.h the statement, the quotient and the lane code): from a witness
// z = (1, x_1 .. x_m, aux ..) and the blinding scalars (r, s) to the 192 bytes A || B || C that nbls_groth16_verify reads, against a proving key that stays on the device.
// The handle (nbls_groth16_pk) is one device block: the three R1CS matrices in CSR form with Montgomery coefficients, the rows ordered by length, the four affine point
// arrays the sums read
//   a_query | alpha_g1 | delta_g1        b_g1_query | beta_g1 | delta_g1        b_g2_query | beta_g2 | delta_g2        l_query | h_query | [slot A] | [slot B1] | delta_g1
// a mask byte per query point (a zero point of the key: a subgroup point stands in, the scalar is forced to zero), and the workspace of ONE proof -- no scratch slot of the
// context is taken: the sums run on MSM_MAIN's slots, which hold SB_STAGED, so the witness is staged inside the handle as well; the transforms touch SB_NTTL_FLAGS alone.
// One chain per witness on the context's stream:
//   H2D copy of z | r | s -> g16p_witness_kernel: canonical check, z to limbs, z_0 == 1 -> g16p_spmv_kernel: a, b, c at rev(j), the flag a_j b_j == c_j
//            -> nbls_fr_ntt_dev x 3 rows to coefficients -> x 3 rows to the values on the coset of 7 -> g16p_quotient_kernel -> one row back to coefficients: h
//            -> g16p_scalars_kernel: (z | 1 | r), (z | 1 | s), (z_aux | h | s | r | -r s), masked; all zero for a refused witness
//            -> dev_msm x 4: A into slot A, B1 into slot B1 (the generator where a sum is the zero point: the flag decides), B in G2, C
//            -> P_G1_COMPRESS / P_G2_COMPRESS -> g16p_finish_kernel: the status, 192 zero bytes where it is not 0
// and behind the last witness one D2H copy of all proofs and statuses.  The witness and (r, s) are secrets: G16pWipe zeroes the handle's copies, the scalars and the
// page-locked block on every way out.  nbls_groth16_quotient is the middle of the chain on caller-chosen vectors, staged as nbls_fr_ntt_large stages (SB_STAGED, SB_KZGC_OUT).
#include "nbls_internal.h"
// (g16p_quot_factor runs on the host here: its inversion's loop asks for an unrolling that the host pass declines, which is all the warning says)
#pragma clang diagnostic ignored "-Wpass-failed"
#include "g16p_exec.h"
#include <algorithm>
#include <errno.h>
#include <sys/random.h>

static const size_t G16P_MAX_WITNESSES = (size_t)1 << 16, G16P_MAX_ENTRIES = (size_t)1 << 24, G16P_MAX_SUM = (size_t)1 << 22;   // (dev_msm's bound on one sum)
static const unsigned G16P_MAX_LOG2 = 21, G16P_QUOT_MAX_LOG2 = 22;

struct G16pMat { uint32_t *rows = nullptr, *cols = nullptr; uint8_t* vals = nullptr; };
struct nbls_groth16_pk {
  int device = 0; unsigned log2_n = 0; size_t n_vars = 0, n_public = 0;
  std::mutex mu;                  // one proof at a time: the workspace below is the handle's
  std::vector<uint32_t> lens;     // the rows' lengths (the longest of a row's three lists), longest first: the rows of at least T entries are the first lower_bound of them
  uint8_t* mem = nullptr;
  G16pMat m[3]; uint32_t* order = nullptr;
  uint8_t *pa = nullptr, *pb1 = nullptr, *pb2 = nullptr, *pc = nullptr, *mask_a = nullptr, *mask_b = nullptr, *mask_l = nullptr, *shift = nullptr;
  // the workspace: secret .. secret + secret_bytes holds w32 (z | r | s as sent), z (limbs), v32 (a | b | c, then h in a's place), sa, sb, sc
  uint8_t *secret = nullptr, *w32 = nullptr, *z = nullptr, *v32 = nullptr, *sa = nullptr, *sb = nullptr, *sc = nullptr, *flags = nullptr, *st3 = nullptr, *zero4 = nullptr,
          *b2aff = nullptr, *caff = nullptr;
  size_t secret_bytes = 0;
};

static unsigned g16p_tail_bits(const nbls_ctx* ctx) { return ctx->ntt_tail_bits ? ctx->ntt_tail_bits : FR_NTTL_DEFAULT_TAIL; }
static bool g16p_ntt_ok(const nbls_ctx* ctx, unsigned log2_n) { return log2_n <= g16p_tail_bits(ctx) || log2_n - g16p_tail_bits(ctx) <= 12; }   // (nbls_fr_ntt_dev's rule, asked before any device work)
static bool is_zero_point(const uint8_t* p, size_t bytes) {
  if (p[0] != 0xc0) return false;
  for (size_t i = 1; i < bytes; i++) if (p[i]) return false;
  return true;
}

EXPORT void nbls_groth16_pk_destroy(nbls_groth16_pk* pk) {
  if (!pk) return;
  handle_free(pk->device, {pk->mem});
  delete pk;
}
EXPORT int nbls_groth16_pk_params(const nbls_groth16_pk* pk, unsigned* log2_n, size_t* n_vars, size_t* n_public) {
  if (!pk || !log2_n || !n_vars || !n_public) return NBLS_EINVAL;
  *log2_n = pk->log2_n; *n_vars = pk->n_vars; *n_public = pk->n_public;
  return NBLS_OK;
}

// for tests: *wiped = 1 when every byte of the handle's secret arrays (the staged witness and (r, s), z, the three vectors and h, the three scalar arrays) reads back as zero
EXPORT int nbls_groth16_pk_wiped(nbls_ctx* ctx, nbls_groth16_pk* pk, int* wiped) {
  WHOLE_CALL(ctx);
  if (!ctx || !pk || !wiped || pk->device != ctx->device) return NBLS_EINVAL;
  std::lock_guard<std::mutex> proving(pk->mu);
  std::vector<uint8_t> got(pk->secret_bytes);
  LOCKED(ctx);
  HIPCHK(hipMemcpyAsync(got.data(), pk->secret, pk->secret_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *wiped = std::all_of(got.begin(), got.end(), [](uint8_t b) { return b == 0; }) ? 1 : 0;
  return NBLS_OK;
}

// one matrix on the host: the offsets padded to N + 1, the coefficients in Montgomery form.  false: the descriptor's arrays break a rule of the header
struct G16pHostMat { std::vector<uint32_t> rows; std::vector<Fr> vals; const uint32_t* cols = nullptr; size_t nnz = 0; };
static bool g16p_host_matrix(size_t N, size_t n_cons, size_t n_vars, const uint32_t* rows, const uint32_t* cols, const uint8_t* vals32, G16pHostMat* o) {
  if (rows[0] != 0) return false;
  for (size_t j = 0; j < n_cons; j++) if (rows[j + 1] < rows[j]) return false;
  o->nnz = rows[n_cons];
  if (o->nnz > G16P_MAX_ENTRIES || (o->nnz && (!cols || !vals32))) return false;
  o->rows.assign(N + 1, (uint32_t)o->nnz);
  std::copy(rows, rows + n_cons + 1, o->rows.begin());
  o->cols = cols;
  o->vals.resize(o->nnz);
  for (size_t k = 0; k < o->nnz; k++) {
    if (cols[k] >= n_vars || fr_ge_r_mask(fr_load_be(vals32 + 32 * k))) return false;
    o->vals[k] = fr_from_bytes(vals32 + 32 * k);
  }
  return true;
}

static int g16p_pk_build(nbls_ctx* ctx, nbls_groth16_pk* pk, const nbls_groth16_pk_desc* d, const G16pHostMat* hm, const std::vector<uint32_t>& order, int8_t* status) {
  const size_t N = (size_t)1 << d->log2_n, nv = d->n_vars, na = nv - d->n_public - 1, n1 = 3 + 2 * nv + na + N - 1, n2 = 2 + nv, row = N * 32;
  // the compressed points as two arrays for the two decoder calls: alpha | beta_g1 | delta_g1 | a_query | b_g1_query | l_query | h_query, and beta_g2 | delta_g2 | b_g2_query
  std::vector<uint8_t> h48(n1 * 48), h96(n2 * 96);
  std::vector<int8_t> st(n1 + n2);
  uint8_t* p = h48.data();
  memcpy(p, d->alpha_g1_48, 48); memcpy(p + 48, d->beta_g1_48, 48); memcpy(p + 96, d->delta_g1_48, 48); p += 144;
  memcpy(p, d->a_query48, nv * 48); p += nv * 48;
  memcpy(p, d->b_g1_query48, nv * 48); p += nv * 48;
  if (na) memcpy(p, d->l_query48, na * 48);
  p += na * 48;
  memcpy(p, d->h_query48, (N - 1) * 48);
  memcpy(h96.data(), d->beta_g2_96, 96); memcpy(h96.data() + 96, d->delta_g2_96, 96); memcpy(h96.data() + 192, d->b_g2_query96, nv * 96);
  uint8_t g2gen[192], sevens[96] = {0};
  g2_wire_negate(neg_g2_wire(), g2gen);
  sevens[31] = sevens[63] = sevens[95] = 7;
  LOCKED(ctx);
  HostIO io{ctx};
  void *d48 = io.alloc(n1 * 48), *d96 = io.alloc(n2 * 96), *a1 = io.alloc(n1 * 96), *a2 = io.alloc(n2 * 192), *dst = io.alloc(n1 + n2), *junk = io.alloc(nv);
  if (!d48 || !d96 || !a1 || !a2 || !dst || !junk) return NBLS_EHIP;
  size_t sz = 0, o_m[3][3];
  for (int k = 0; k < 3; k++) { o_m[k][0] = carve(&sz, (N + 1) * 4); o_m[k][1] = carve(&sz, (hm[k].nnz + 1) * 4); o_m[k][2] = carve(&sz, (hm[k].nnz + 1) * 32); }
  const size_t o_ord = carve(&sz, N * 4), o_pa = carve(&sz, (nv + 2) * 96), o_pb1 = carve(&sz, (nv + 2) * 96), o_pb2 = carve(&sz, (nv + 2) * 192), o_pc = carve(&sz, (na + N + 2) * 96),
               o_ma = carve(&sz, nv), o_mb = carve(&sz, nv), o_ml = carve(&sz, na + 1), o_g2 = carve(&sz, 192), o_sh = carve(&sz, 96), o_w = carve(&sz, (nv + 2) * 32), o_z = carve(&sz, nv * 32),
               o_v = carve(&sz, 3 * row), o_sa = carve(&sz, (nv + 2) * 32), o_sb = carve(&sz, (nv + 2) * 32), o_sc = carve(&sz, (na + N + 2) * 32), o_end = sz, o_fl = carve(&sz, G16P_FLAGS),
               o_st3 = carve(&sz, 4), o_z4 = carve(&sz, 4), o_b2 = carve(&sz, 192), o_c = carve(&sz, 96);
  HIPCHK(hipMalloc(&pk->mem, sz));   // (freed by the caller's nbls_groth16_pk_destroy on every error return)
  uint8_t* M = pk->mem;
  for (int k = 0; k < 3; k++) pk->m[k] = G16pMat{(uint32_t*)(M + o_m[k][0]), (uint32_t*)(M + o_m[k][1]), M + o_m[k][2]};
  pk->order = (uint32_t*)(M + o_ord); pk->pa = M + o_pa; pk->pb1 = M + o_pb1; pk->pb2 = M + o_pb2; pk->pc = M + o_pc; pk->mask_a = M + o_ma; pk->mask_b = M + o_mb; pk->mask_l = M + o_ml;
  pk->shift = M + o_sh; pk->secret = pk->w32 = M + o_w; pk->z = M + o_z; pk->v32 = M + o_v; pk->sa = M + o_sa; pk->sb = M + o_sb; pk->sc = M + o_sc; pk->secret_bytes = o_end - o_w;
  pk->flags = M + o_fl; pk->st3 = M + o_st3; pk->zero4 = M + o_z4; pk->b2aff = M + o_b2; pk->caff = M + o_c;
  uint8_t* G2FIX = M + o_g2;
  int r;
  HIPCHK(hipMemcpyAsync(d48, h48.data(), n1 * 48, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d96, h96.data(), n2 * 96, hipMemcpyHostToDevice, s));
  if ((r = dev_decompress(ctx, false, n1, d48, a1, dst, s)) || (r = dev_decompress(ctx, true, n2, d96, a2, (uint8_t*)dst + n1, s))) return r;
  HIPCHK(hipMemcpyAsync(st.data(), dst, n1 + n2, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // the decoder's arrays: G1 fixed 0 .. 2, a_query at 3, b_g1_query at 3 + nv, l_query at 3 + 2 nv, h_query behind; G2 fixed at n1, b_g2_query at n1 + 2
  const int8_t *st_a = st.data() + 3, *st_b1 = st_a + nv, *st_l = st_b1 + nv, *st_h = st_l + na, *st_b2 = st.data() + n1 + 2;
  if (status) {
    status[0] = st[0]; status[1] = st[1]; status[2] = st[n1]; status[3] = st[2]; status[4] = st[n1 + 1];
    int8_t* q = status + 5;
    memcpy(q, st_a, nv); memcpy(q + nv, st_b1, nv); memcpy(q + 2 * nv, st_b2, nv); memcpy(q + 3 * nv, st_l, na); memcpy(q + 3 * nv + na, st_h, N - 1);
  }
  bool bad = st[0] || st[1] || st[2] || st[n1] || st[n1 + 1];
  for (size_t i = 0; i < N - 1; i++) bad = bad || st_h[i] != 0;
  for (size_t i = 0; i < 2 * nv + na; i++) bad = bad || st_a[i] > 1 || st_a[i] < 0;
  for (size_t i = 0; i < nv; i++) bad = bad || st_b2[i] > 1 || st_b2[i] < 0;
  if (bad) return NBLS_EDECODE;
  // the four arrays, device to device
  const uint8_t *A1 = (const uint8_t*)a1, *A2 = (const uint8_t*)a2, *dq = (const uint8_t*)dst;
  auto put = [&](uint8_t* to, const uint8_t* from, size_t bytes) { return bytes ? hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess; };
  HIPCHK(put(pk->pa, A1 + 3 * 96, nv * 96)); HIPCHK(put(pk->pa + nv * 96, A1, 96)); HIPCHK(put(pk->pa + (nv + 1) * 96, A1 + 2 * 96, 96));
  HIPCHK(put(pk->pb1, A1 + (3 + nv) * 96, nv * 96)); HIPCHK(put(pk->pb1 + nv * 96, A1 + 96, 96)); HIPCHK(put(pk->pb1 + (nv + 1) * 96, A1 + 2 * 96, 96));
  HIPCHK(put(pk->pb2, A2 + 2 * 192, nv * 192)); HIPCHK(put(pk->pb2 + nv * 192, A2, 2 * 192));
  HIPCHK(put(pk->pc, A1 + (3 + 2 * nv) * 96, (na + N - 1) * 96));
  uint8_t* SLOTS = pk->pc + (na + N - 1) * 96;
  HIPCHK(put(SLOTS, ctx->gen_g1, 96)); HIPCHK(put(SLOTS + 96, ctx->gen_g1, 96)); HIPCHK(put(SLOTS + 192, A1 + 2 * 96, 96));
  HIPCHK(hipMemcpyAsync(G2FIX, g2gen, 192, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(pk->shift, sevens, 96, hipMemcpyHostToDevice, s));
  LAUNCHCHK(nbls_g16p_mask_launch(nv, 96, dq + 3, ctx->gen_g1, pk->pa, pk->mask_a, s));
  LAUNCHCHK(nbls_g16p_mask_launch(nv, 96, dq + 3 + nv, ctx->gen_g1, pk->pb1, pk->mask_b, s));
  LAUNCHCHK(nbls_g16p_mask_launch(nv, 192, dq + n1 + 2, G2FIX, pk->pb2, junk, s));   // (the same mask as b_g1_query's: the two were checked to agree)
  LAUNCHCHK(nbls_g16p_mask_launch(na, 96, dq + 3 + 2 * nv, ctx->gen_g1, pk->pc, pk->mask_l, s));
  for (int k = 0; k < 3; k++) {
    HIPCHK(hipMemcpyAsync(pk->m[k].rows, hm[k].rows.data(), (N + 1) * 4, hipMemcpyHostToDevice, s));
    if (hm[k].nnz) {
      HIPCHK(hipMemcpyAsync(pk->m[k].cols, hm[k].cols, hm[k].nnz * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(pk->m[k].vals, hm[k].vals.data(), hm[k].nnz * 32, hipMemcpyHostToDevice, s));
    }
  }
  HIPCHK(hipMemcpyAsync(pk->order, order.data(), N * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(pk->secret, 0, pk->secret_bytes, s));
  HIPCHK(hipStreamSynchronize(s));   // (the host arrays are read by the copies until here; an error return waits in ~HostIO)
  return NBLS_OK;
}

EXPORT int nbls_groth16_pk_create(nbls_ctx* ctx, const nbls_groth16_pk_desc* d, int8_t* status, nbls_groth16_pk** out) {
  WHOLE_CALL(ctx);
  if (out) *out = nullptr;
  if (!ctx || !d || !out || d->log2_n < 1 || d->log2_n > G16P_MAX_LOG2 || !d->n_public || d->n_vars <= d->n_public) return NBLS_EINVAL;
  const size_t N = (size_t)1 << d->log2_n, nv = d->n_vars, na = nv - d->n_public - 1;
  if (d->n_constraints > N || na + N + 2 > G16P_MAX_SUM || nv + 2 > G16P_MAX_SUM || !d->a_rows || !d->b_rows || !d->c_rows || !d->alpha_g1_48 || !d->beta_g1_48 || !d->beta_g2_96 ||
      !d->delta_g1_48 || !d->delta_g2_96 || !d->a_query48 || !d->b_g1_query48 || !d->b_g2_query96 || (na && !d->l_query48) || !d->h_query48)
    return NBLS_EINVAL;
  G16pHostMat hm[3];
  if (!g16p_host_matrix(N, d->n_constraints, nv, d->a_rows, d->a_cols, d->a_vals32, &hm[0]) || !g16p_host_matrix(N, d->n_constraints, nv, d->b_rows, d->b_cols, d->b_vals32, &hm[1]) ||
      !g16p_host_matrix(N, d->n_constraints, nv, d->c_rows, d->c_cols, d->c_vals32, &hm[2]))
    return NBLS_EINVAL;
  for (size_t i = 0; i < nv; i++) if (is_zero_point(d->b_g1_query48 + 48 * i, 48) != is_zero_point(d->b_g2_query96 + 96 * i, 96)) return NBLS_EINVAL;
  // the rows, longest first (a stable sort: rows of one length keep their order, so neighbours in the matrix stay neighbours in a wavefront)
  std::vector<uint32_t> len(N), order(N);
  for (size_t j = 0; j < N; j++) {
    len[j] = std::max({hm[0].rows[j + 1] - hm[0].rows[j], hm[1].rows[j + 1] - hm[1].rows[j], hm[2].rows[j + 1] - hm[2].rows[j]});
    order[j] = (uint32_t)j;
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return len[x] > len[y]; });
  return handle_create(ctx, out, nbls_groth16_pk_destroy, [&](nbls_groth16_pk* pk) {
    pk->log2_n = d->log2_n; pk->n_vars = nv; pk->n_public = d->n_public;
    pk->lens.resize(N);
    for (size_t j = 0; j < N; j++) pk->lens[j] = len[order[j]];
    return g16p_pk_build(ctx, pk, d, hm, order, status);
  });
}

// The quotient of n triples on the device, in place: A, B, C hold n rows of 2^L values each (16-byte aligned; they need not be adjacent), shift: n elements 7, st3: 3 n bytes.
// -> the coefficients of h in A's rows where `out` is NULL, else in out (disjoint from A); st3 = the statuses of the first transform (rows of A | of B | of C)
static int g16p_quotient_dev(nbls_ctx* ctx, unsigned L, size_t n, uint8_t* A, uint8_t* B, uint8_t* C, const uint8_t* shift, uint8_t* st3, uint8_t* out, hipStream_t s) {
  uint8_t* V[3] = {A, B, C}; int r;
  for (int k = 0; k < 3; k++) if ((r = nbls_fr_ntt_dev(ctx, L, NBLS_NTT_TO_COEFFS, n, V[k], nullptr, V[k], st3 + k * n, s))) return r;
  for (int k = 0; k < 3; k++) if ((r = nbls_fr_ntt_dev(ctx, L, NBLS_NTT_TO_EVALS, n, V[k], shift, V[k], nullptr, s))) return r;
  const Fr kinv = g16p_quot_factor(L);
  LAUNCHCHK(nbls_g16p_quotient_launch(L, n, A, B, C, st3, kinv.l, s));
  return nbls_fr_ntt_dev(ctx, L, NBLS_NTT_TO_COEFFS, n, A, shift, out ? out : A, nullptr, s);
}

EXPORT int nbls_groth16_quotient(nbls_ctx* ctx, unsigned log2_n, size_t n, const uint8_t* a32, const uint8_t* b32, const uint8_t* c32, uint8_t* out_h32, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || log2_n < 1 || log2_n > G16P_QUOT_MAX_LOG2 || !g16p_ntt_ok(ctx, log2_n) || n > (KZG_MAX_ELEMS >> log2_n) || (n && (!a32 || !b32 || !c32 || !out_h32))) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  std::vector<uint8_t> sevens(n * 32, 0);
  for (size_t i = 0; i < n; i++) sevens[32 * i + 31] = 7;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const size_t qb = (n * 32) << log2_n, o_a = io.bytes(a32, qb), o_b = io.bytes(b32, qb), o_c = io.bytes(c32, qb), o_sh = io.bytes(sevens.data(), n * 32), back = qb + n;
  size_t sz = 0;
  const size_t a_out = carve(&sz, back), a_st3 = carve(&sz, 3 * n), a_vio = carve(&sz, n);
  uint8_t *c, *O; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_KZGC_OUT, sz, &O)) || (r = io.send(c, back))) return r;
  HIPCHK(hipMemsetAsync(O + a_vio, 0, n, s));
  LAUNCHCHK(nbls_g16p_check_launch(log2_n, n, c + o_a, c + o_b, c + o_c, O + a_vio, s));
  if ((r = g16p_quotient_dev(ctx, log2_n, n, c + o_a, c + o_b, c + o_c, c + o_sh, O + a_st3, O + a_out, s))) return r;
  LAUNCHCHK(nbls_g16p_quot_status_launch(n, O + a_st3, O + a_vio, O + a_out + qb, s));
  return io.fetch_to(O + a_out, out_h32, qb, status, n);
}

// uniform below r from the OS: 32 bytes masked to 255 bits, redrawn while >= r
static int g16p_random_scalar(uint8_t* out32) {
  for (;;) {
    const int r = os_seed(out32);
    if (r) return r;
    out32[0] &= 0x7f;
    if (!fr_ge_r_mask(fr_load_be(out32))) return NBLS_OK;
  }
}
// the prover's secrets on every way out of nbls_groth16_prove: behind a wait for the device, the handle's copies and the scalars are zeroed and the page-locked block wiped
struct G16pWipe {
  nbls_ctx* ctx; nbls_groth16_pk* pk; size_t host_bytes; bool done = false;
  ~G16pWipe() {
    if (!done) { (void)hipDeviceSynchronize(); (void)hipMemset(pk->secret, 0, pk->secret_bytes); }
    if (ctx->pinned && host_bytes <= ctx->pinned_cap) memset(ctx->pinned, 0, host_bytes);
  }
};

EXPORT int nbls_groth16_prove(nbls_ctx* ctx, nbls_groth16_pk* pk, size_t n, const uint8_t* witness32, const uint8_t* rs32, uint8_t* out_proofs192, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !pk || !n || n > G16P_MAX_WITNESSES || !witness32 || !out_proofs192 || pk->device != ctx->device || !g16p_ntt_ok(ctx, pk->log2_n)) return NBLS_EINVAL;
  const unsigned L = pk->log2_n;
  const size_t N = (size_t)1 << L, nv = pk->n_vars, na = nv - pk->n_public - 1, wb = (nv + 2) * 32, row = N * 32, back = n * 192 + n;
  std::vector<uint8_t> drawn;
  if (!rs32) {
    drawn.resize(n * 64);
    for (size_t i = 0; i < 2 * n; i++) { const int r = g16p_random_scalar(drawn.data() + 32 * i); if (r) { std::fill(drawn.begin(), drawn.end(), 0); return r; } }
    rs32 = drawn.data();
  }
  struct DrawnWipe { std::vector<uint8_t>& v; ~DrawnWipe() { std::fill(v.begin(), v.end(), 0); } } drawn_wipe{drawn};
  std::lock_guard<std::mutex> proving(pk->mu);
  // the rows of at least T entries: the head of the handle's order
  const size_t T = ctx->g16p_row_wave ? ctx->g16p_row_wave : (size_t)G16P_ROW_WAVE_DEFAULT;
  const unsigned n_wave = (unsigned)(std::lower_bound(pk->lens.begin(), pk->lens.end(), T, [](uint32_t len, size_t t) { return len >= t; }) - pk->lens.begin());
  const void* mats[9];
  for (int k = 0; k < 3; k++) { mats[3 * k] = pk->m[k].rows; mats[3 * k + 1] = pk->m[k].cols; mats[3 * k + 2] = pk->m[k].vals; }
  const G16pScalars S{nv, pk->n_public, N, pk->w32, pk->v32, pk->mask_a, pk->mask_b, pk->mask_l, pk->flags, pk->sa, pk->sb, pk->sc};
  uint8_t *SLOT_A = pk->pc + (na + N - 1) * 96, *SLOT_B1 = SLOT_A + 96, *Z4 = pk->zero4;   // Z4: the zero flags of A, B, C, B1
  DEV_ENTER(ctx, nullptr);
  HostIO io{ctx};
  uint8_t* O = (uint8_t*)io.alloc(back);
  int r;
  if (!O) return NBLS_EHIP;
  if ((r = ensure_pinned(ctx, wb)) || (r = ensure_pinned_out(ctx, back))) return r;
  G16pWipe wipe{ctx, pk, wb};
  for (size_t i = 0; i < n; i++) {
    if (i) HIPCHK(hipStreamSynchronize(s));   // (the copy of the witness before still reads the page-locked block)
    memcpy(ctx->pinned, witness32 + i * nv * 32, nv * 32);
    memcpy(ctx->pinned + nv * 32, rs32 + 64 * i, 64);
    HIPCHK(hipMemcpyAsync(pk->w32, ctx->pinned, wb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(pk->flags, 0, G16P_FLAGS, s));
    LAUNCHCHK(nbls_g16p_witness_launch(nv, pk->w32, pk->z, pk->flags, s));
    LAUNCHCHK(nbls_g16p_spmv_launch(L, n_wave, pk->order, mats, pk->z, pk->v32, pk->flags, s));
    if ((r = g16p_quotient_dev(ctx, L, 1, pk->v32, pk->v32 + row, pk->v32 + 2 * row, pk->shift, pk->st3, nullptr, s))) return r;
    LAUNCHCHK(nbls_g16p_scalars_launch(&S, s));
    if ((r = dev_msm(ctx, false, nv + 2, pk->pa, pk->sa, 0, SLOT_A, Z4, s))) return r;
    LAUNCHCHK(nbls_agg_fix_zero_launch(1, Z4, ctx->gen_g1, SLOT_A, nullptr, s));
    if ((r = dev_msm(ctx, false, nv + 2, pk->pb1, pk->sb, 0, SLOT_B1, Z4 + 3, s))) return r;
    LAUNCHCHK(nbls_agg_fix_zero_launch(1, Z4 + 3, ctx->gen_g1, SLOT_B1, nullptr, s));
    if ((r = dev_msm(ctx, true, nv + 2, pk->pb2, pk->sb, 0, pk->b2aff, Z4 + 1, s)) || (r = dev_msm(ctx, false, na + N + 2, pk->pc, pk->sc, 0, pk->caff, Z4 + 2, s))) return r;
    uint8_t* P = O + 192 * i;
    if ((r = run(ctx, P_G1_COMPRESS, 1, {B(0, SLOT_A, 96), B(2, P, 48)}, s)) || (r = run(ctx, P_G2_COMPRESS, 1, {B(0, pk->b2aff, 192), B(2, P + 48, 96)}, s)) ||
        (r = run(ctx, P_G1_COMPRESS, 1, {B(0, pk->caff, 96), B(2, P + 144, 48)}, s)))
      return r;
    LAUNCHCHK(nbls_g16p_finish_launch(pk->flags, Z4, P, O + 192 * n + i, s));
  }
  HIPCHK(hipMemsetAsync(pk->secret, 0, pk->secret_bytes, s));
  HIPCHK(hipMemcpyAsync(ctx->pinned_out, O, back, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  wipe.done = true;
  memcpy(out_proofs192, ctx->pinned_out, n * 192);
  if (status) memcpy(status, ctx->pinned_out + n * 192, n);
  return NBLS_OK;
}
