// pipelines_codec.cpp -- validity, decoders / encoders, hash-to-curve, point sums, scalar multiplication and sign (reference index.ts:207-327, 359-448, 481-690, 738-752, 771-788).
#include "nbls_internal.h"

// ================================================================================================================
// Validity, decoders, hash-to-G2, point sums, verifyBatch.  Device-side pipelines (dev_*) work on device pointers and
// enqueue on `s`; the exported wrappers stage host buffers.
// ================================================================================================================
int dev_validate(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, void* d_status, hipStream_t s) {
  return g2 ? run(ctx, P_G2_VALIDATE, n, {B(1, d_pts, 192), B(7, d_status, 1)}, s) : run(ctx, P_G1_VALIDATE, n, {B(0, d_pts, 96), B(7, d_status, 1)}, s);
}
// PointG1.fromHex (48 B) / PointG2.fromSignature (96 B): compressed -> affine wire bytes + status
// sl: the scratch slots of this instance (three arrays and the exponentiation table), so that two chains can run on different streams at the same time
// mode (G2 only): 0 fromSignature 96 B, 1 fromSignature 192 B, 2 fromHex 96 B (no subgroup check, flag rules)
// io / ntot: the call works on items [io, io + n) of scratch arrays sized for ntot items (verify_pipeline: sub-batches of one call run side by side on slices of the same arrays)
int dev_decompress(nbls_ctx* ctx, bool g2, size_t n, const void* d_in, void* d_out, void* d_status, hipStream_t s, const DecSlots& sl, int mode, size_t io, size_t ntot) {
  const size_t e = g2 ? (mode == 1 ? 192 : 96) : 48, q = g2 ? 2 * RAW : RAW, pq = POW_TAB * (g2 ? 2 : 1) * RAW;
  if (ntot < io + n) ntot = io + n;
  uint8_t *X, *R, *Cd, *pw; int r;
  if ((r = need(ctx, sl.x, ntot * q, &X)) || (r = need(ctx, sl.r, ntot * q, &R)) || (r = need(ctx, sl.c, ntot * q, &Cd)) || (r = need(ctx, sl.pow, ntot * pq, &pw))) return r;
  X += io * q; R += io * q; Cd += io * q; pw += io * pq;
  const ProgId pa = !g2 ? P_G1_DEC_A : mode == 1 ? P_G2_DEC_A192 : P_G2_DEC_A, pb = !g2 ? P_G1_DEC_B : mode == 1 ? P_G2_DEC_B192 : mode == 2 ? P_G2_DEC_B_HEX : P_G2_DEC_B;
  if ((r = run(ctx, pa, n, {B(0, d_in, e), B(3, X, q), B(4, R, q)}, s))) return r;
  if ((r = run_pow(ctx, g2 ? 1 : 0, n, R, Cd, s, pw))) return r;
  return run(ctx, pb, n, {B(0, d_in, e), B(3, X, q), B(4, R, q), B(5, Cd, q), B(6, d_out, g2 ? 192 : 96), B(7, d_status, 1)}, s);
}
// raw projective points -> affine wire bytes + status (1 = the zero point): [norm of Z ->] inversion -> affine program.  norm = false: an earlier program has left the norms in N
int to_affine(nbls_ctx* ctx, bool g2, size_t n, const void* Pj, void* N, void* NI, void* d_out, void* d_status, hipStream_t s, bool norm) {
  const size_t p = g2 ? 6 * RAW : 3 * RAW; int r;
  if (norm && (r = run(ctx, g2 ? P_G2_NORM : P_G1_NORM, n, {B(3, Pj, p), B(4, N, RAW)}, s))) return r;
  if ((r = run_inv_buf(ctx, n, N, NI, s))) return r;
  return run(ctx, g2 ? P_G2_TO_AFFINE : P_G1_TO_AFFINE, n, {B(3, Pj, p), B(4, NI, RAW), B(2, d_out, g2 ? 192 : 96), B(7, d_status, 1)}, s);
}
// 256 uniform bytes per message (expand_message_xmd output) -> hash point, affine wire bytes (PointG2.hashToCurve, index.ts:481-490)
// PointG2.clearCofactor (index.ts:659-672) on raw projective points: three programs: the t1-independent points, then one around each multiplication by x (programs.h P_H2C_C0 / C1 / C2).
// in -> out (may alias in or base), norm of Z -> N; base and S are scratch of n * 6 raw elements each, and `in` is scratch too from the second program on (t1 is stored over P)
int dev_clear_g2(nbls_ctx* ctx, size_t n, void* in, uint8_t* base, uint8_t* S, void* out, void* N, hipStream_t s) {
  int r = run(ctx, P_H2C_C0, n, {B(3, in, 6 * RAW), B(6, base, 6 * RAW), B(5, S, 6 * RAW)}, s); if (r) return r;     // v = psi(P) -> base, u = psi^2(2P) - psi(P) - P -> S
  if ((r = run(ctx, pt_ls2_variant(ctx, P_H2C_C1, n), n, {B(3, in, 6 * RAW), B(6, base, 6 * RAW)}, s))) return r;                          // base = t1 + v over v, t1 = -[x]P over P
  // out may be in: every item reads its t1 before its result is stored
  return run(ctx, pt_ls2_variant(ctx, P_H2C_C2, n), n, {B(3, base, 6 * RAW), B(4, in, 6 * RAW), B(5, S, 6 * RAW), B(6, out, 6 * RAW), B(7, N, RAW)}, s);
}
// io / ntot: see dev_decompress; proj: stop at the raw projective points (SB_WORK_B) -- the caller multiplies them (sign) and normalises once, at the end
int dev_hash_to_g2(nbls_ctx* ctx, size_t n, const void* d_uniform, void* d_out, hipStream_t s, size_t io, size_t ntot, uint8_t** proj) {
  if (ntot < io + n) ntot = io + n;
  uint8_t *T, *E, *Pw, *Q, *N, *NI, *st, *St, *Pt2, *S, *tab; int r;
  const size_t ST = 32;   // raw elements of SWU state per message: 2 x 12 (P_H2C_A) or 2 x 16 (P_H2C_NA / NM)
  if ((r = need(ctx, SB_WORK_A, ntot * 4 * RAW, &T)) || (r = need(ctx, SB_WORK_B, ntot * 6 * RAW, &E)) || (r = need(ctx, SB_WORK_C, ntot * 4 * RAW, &Pw)) ||
      (r = need(ctx, SB_WORK_D, ntot * 6 * RAW, &Q)) || (r = need(ctx, SB_NORM, ntot * RAW, &N)) || (r = need(ctx, SB_NORM_INV, ntot * RAW, &NI)) || (r = need(ctx, SB_POINT_ST, ntot, &st)) ||
      (r = need(ctx, SB_SWU_STATE, ntot * ST * RAW, &St)) || (r = need(ctx, SB_SWU_POINTS, ntot * 12 * RAW, &Pt2)) || (r = need(ctx, SB_CLEAR_S, ntot * 6 * RAW, &S)) ||
      (r = need(ctx, SB_POW_TABLE, ntot * 4 * POW_TAB * RAW, &tab))) return r;
  T += io * 4 * RAW; E += io * 6 * RAW; Pw += io * 4 * RAW; Q += io * 6 * RAW; N += io * RAW; NI += io * RAW; st += io; St += io * ST * RAW; Pt2 += io * 12 * RAW; S += io * 6 * RAW;
  tab += io * 4 * POW_TAB * RAW;
  if (ntot >= ctx->h2c_norm_min) {   // ntot: the messages of the whole call (verifyBatch hashes its sub-batches side by side)
    // The SWU square root by the norm method (codec.h swu_norm_*): two Fp exponentiations with a short program between them where the Fp2 form spends one exponentiation of
    // twice the work.  Same points (the root's sign is fixed by sgn0 afterwards); two more launches, so single messages keep the Fp2 form.
    if ((r = run(ctx, P_H2C_NA, n, {B(0, d_uniform, 256), B(3, T, 4 * RAW), B(4, E, 2 * RAW), B(5, St, 32 * RAW)}, s))) return r;
    if ((r = run_pow(ctx, 0, 2 * n, E, Pw, s, tab))) return r;                                        // n = N(a)^((p+1)/4)
    if ((r = run(ctx, P_H2C_NM, 2 * n, {B(3, T, 2 * RAW), B(4, St, 16 * RAW), B(5, Pw, RAW), B(6, St + 9 * RAW, 16 * RAW), B(7, E, RAW)}, s))) return r;
    if ((r = run_pow(ctx, 3, 2 * n, E, Pw, s, tab))) return r;                                        // e = (delta d^3)^((p-3)/4)
    if ((r = run(ctx, P_H2C_NB, 2 * n, {B(3, T, 2 * RAW), B(4, St, 16 * RAW), B(5, Pw, RAW), B(6, Pt2, 6 * RAW)}, s))) return r;
  } else {
    // H2C_A: per message the two field elements t (T), the exponentiation inputs (E) and the rest of the SWU state (St: twelve raw elements per map)
    if ((r = run(ctx, P_H2C_A, n, {B(0, d_uniform, 256), B(3, T, 4 * RAW), B(4, E, 4 * RAW), B(5, St, 24 * RAW)}, s))) return r;
    if ((r = run_pow(ctx, 2, 2 * n, E, Pw, s, tab))) return r;
    // H2C_B1: one map per item (2 n items) -> its point on E2'
    if ((r = run(ctx, P_H2C_B1, 2 * n, {B(3, T, 2 * RAW), B(5, Pw, 2 * RAW), B(4, St, 12 * RAW), B(6, Pt2, 6 * RAW)}, s))) return r;
  }
  // H2C_B2: the two points of a message -> their sum on E2 (round 3: one program, 62 slots, four workgroups per CU)
  if ((r = run(ctx, P_H2C_B2, n, {B(3, Pt2, 12 * RAW), B(6, E, 6 * RAW)}, s))) return r;        // E is free again: reuse it for the E2 point
  if ((r = dev_clear_g2(ctx, n, E, Q, S, E, N, s))) return r;
  if (proj) { *proj = E; return NBLS_OK; }
  return to_affine(ctx, true, n, E, N, NI, d_out, st, s, false);
}
// sum of n affine points (left fold of add == tree of complete additions): affine wire bytes + status (1 = sum is the zero point)
int dev_point_sum(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, void* d_out, void* d_status, hipStream_t s) {
  const size_t a = g2 ? 192 : 96, p = g2 ? 6 * RAW : 3 * RAW;
  uint8_t *A, *Bf, *N, *NI; int r;
  if ((r = need(ctx, SB_WORK_A, (n + 2) * p, &A)) || (r = need(ctx, SB_WORK_B, (n / 2 + 2) * p, &Bf)) || (r = need(ctx, SB_NORM, RAW, &N)) || (r = need(ctx, SB_NORM_INV, RAW, &NI))) return r;
  uint8_t* ident = g2 ? ctx->ident_g2 : ctx->ident_g1;
  if (n == 0) { HIPCHK(hipMemcpyAsync(A, ident, p, hipMemcpyDeviceToDevice, s)); }
  else if ((r = run(ctx, g2 ? P_G2_TO_PROJ : P_G1_TO_PROJ, n, {B(g2 ? 1 : 0, d_pts, a), B(3, A, p)}, s))) return r;
  uint8_t *src = A, *dst = Bf; size_t m = n ? n : 1;
  while (m > 1) {
    if (m & 1) { HIPCHK(hipMemcpyAsync(src + m * p, ident, p, hipMemcpyDeviceToDevice, s)); m++; }
    if ((r = run(ctx, g2 ? P_G2_ADD2 : P_G1_ADD2, m / 2, {B(3, src, 2 * p), B(5, dst, p)}, s))) return r;
    std::swap(src, dst); m /= 2;
  }
  return to_affine(ctx, g2, 1, src, N, NI, d_out, d_status, s);
}

EXPORT int nbls_g1_validate_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, int8_t* status) {
  if (!ctx || (n && (!g1_aff || !status))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * 96), *st = io.alloc(n); if (!d || !st) return NBLS_EHIP;
  HIPCHK(hipMemcpyAsync(d, g1_aff, n * 96, hipMemcpyHostToDevice, s));
  int r = dev_validate(ctx, false, n, d, st, s); if (r) return r;
  HIPCHK(hipMemcpyAsync(status, st, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); return NBLS_OK;
}
EXPORT int nbls_g2_validate_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, int8_t* status) {
  if (!ctx || (n && (!g2_aff || !status))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * 192), *st = io.alloc(n); if (!d || !st) return NBLS_EHIP;
  HIPCHK(hipMemcpyAsync(d, g2_aff, n * 192, hipMemcpyHostToDevice, s));
  int r = dev_validate(ctx, true, n, d, st, s); if (r) return r;
  HIPCHK(hipMemcpyAsync(status, st, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); return NBLS_OK;
}
int decompress_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* in, uint8_t* out, int8_t* status) {
  if (!ctx || (n && (!in || !out))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  const size_t e = g2 ? 96 : 48;
  LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * e), *o = io.alloc(n * 2 * e), *st = io.alloc(n); if (!d || !o || !st) return NBLS_EHIP;
  HIPCHK(hipMemcpyAsync(d, in, n * e, hipMemcpyHostToDevice, s));
  int r = dev_decompress(ctx, g2, n, d, o, st, s); if (r) return r;
  HIPCHK(hipMemcpyAsync(out, o, n * 2 * e, hipMemcpyDeviceToHost, s));
  std::vector<int8_t> tmp(n); HIPCHK(hipMemcpyAsync(tmp.data(), st, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  if (status) memcpy(status, tmp.data(), n);
  return NBLS_OK;
}
EXPORT int nbls_g1_decompress_batch(nbls_ctx* ctx, size_t n, const uint8_t* in48, uint8_t* out96, int8_t* status) { return decompress_host(ctx, false, n, in48, out96, status); }
EXPORT int nbls_g2_decompress_batch(nbls_ctx* ctx, size_t n, const uint8_t* in96, uint8_t* out192, int8_t* status) { return decompress_host(ctx, true, n, in96, out192, status); }

// expand_message_xmd for all messages on the device (xmd_kernel.hip): uploads the message blob, the n+1 offsets and the DST
// into the scratch pool and leaves len_in_bytes (64, 128 or 256) uniform bytes per message in *d_uniform.  Only a DST longer than 255 bytes is touched
// on the host (RFC 9380 5.3.3: replaced by its SHA-256 digest), which is per call, not per message.
int dev_expand(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offs, const uint8_t* dst, size_t dst_len, uint8_t** d_uniform, hipStream_t s, unsigned len_in_bytes) {
  for (size_t i = 0; i < n; i++) if (offs[i + 1] < offs[i]) return NBLS_EINVAL;
  const size_t total = offs[n] - offs[0];
  uint8_t dst_hash[32];
  dst = effective_dst(dst, &dst_len, dst_hash);
  uint8_t *dm, *dofs, *dd, *du; int r;
  if ((r = need(ctx, SB_MSGS, total + 4, &dm)) || (r = need(ctx, SB_OFFS_DST, (n + 1) * 4 + 256, &dofs)) || (r = need(ctx, SB_UNIFORM, n * (size_t)len_in_bytes, &du))) return r;
  dd = dofs + (n + 1) * 4;
  std::vector<uint32_t> rel(n + 1); pack_rel(rel.data(), offs, n);   // (three copies from pageable memory straight into the slots: this path does not stage through the block)
  if (total) HIPCHK(hipMemcpyAsync(dm, msgs + offs[0], total, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dofs, rel.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dd, dst, dst_len, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));     // `rel` and a hashed DST live on this stack frame
  LAUNCHCHK(nbls_xmd_launch((unsigned)n, dm, dofs, dd, (unsigned)dst_len, du, len_in_bytes, nullptr, s));
  *d_uniform = du;
  return NBLS_OK;
}
EXPORT int nbls_hash_to_g2_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out192) {
  if (!ctx || (n && (!offsets || !out192 || !dst))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  LOCKED(ctx); HostIO io{ctx}; void* o = io.alloc(n * 192); if (!o) return NBLS_EHIP;
  uint8_t* d; int r = dev_expand(ctx, n, msgs, offsets, dst, dst_len, &d, s); if (r) return r;
  if ((r = dev_hash_to_g2(ctx, n, d, o, s))) return r;
  HIPCHK(hipMemcpyAsync(out192, o, n * 192, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); return NBLS_OK;
}
int sum_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* pts, uint8_t* out, int8_t* status) {
  if (!ctx || !out || (n && !pts)) return NBLS_EINVAL;
  const size_t a = g2 ? 192 : 96;
  LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * a), *o = io.alloc(a), *st = io.alloc(1); if (!d || !o || !st) return NBLS_EHIP;
  if (n) HIPCHK(hipMemcpyAsync(d, pts, n * a, hipMemcpyHostToDevice, s));
  int r = dev_point_sum(ctx, g2, n, d, o, st, s); if (r) return r;
  int8_t z = 0; HIPCHK(hipMemcpyAsync(out, o, a, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&z, st, 1, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  if (status) *status = z;
  return NBLS_OK;
}
EXPORT int nbls_g1_sum(nbls_ctx* ctx, size_t n, const uint8_t* pts96, uint8_t* out96, int8_t* status) { return sum_host(ctx, false, n, pts96, out96, status); }
EXPORT int nbls_g2_sum(nbls_ctx* ctx, size_t n, const uint8_t* pts192, uint8_t* out192, int8_t* status) { return sum_host(ctx, true, n, pts192, out192, status); }

// PointG1.hashToCurve (count = 2) / PointG1.encodeToCurve (count = 1) on 64 * count uniform bytes per message (index.ts:331-350)
int dev_hash_to_g1(nbls_ctx* ctx, int count, size_t n, const void* d_uniform, void* d_out, hipStream_t s) {
  uint8_t *U, *E, *Pw, *Q, *Q2, *N, *NI, *st; int r;
  if ((r = need(ctx, SB_WORK_A, n * 2 * RAW, &U)) || (r = need(ctx, SB_WORK_B, n * 3 * RAW, &E)) || (r = need(ctx, SB_WORK_C, n * 2 * RAW, &Pw)) || (r = need(ctx, SB_WORK_D, n * 3 * RAW, &Q)) ||
      (r = need(ctx, SB_NORM, n * RAW, &N)) || (r = need(ctx, SB_NORM_INV, n * RAW, &NI)) || (r = need(ctx, SB_POINT_ST, n, &st))) return r;
  Q2 = E;   // E (the exponentiation inputs) is free again after the pow kernel
  const size_t us = (size_t)count * RAW;
  if ((r = run(ctx, count == 2 ? P_H2C1_A : P_ENC1_A, n, {B(0, d_uniform, 64 * (size_t)count), B(3, U, us), B(4, E, us)}, s))) return r;
  if ((r = run_pow(ctx, 3, (size_t)count * n, E, Pw, s))) return r;
  if ((r = run(ctx, count == 2 ? P_H2C1_B : P_ENC1_B, n, {B(3, U, us), B(5, Pw, us), B(6, Q, 3 * RAW)}, s))) return r;
  if ((r = run(ctx, P_G1_CLEAR, n, {B(3, Q, 3 * RAW), B(6, Q2, 3 * RAW), B(7, N, RAW)}, s))) return r;
  return to_affine(ctx, false, n, Q2, N, NI, d_out, st, s, false);
}
// PointG2.encodeToCurve on 128 uniform bytes per message (index.ts:491-497)
int dev_encode_to_g2(nbls_ctx* ctx, size_t n, const void* d_uniform, void* d_out, hipStream_t s) {
  uint8_t *T, *E, *Pw, *Q, *N, *NI, *st; int r;
  if ((r = need(ctx, SB_WORK_A, n * 2 * RAW, &T)) || (r = need(ctx, SB_WORK_B, n * 6 * RAW, &E)) || (r = need(ctx, SB_WORK_C, n * 2 * RAW, &Pw)) || (r = need(ctx, SB_WORK_D, n * 6 * RAW, &Q)) ||
      (r = need(ctx, SB_NORM, n * RAW, &N)) || (r = need(ctx, SB_NORM_INV, n * RAW, &NI)) || (r = need(ctx, SB_POINT_ST, n, &st))) return r;
  if ((r = run(ctx, P_ENC2_A, n, {B(0, d_uniform, 128), B(3, T, 2 * RAW), B(4, E, 2 * RAW)}, s))) return r;
  if ((r = run_pow(ctx, 2, n, E, Pw, s))) return r;
  if ((r = run(ctx, P_ENC2_B, n, {B(3, T, 2 * RAW), B(5, Pw, 2 * RAW), B(6, E, 6 * RAW)}, s))) return r;
  uint8_t* S; if ((r = need(ctx, SB_CLEAR_S, n * 6 * RAW, &S))) return r;
  if ((r = dev_clear_g2(ctx, n, E, Q, S, E, N, s))) return r;
  return to_affine(ctx, true, n, E, N, NI, d_out, st, s, false);
}
// mode: 0 = PointG1.hashToCurve, 1 = PointG1.encodeToCurve, 2 = PointG2.encodeToCurve
int hash_curve_host(nbls_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out) {
  if (!ctx || (n && (!offsets || !out || !dst))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  const size_t a = mode == 2 ? 192 : 96;
  LOCKED(ctx); HostIO io{ctx}; void* o = io.alloc(n * a); if (!o) return NBLS_EHIP;
  uint8_t* d; int r = dev_expand(ctx, n, msgs, offsets, dst, dst_len, &d, s, mode == 1 ? 64 : 128); if (r) return r;
  r = mode == 2 ? dev_encode_to_g2(ctx, n, d, o, s) : dev_hash_to_g1(ctx, mode == 0 ? 2 : 1, n, d, o, s); if (r) return r;
  HIPCHK(hipMemcpyAsync(out, o, n * a, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); return NBLS_OK;
}
EXPORT int nbls_hash_to_g1_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out96) { return hash_curve_host(ctx, 0,
    n, msgs, offsets, dst, dst_len, out96); }
EXPORT int nbls_encode_to_g1_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out96) { return hash_curve_host(ctx, 1,
    n, msgs, offsets, dst, dst_len, out96); }
EXPORT int nbls_encode_to_g2_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out192) { return hash_curve_host(ctx,
    2, n, msgs, offsets, dst, dst_len, out192); }

// hash-to-curve BEHIND expand_message_xmd on caller-chosen uniform bytes (tests/test_gpu_h2c_map.py): the bodies of nbls_hash_to_g2_batch / hash_curve_host without dev_expand, so the
// launches are the pipelines' own -- h2c_norm_min against n, the point chains' form by n, run_pow's wide form up to pow_wide_max() elements.
// kind: 0 G2 hash (256 bytes in, 192 out), 1 G2 encode (128 -> 192), 2 G1 hash (128 -> 96), 3 G1 encode (64 -> 96); status 1 = the zero point (P_G*_TO_AFFINE found Z = 0)
EXPORT int nbls_map_uniform_batch(nbls_ctx* ctx, int kind, size_t n, const uint8_t* uniform, uint8_t* out, int8_t* status) {
  if (!ctx || kind < 0 || kind > 3 || (n && (!uniform || !out))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  const size_t in = kind == 0 ? 256 : kind == 3 ? 64 : 128, a = kind < 2 ? 192 : 96;
  LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * in), *o = io.alloc(n * a); if (!d || !o) return NBLS_EHIP;
  HIPCHK(hipMemcpyAsync(d, uniform, n * in, hipMemcpyHostToDevice, s));
  int r = kind == 0 ? dev_hash_to_g2(ctx, n, d, o, s) : kind == 1 ? dev_encode_to_g2(ctx, n, d, o, s) : dev_hash_to_g1(ctx, kind == 2 ? 2 : 1, n, d, o, s); if (r) return r;
  uint8_t* st; if ((r = need(ctx, SB_POINT_ST, n, &st))) return r;       // where all three pipelines leave to_affine's status bytes
  std::vector<int8_t> zero(n);
  HIPCHK(hipMemcpyAsync(out, o, n * a, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(zero.data(), st, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; i++) if (zero[i]) memset(out + i * a, 0, a);
  if (status) memcpy(status, zero.data(), n);
  return NBLS_OK;
}

// PointG1.toHex(true) / PointG2.toSignature for non-zero affine points (index.ts:359-371, 586-602): bulk serialisation
int compress_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* aff, uint8_t* out) {
  if (!ctx || (n && (!aff || !out))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  const size_t a = g2 ? 192 : 96, c = a / 2;
  LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * a), *o = io.alloc(n * c); if (!d || !o) return NBLS_EHIP;
  HIPCHK(hipMemcpyAsync(d, aff, n * a, hipMemcpyHostToDevice, s));
  int r = run(ctx, g2 ? P_G2_COMPRESS : P_G1_COMPRESS, n, {B(0, d, a), B(2, o, c)}, s); if (r) return r;
  HIPCHK(hipMemcpyAsync(out, o, n * c, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  return NBLS_OK;
}
EXPORT int nbls_g1_compress_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, uint8_t* out48) { return compress_host(ctx, false, n, g1_aff, out48); }
EXPORT int nbls_g2_compress_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, uint8_t* out96) { return compress_host(ctx, true, n, g2_aff, out96); }

// ---- every wire form of the reference's point codecs, in bulk --------------------------------------------------------------
// PointG1.fromHex (index.ts:298-327): 48 compressed or 96 uncompressed bytes per point; PointG2.fromHex (index.ts:532-579): 96 compressed
// (flag rules, no subgroup check) or 192 uncompressed bytes; PointG2.fromSignature (index.ts:500-530): 96 or 192 bytes.
int decode_host(nbls_ctx* ctx, int kind /* 0 g1.fromHex, 1 g2.fromHex, 2 g2.fromSignature */, size_t n, const uint8_t* in, size_t len, uint8_t* out, int8_t* status) {
  if (!ctx || (n && (!in || !out || !status))) return NBLS_EINVAL;
  const bool g2 = kind != 0;
  const size_t a = g2 ? 192 : 96;
  if (len != a && len != a / 2) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * len), *o = io.alloc(n * a), *st = io.alloc(n); if (!d || !o || !st) return NBLS_EHIP;
  HIPCHK(hipMemcpyAsync(d, in, n * len, hipMemcpyHostToDevice, s));
  int r;
  if (kind == 0) r = len == 48 ? dev_decompress(ctx, false, n, d, o, st, s) : run(ctx, P_G1_FROM_RAW, n, {B(0, d, 96), B(6, o, 96), B(7, st, 1)}, s);
  else if (kind == 1) r = len == 96 ? dev_decompress(ctx, true, n, d, o, st, s, DEC_MAIN, 2) : run(ctx, P_G2_FROM_RAW, n, {B(0, d, 192), B(6, o, 192), B(7, st, 1)}, s);
  else r = dev_decompress(ctx, true, n, d, o, st, s, DEC_MAIN, len == 192 ? 1 : 0);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(out, o, n * a, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(status, st, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  return NBLS_OK;
}
EXPORT int nbls_g1_from_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* in, size_t len, uint8_t* out96, int8_t* status) { return decode_host(ctx, 0, n, in, len, out96, status); }
EXPORT int nbls_g2_from_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* in, size_t len, uint8_t* out192, int8_t* status) { return decode_host(ctx, 1, n, in, len, out192, status); }
EXPORT int nbls_g2_from_signature_batch(nbls_ctx* ctx, size_t n, const uint8_t* in, size_t len, uint8_t* out192, int8_t* status) { return decode_host(ctx, 2, n, in, len, out192, status); }
// PointG1.toHex / PointG2.toHex (index.ts:359-381, 603-631) for n valid affine points; zero[i] != 0 marks the zero point (its affine bytes are
// ignored): compressed 0xc0 00.., uncompressed 0x40 00..
int encode_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* aff, const int8_t* zero, int compressed, uint8_t* out) {
  if (!ctx || (n && (!aff || !out))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  const size_t a = g2 ? 192 : 96, c = compressed ? a / 2 : a;
  int r;
  if (compressed) { if ((r = compress_host(ctx, g2, n, aff, out))) return r; }
  else if (!g2) memcpy(out, aff, n * a);
  else {
    LOCKED(ctx); HostIO io{ctx}; void *d = io.alloc(n * a), *o = io.alloc(n * a); if (!d || !o) return NBLS_EHIP;
    HIPCHK(hipMemcpyAsync(d, aff, n * a, hipMemcpyHostToDevice, s));
    if ((r = run(ctx, P_G2_SWAP, n, {B(0, d, a), B(2, o, a)}, s))) return r;
    HIPCHK(hipMemcpyAsync(out, o, n * a, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  }
  if (zero) for (size_t i = 0; i < n; i++) if (zero[i]) { memset(out + i * c, 0, c); out[i * c] = compressed ? 0xc0 : 0x40; }
  return NBLS_OK;
}
EXPORT int nbls_g1_to_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const int8_t* zero, int compressed, uint8_t* out) { return encode_host(ctx, false, n, g1_aff, zero, compressed, out); }
EXPORT int nbls_g2_to_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, const int8_t* zero, int compressed, uint8_t* out) { return encode_host(ctx, true, n, g2_aff, zero, compressed, out); }
// PointG1.clearCofactor (index.ts:401-405) / PointG2.clearCofactor (index.ts:659-672) for n affine points ON THE CURVE (any subgroup):
// status 1 = the result is the zero point
int clear_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* aff, uint8_t* out, int8_t* status) {
  if (!ctx || (n && (!aff || !out || !status))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  const size_t a = g2 ? 192 : 96, p = g2 ? 6 * RAW : 3 * RAW;
  LOCKED(ctx); HostIO io{ctx};
  void *d = io.alloc(n * a), *P = io.alloc(n * p), *Q = io.alloc(n * p), *N = io.alloc(n * RAW), *NI = io.alloc(n * RAW), *o = io.alloc(n * a), *st = io.alloc(n);
  if (!d || !P || !Q || !N || !NI || !o || !st) return NBLS_EHIP;
  HIPCHK(hipMemcpyAsync(d, aff, n * a, hipMemcpyHostToDevice, s));
  int r;
  if ((r = run(ctx, g2 ? P_G2_TO_PROJ : P_G1_TO_PROJ, n, {B(g2 ? 1 : 0, d, a), B(3, P, p)}, s))) return r;
  if (g2) { void* S2 = io.alloc(n * p); if (!S2) return NBLS_EHIP; if ((r = dev_clear_g2(ctx, n, P, (uint8_t*)Q, (uint8_t*)S2, Q, N, s))) return r; }
  else if ((r = run(ctx, P_G1_CLEAR, n, {B(3, P, p), B(6, Q, p), B(7, N, RAW)}, s))) return r;
  if ((r = to_affine(ctx, g2, n, Q, N, NI, o, st, s, false))) return r;
  HIPCHK(hipMemcpyAsync(out, o, n * a, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(status, st, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  return NBLS_OK;
}
EXPORT int nbls_g1_clear_cofactor_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, uint8_t* out96, int8_t* status) { return clear_host(ctx, false, n, g1_aff, out96, status); }
EXPORT int nbls_g2_clear_cofactor_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, uint8_t* out192, int8_t* status) { return clear_host(ctx, true, n, g2_aff, out192, status); }

// [k_i]P_i for per-item 256-bit big-endian scalars (pt_stride 0 = one point for all items): ladder -> inversion -> affine
// the fixed-base table of G1.BASE (curve.h pt_mul_fixed_g1): for every window w and digit d = 1 .. 2^WIN - 1 the point [d 2^(WIN w)]G as a raw projective point (x, y, 1), computed
// ONCE per context by the variable-base ladder itself (602 scalar multiplications with WIN = 3: a few hundred microseconds) -- no table of constants enters the source
int ensure_g1_fixed(nbls_ctx* ctx, hipStream_t s) {
  if (ctx->g1_fixed) return NBLS_OK;
  const int WIN = G1_FIXED_WIN, NW = g1_fixed_windows(), NE = g1_fixed_entries();
  const size_t m = (size_t)NW * NE;
  std::vector<uint8_t> ks(m * 32, 0);
  for (int w = 0; w < NW; w++)
    for (int d = 1; d <= NE; d++) {
      uint8_t* k = &ks[((size_t)w * NE + d - 1) * 32];
      const int sh = WIN * w;                                         // d << sh as a 256-bit big-endian integer; digits that would pass bit 255 (the short top window) are never read: [1]G stands in
      if (sh + 32 - __builtin_clz((unsigned)d) > 256) { k[31] = 1; continue; }
      for (int bit = 0; bit < WIN; bit++) if ((d >> bit) & 1) { const int pos = sh + bit; k[31 - pos / 8] |= (uint8_t)(1u << (pos % 8)); }
    }
  uint8_t *dk = nullptr, *aff = nullptr, *st = nullptr, *tab = nullptr;
  auto fail = [&](int code) { for (uint8_t* p : {dk, aff, st, tab}) if (p) hipFree(p); return code; };
  if (hipMalloc(&dk, m * 32) != hipSuccess || hipMalloc(&aff, m * 96) != hipSuccess || hipMalloc(&st, m) != hipSuccess || hipMalloc(&tab,
      m * 3 * RAW) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); return fail(NBLS_EHIP); }
  if (hipMemcpyAsync(dk, ks.data(), m * 32, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); return fail(NBLS_EHIP); }
  int r = dev_point_mul(ctx, false, m, ctx->gen_g1, 0, dk, aff, st, s, false);
  if (!r) r = run(ctx, P_G1_TO_PROJ, m, {B(0, aff, 96), B(3, tab, 3 * RAW)}, s);
  if (!r && hipStreamSynchronize(s) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); r = NBLS_EHIP; }
  if (r) return fail(r);
  hipFree(dk); hipFree(aff); hipFree(st);
  ctx->g1_fixed = tab;
  return NBLS_OK;
}
// The psi-split G2 ladders (NBLS_G2_GLS=0 keeps the plain one) and which of the two forms n items take: up to sac_max the sign-aligned form, which reads RAW PROJECTIVE points
// (six raw elements each, pt_stride = 6 * RAW); above, the windowed form on affine wire points.  dev_point_mul and every caller that prepares its points (sign_points,
// combine_pipeline) ask here, so the ladder and its input cannot disagree
static bool g2_gls_on() { static const bool on = env_long("NBLS_G2_GLS", 1) != 0; return on; }
bool g2_ladder_takes_projective(const nbls_ctx* ctx, size_t n) { return g2_gls_on() && n <= ctx->sac_max; }
int dev_point_mul(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, size_t pt_stride, const void* d_scalars, void* d_out, void* d_status, hipStream_t s, bool allow_fixed, bool in_subgroup,
                  uint8_t* recoded, uint8_t** proj) {   // recoded: the sign-aligned digits of the scalars, made by the caller (sign_points: beside the hash chain), or NULL
  // proj: stop at the ladder's raw projective points (SB_WORK_A) -- the caller sums them and normalises only the sums (combine_pipeline)
  const size_t p = g2 ? 6 * RAW : 3 * RAW;
  uint8_t *Pj, *N, *NI; int r;
  // getPublicKey (the base point is G1.BASE for every item): no doublings, the multiples of the generator come from a table (round 5: 86 additions instead of 256 doublings + 128
  // additions; NBLS_G1_FIXED=0 keeps the ladder)
  static const bool fixed_on = env_long("NBLS_G1_FIXED", 1) != 0;
  const bool fixed = allow_fixed && fixed_on && !g2 && d_pts == ctx->gen_g1 && pt_stride == 0;
  if (fixed && (r = ensure_g1_fixed(ctx, s))) return r;
  if ((r = need(ctx, SB_WORK_A, n * p, &Pj)) || (r = need(ctx, SB_NORM, n * RAW, &N)) || (r = need(ctx, SB_NORM_INV, n * RAW, &NI))) return r;
  // sign (the base points are hash outputs: in G2 by construction): the scalar split along psi, four 65-bit digits on one accumulator (codec.h pt_mul_gls_g2: 66 doublings + 132 additions
  // instead of 256 + 128; NBLS_G2_GLS=0 keeps the plain ladder).  The digits are made on the device by the MSM's decomposition kernel (branch-free long division by |z|).
  if (g2 && in_subgroup && g2_gls_on()) {
    const bool sac = g2_ladder_takes_projective(ctx, n);
    // up to sac_max keys d_pts are RAW PROJECTIVE points (six raw elements each, pt_stride = 6 * RAW: sign_points() below) -- the hash points as cofactor clearing leaves them in
    // SB_WORK_B, so the digits go to SB_WORK_C; above, affine wire points as everywhere else
    uint8_t* dig = recoded;
    if (!dig && (r = need(ctx, sac ? SB_WORK_C : SB_WORK_B, n * 128, &dig))) return r;
    ForkGuard digits{true, dig, n * 128};   // an error return before the memset behind the ladder is enqueued zeroes the digits
    // while every wavefront of the launch is resident at once the length of ONE wavefront's instruction stream is the time: the sign-aligned recoding with one addition per bit
    // (codec.h pt_mul_sac_g2: 65 doublings + 73 additions; its table of eight points takes 101 slots = three workgroups per CU = 768 wavefronts of 8 keys); above 6144 keys the
    // windowed form, whose table of four leaves room for six workgroups per CU (NBLS_G2_SAC_MAX / NBLS_TUNE_SAC_MAX; 0 = never)
    if (sac) {
      if (!recoded) LAUNCHCHK(nbls_msm_sac_launch((unsigned)n, d_scalars, dig, s));
      if ((r = run(ctx, pt_ls2_variant(ctx, P_G2_MUL_SAC, n), n, {B(1, d_pts, pt_stride), B(2, dig, 128), B(3, Pj, p), B(4, N, RAW)}, s))) return r;
    } else {
    LAUNCHCHK(nbls_msm_decompose_launch((unsigned)n, 4, d_scalars, dig, s));
    if ((r = run(ctx, P_G2_MUL_GLS, n, {B(1, d_pts, pt_stride), B(2, dig, 128), B(3, Pj, p), B(4, N, RAW)}, s))) return r;
    }
    HIPCHK(hipMemsetAsync(dig, 0, n * 128, s));      // the recoded digits ARE the private keys: not left in a scratch slot that later calls reuse
    digits.armed = false;
  } else
  if (fixed) {
    if ((r = run(ctx, P_G1_MUL_FIXED, n, {B(2, d_scalars, 32), B(5, ctx->g1_fixed, 0), B(3, Pj, p), B(4, N, RAW)}, s))) return r;
  } else {
  // up to one wavefront per SIMD (16 / 8 items per wavefront) the length of one wavefront's instruction stream counts: 3-bit windows (85 additions); above, wavefronts per CU
  // count: 2-bit windows, whose table of four leaves room for seven workgroups per CU instead of three / four (tools/mul_time.py)
  static const size_t w3_waves = (size_t)env_long("NBLS_MUL_W3_WAVES", 1024);
  const bool w3 = (n + (g2 ? 7 : 15)) / (g2 ? 8 : 16) <= w3_waves;
  if ((r = run(ctx, g2 ? (w3 ? P_G2_MUL_W3 : P_G2_MUL) : (w3 ? P_G1_MUL_W3 : P_G1_MUL), n, {B(g2 ? 1 : 0, d_pts, pt_stride), B(2, d_scalars, 32), B(3, Pj, p), B(4, N, RAW)}, s))) return r;
  }
  if (proj) { *proj = Pj; return NBLS_OK; }
  return to_affine(ctx, g2, n, Pj, N, NI, d_out, d_status, s, false);
}
// sign's two halves: hash-to-G2, then the key ladder on the hash points.  Up to sac_max keys the points stay projective in between (no inversion, no affine program: the
// sign-aligned ladder reads raw projective points); above, they are normalised first (the windowed ladder's affine input keeps it at six workgroups per CU).  `h`: n * 192 bytes of
// device scratch for the affine points of the second form
int sign_points(nbls_ctx* ctx, size_t n, const void* d_uniform, void* h, const void* d_keys32, void* d_out192, void* d_status, hipStream_t s) {
  int r;
  if (g2_ladder_takes_projective(ctx, n)) {
    // the recoding of the keys (0.045 ms for one key: a branch-free long division) does not need the hash points: it runs beside the hash chain on a side stream (round 6)
    uint8_t *pj, *dig;
    if ((r = need(ctx, SB_MSGS, n * 128, &dig)) || (r = ensure_side2(ctx))) return r;
    HIPCHK(hipEventRecord(ctx->ev_fork, s)); HIPCHK(hipStreamWaitEvent(ctx->side2, ctx->ev_fork, 0));
    ForkGuard fork{true, dig, n * 128};   // the digits are the keys: an error return before the ladder has read them (dev_point_mul zeroes them behind it) zeroes them too
    LAUNCHCHK(nbls_msm_sac_launch((unsigned)n, d_keys32, dig, ctx->side2));
    HIPCHK(hipEventRecord(ctx->ev_join2, ctx->side2));
    if ((r = dev_hash_to_g2(ctx, n, d_uniform, nullptr, s, 0, 0, &pj))) return r;
    HIPCHK(hipStreamWaitEvent(s, ctx->ev_join2, 0));
    if (!(r = dev_point_mul(ctx, true, n, pj, 6 * RAW, d_keys32, d_out192, d_status, s, true, true, dig))) fork.armed = false;
    return r;
  }
  if ((r = dev_hash_to_g2(ctx, n, d_uniform, h, s))) return r;
  return dev_point_mul(ctx, true, n, h, 192, d_keys32, d_out192, d_status, s, true, true);      // H(m) is in G2: the ladder may split the key along psi
}
// scalar k is acceptable iff k mod r != 0 (normalizePrivKey, index.ts:269-279, reduces mod r and rejects zero); the ladder
// itself takes any 256-bit value since the points are in the order-r subgroup
bool scalar_is_zero_mod_r(const uint8_t* k32) {
  static const uint8_t R_BE[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                   0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
  uint8_t m[32] = {0};   // m = 0, r, 2r, 3r  (4r > 2^256 - 1? 4r = 0x1cfb6..., 33 bytes: stop at 3r)
  for (int mult = 0; mult < 4; mult++) {
    if (memcmp(m, k32, 32) == 0) return true;
    unsigned c = 0; for (int i = 31; i >= 0; i--) { unsigned v = (unsigned)m[i] + R_BE[i] + c; m[i] = (uint8_t)v; c = v >> 8; }
    if (c) break;
  }
  return false;
}
int mul_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* pts, const uint8_t* scalars32, uint8_t* out, int8_t* status) {
  if (!ctx || (n && (!scalars32 || !out)) || (g2 && n && !pts)) return NBLS_EINVAL; if (!n) return NBLS_OK;
  const size_t a = g2 ? 192 : 96;
  LOCKED(ctx); HostIO io{ctx}; void *dp = pts ? io.alloc(n * a) : nullptr, *dk = io.alloc(n * 32), *o = io.alloc(n * a), *st = io.alloc(n);
  if ((pts && !dp) || !dk || !o || !st) return NBLS_EHIP;
  io.secret(dk, n * 32);      // the scalars are private keys in getPublicKey / sign: zeroed before the staging block goes back to the pool
  if (pts) HIPCHK(hipMemcpyAsync(dp, pts, n * a, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dk, scalars32, n * 32, hipMemcpyHostToDevice, s));
  int r = dev_point_mul(ctx, g2, n, pts ? dp : ctx->gen_g1, pts ? a : 0, dk, o, st, s); if (r) return r;
  std::vector<int8_t> tmp(n), zero(n, 0);
  if ((r = io.wipe(s))) return r;
  HIPCHK(hipMemcpyAsync(out, o, n * a, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(tmp.data(), st, n, hipMemcpyDeviceToHost, s));
  for (size_t i = 0; i < n; i++) if (scalar_is_zero_mod_r(scalars32 + 32 * i)) zero[i] = 1;      // host work under the device's (round 6: 0.3 ms at 8192 keys when it followed the synchronisation)
  HIPCHK(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; i++) if (zero[i]) tmp[i] = 5;
  if (status) memcpy(status, tmp.data(), n);
  return NBLS_OK;
}
// PointG1.fromPrivateKey / getPublicKey core (index.ts:350-353, 738-740): [k_i]P_i, P = generator when g1_aff is NULL
EXPORT int nbls_g1_mul_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const uint8_t* scalars32, uint8_t* out96, int8_t* status) { return mul_host(ctx, false, n, g1_aff, scalars32,
    out96, status); }
EXPORT int nbls_g2_mul_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, const uint8_t* scalars32, uint8_t* out192, int8_t* status) { return mul_host(ctx, true, n, g2_aff, scalars32,
    out192, status); }
// sign(message_i, key_i) (index.ts:744-752): hashToCurve -> multiply by the key -> affine signature point (the caller
// compresses, PointG2.toSignature index.ts:586-602).  status: 0 ok, 5 key is 0 mod r.
EXPORT int nbls_sign_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, const uint8_t* keys32, uint8_t* out192, int8_t* status) {
  WHOLE_CALL(ctx);   // scratch and I/O staging buffers belong to this call until it returns
  if (!ctx || (n && (!offsets || !out192 || !dst || !keys32))) return NBLS_EINVAL; if (!n) return NBLS_OK;
  // Round 6: ONE pinned staging block in, one out (Staged, staging.h).  Round 5 made six copies from / to pageable memory (messages, offsets, tag, keys; signatures, statuses) with a
  // synchronisation in the middle: 0.5 ms of a 4.4 ms call at 8192 keys (the same call on resident inputs: 3.85 ms).  Inputs are packed into the context's pinned buffer --
  // [message bytes | n + 1 relative offsets | tag (256 B) | keys] -- and travel as one asynchronous copy; signatures and statuses come back the same way.
  for (size_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) return NBLS_EINVAL;
  const size_t total = offsets[n] - offsets[0];
  LOCKED(ctx); HostIO io{ctx};
  Staged st(ctx, s);   // (behind the HostIO: an error return waits for the device and zeroes the host copy of the keys before the device blocks go back to the pool)
  const size_t o_msg = st.bytes(total ? msgs + offsets[0] : nullptr, total), o_off = st.rel(offsets, n), o_dst = st.dst(dst, dst_len), o_key = st.secret(keys32, n * 32), out_bytes = n * 192 + n;
  uint8_t *h = (uint8_t*)io.alloc(n * 192), *din = (uint8_t*)io.alloc(st.in_bytes), *dout = (uint8_t*)io.alloc(out_bytes), *du; const uint8_t* res;
  if (!h || !din || !dout) return NBLS_EHIP;
  io.secret(din + o_key, n * 32);
  int r;
  if ((r = need(ctx, SB_UNIFORM, n * 256, &du)) || (r = st.send(din, out_bytes))) return r;
  LAUNCHCHK(nbls_xmd_launch((unsigned)n, din + o_msg, din + o_off, din + o_dst, (unsigned)st.dst_len, du, 256, nullptr, s));
  if ((r = sign_points(ctx, n, du, h, din + o_key, dout, dout + n * 192, s))) return r;
  if ((r = io.wipe(s))) return r;
  std::vector<int8_t> tmp(n, 0);
  for (size_t i = 0; i < n; i++) if (scalar_is_zero_mod_r(keys32 + 32 * i)) tmp[i] = 5;      // (host work under the device's: normalizePrivKey's rejection, index.ts:269-279)
  if ((r = st.fetch(dout, out_bytes, &res))) return r;
  memcpy(out192, res, n * 192);
  for (size_t i = 0; i < n; i++) if (tmp[i] != 5) tmp[i] = (int8_t)res[n * 192 + i];
  if (status) memcpy(status, tmp.data(), n);
  return NBLS_OK;
}

// The domain-separation tag of the device-resident hash entry points, kept on the device between calls (a service works under one tag): no copy, no synchronisation in the steady
// state.  A DST longer than 255 bytes is replaced by its SHA-256 digest (RFC 9380 5.3.3), as in dev_expand and the reference's expand_message_xmd (index.ts:207-231).
int dst_on_device(nbls_ctx* ctx, const uint8_t* dst, size_t* dst_len, hipStream_t s, uint8_t** dd) {
  uint8_t dst_hash[32];
  dst = effective_dst(dst, dst_len, dst_hash);
  std::lock_guard<std::recursive_mutex> g_(ctx->mu); HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->dst_dev) HIPCHK(hipMalloc(&ctx->dst_dev, 256));
  if (ctx->dst_host.size() != *dst_len || memcmp(ctx->dst_host.data(), dst, *dst_len)) {
    HIPCHK(hipStreamSynchronize(s));   // an earlier call may still read the old tag
    HIPCHK(hipMemcpy(ctx->dst_dev, dst, *dst_len, hipMemcpyHostToDevice));
    ctx->dst_host.assign(dst, dst + *dst_len);
  }
  *dd = ctx->dst_dev;
  return NBLS_OK;
}
// sign with everything resident in HBM (round 5): message bytes + offsets, 32-byte keys -> affine signature points and status bytes; SHA-256 expand_message_xmd, hash-to-G2 and
// the constant-time ladder in one chain on `stream`.  Synchronises (the offsets are validated by the hashing kernel and the verdict is read back).  index.ts:744-752.
EXPORT int nbls_sign_batch_dev(nbls_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len, const void* d_keys32, void* d_out192, void* d_status,
    void* stream) {
  WHOLE_CALL(ctx);
  if (!ctx || (n && (!d_offsets || !d_keys32 || !d_out192 || !d_status || !dst))) return NBLS_EINVAL;
  if (!n) return NBLS_OK;
  DEV_ENTER(ctx, stream);
  uint8_t* dd; int r;
  if ((r = dst_on_device(ctx, dst, &dst_len, s, &dd))) return r;   // (enqueues nothing on s; with a new tag it waits for s, which StreamOrder has put behind the previous call's stream)
  HostIO io{ctx}; io.s = s; void* h = io.alloc(n * 192); if (!h) return NBLS_EHIP;
  uint8_t* du;
  if ((r = need(ctx, SB_UNIFORM, n * 256 + 16, &du))) return r;
  uint32_t* d_bad = (uint32_t*)(du + n * 256);
  HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));
  LAUNCHCHK(nbls_xmd_launch((unsigned)n, d_msgs, d_offsets, dd, (unsigned)dst_len, du, 256, d_bad, s));
  if ((r = sign_points(ctx, n, du, h, d_keys32, d_out192, d_status, s))) return r;
  uint32_t bad = 0; HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  return bad ? NBLS_EINVAL : NBLS_OK;     // offsets[i + 1] < offsets[i] somewhere
}

