/*
 * nbls_napi.c -- thin N-API addon: exposes the C ABI of libnbls.so (include/nbls.h) to Node.  No arithmetic here.
 * libnbls.so is loaded with dlopen at module init so the addon builds with plain gcc (no HIP needed):
 *     gcc -shared -fPIC -I/usr/include/node -I../../include nbls_napi.c -o nbls_napi.node -ldl
 * Calls are synchronous (they block for the duration of the GPU work) except verifyBatchAsync (and signBatchAsync, verifyMultipleAsync, verifyAggregatesAsync, verifyMultipleSharedAsync, verifyAggregatesSharedAsync, frOpAsync, lagrangeAtZeroAsync, combineSharesAsync, polyEvalAsync, kzgVerifyProofsAsync, kzgVerifyBlobsAsync, kzgProveAsync, frNttAsync, kzgComputeCellsAsync, kzgCellsAndProofsAsync, kzgVerifyCellsAsync, groth16VerifyAsync), which runs on a libuv worker thread
 * (napi_create_async_work) and resolves a Promise: the facade's verifyBatch uses it for wire-format inputs (the calls that can take tens of milliseconds).  Typed arrays are passed by reference (napi_get_typedarray_info), no copies.
 */
#include <node_api.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nbls.h"

static void* lib;
#define SYM(name) static __typeof__(&name) p_##name;
SYM(nbls_init) SYM(nbls_destroy) SYM(nbls_strerror) SYM(nbls_pairing_batch) SYM(nbls_miller_product) SYM(nbls_final_exp_batch)
SYM(nbls_g1_validate_batch) SYM(nbls_g2_validate_batch) SYM(nbls_g1_decompress_batch) SYM(nbls_g2_decompress_batch)
SYM(nbls_hash_to_g2_batch) SYM(nbls_g1_sum) SYM(nbls_g2_sum) SYM(nbls_verify_batch) SYM(nbls_g1_mul_batch) SYM(nbls_g2_mul_batch) SYM(nbls_sign_batch) SYM(nbls_hash_to_g1_batch) SYM(nbls_encode_to_g1_batch) SYM(nbls_encode_to_g2_batch) SYM(nbls_g1_msm) SYM(nbls_g2_msm)
SYM(nbls_init_multi) SYM(nbls_destroy_multi) SYM(nbls_multi_device_count) SYM(nbls_multi_context) SYM(nbls_multi_pairing_batch) SYM(nbls_multi_miller_product) SYM(nbls_multi_verify_batch)
SYM(nbls_g2_prepare) SYM(nbls_pairing_prepared) SYM(nbls_verify_multiple) SYM(nbls_verify_aggregates) SYM(nbls_verify_multiple_shared) SYM(nbls_verify_aggregates_shared)
SYM(nbls_g1_from_hex_batch) SYM(nbls_g2_from_hex_batch) SYM(nbls_g2_from_signature_batch) SYM(nbls_g1_clear_cofactor_batch) SYM(nbls_g2_clear_cofactor_batch)
SYM(nbls_fr_op_batch) SYM(nbls_lagrange_at_zero) SYM(nbls_g2_combine_shares) SYM(nbls_g1_combine_shares) SYM(nbls_g1_poly_eval) SYM(nbls_g2_poly_eval)
SYM(nbls_kzg_verify_proofs) SYM(nbls_kzg_verify_blobs)
SYM(nbls_kzg_setup_create) SYM(nbls_kzg_setup_destroy) SYM(nbls_kzg_setup_log2n) SYM(nbls_kzg_commit_blobs) SYM(nbls_kzg_compute_proofs) SYM(nbls_kzg_compute_blob_proofs)
SYM(nbls_fr_ntt) SYM(nbls_kzg_compute_cells) SYM(nbls_kzg_monomial_create) SYM(nbls_kzg_monomial_destroy) SYM(nbls_kzg_monomial_log2n) SYM(nbls_kzg_compute_cells_and_proofs) SYM(nbls_kzg_verify_cells)
SYM(nbls_kzg_recover_cells) SYM(nbls_kzg_recover_cells_and_proofs)
SYM(nbls_groth16_vk_create) SYM(nbls_groth16_vk_destroy) SYM(nbls_groth16_vk_inputs) SYM(nbls_groth16_verify)
SYM(nbls_groth16_pk_create) SYM(nbls_groth16_pk_destroy) SYM(nbls_groth16_pk_params) SYM(nbls_groth16_prove)
static nbls_ctx* ctx;
static nbls_multi* multi;   /* several GPUs behind one handle (initMulti): ctx is then its first context; the batch calls shard over all of them */
#define MULTI() (multi && p_nbls_multi_device_count(multi) > 1)

#define CHECK(env, call) do { if ((call) != napi_ok) { napi_throw_error(env, NULL, "N-API call failed: " #call); return NULL; } } while (0)
static napi_value throw_code(napi_env env, int code) { char m[128]; snprintf(m, sizeof m, "nbls: %s (code %d)", p_nbls_strerror ? p_nbls_strerror(code) : "error", code); napi_throw_error(env, NULL, m); return NULL; }

static int get_bytes(napi_env env, napi_value v, uint8_t** data, size_t* len) {
  bool is_ta = false; napi_is_typedarray(env, v, &is_ta);
  if (is_ta) { napi_typedarray_type t; napi_value ab; size_t off; void* d; if (napi_get_typedarray_info(env, v, &t, len, &d, &ab, &off) != napi_ok) return 0; if (t == napi_uint32_array || t == napi_int32_array) *len *= 4;   /* length in bytes */ *data = (uint8_t*)d; return 1; }
  bool is_buf = false; napi_is_buffer(env, v, &is_buf);
  if (is_buf) { void* d; if (napi_get_buffer_info(env, v, &d, len) != napi_ok) return 0; *data = (uint8_t*)d; return 1; }
  return 0;
}
static napi_value new_u8(napi_env env, size_t n, uint8_t** data) {
  napi_value ab, ta; void* d; if (napi_create_arraybuffer(env, n, &d, &ab) != napi_ok) return NULL; *data = (uint8_t*)d;
  if (napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta) != napi_ok) return NULL; return ta;
}
static napi_value result2(napi_env env, napi_value out, napi_value status) {
  napi_value o; napi_create_object(env, &o); napi_set_named_property(env, o, "out", out); napi_set_named_property(env, o, "status", status); return o;
}
#define ARGS(n) size_t argc = n; napi_value argv[n]; CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL)); if (argc < n) { napi_throw_type_error(env, NULL, "missing arguments"); return NULL; }
#define NEED_CTX() if (!ctx) { napi_throw_error(env, NULL, "nbls: call init(deviceId) first"); return NULL; }
#define COUNT_FROM_OFFSETS(n, lo) if ((lo) < 4 || (lo) % 4) { napi_throw_range_error(env, NULL, "offsets must hold n + 1 entries"); return NULL; } size_t n = (lo) / 4 - 1;
#define ALLOCATED(v) if (!(v)) { napi_throw_error(env, NULL, "nbls: out of memory"); return NULL; }
#define BYTES(i, d, l) uint8_t* d; size_t l; if (!get_bytes(env, argv[i], &d, &l)) { napi_throw_type_error(env, NULL, "expected Uint8Array"); return NULL; }

/* Contexts for asynchronous calls in flight: verifyBatchAsync takes them round-robin, so that `await Promise.all([verifyBatch(..), verifyBatch(..), ..])`
 * overlaps the calls on the GPU (three 65,536-signature calls in flight: 21 ms per call amortised against 26 ms one at a time, bench.py).  pool[0] = ctx;
 * NBLS_CONTEXTS (default 1) or init(device, contexts) sets the size; the extra contexts are created on first use. */
#define MAX_POOL 8
static nbls_ctx* pool[MAX_POOL]; static int pool_size = 1, pool_dev = 0; static unsigned pool_next = 0;
static void pool_clear(void) { for (int i = 1; i < MAX_POOL; i++) if (pool[i]) { p_nbls_destroy(pool[i]); pool[i] = NULL; } pool[0] = NULL; pool_next = 0; }
static nbls_ctx* pool_take(void) {
  if (pool_size <= 1 || !ctx) return ctx;
  const int k = (int)(pool_next++ % (unsigned)pool_size);
  if (k == 0) return ctx;
  if (!pool[k] && p_nbls_init(pool_dev, &pool[k]) != 0) { pool[k] = NULL; return ctx; }
  return pool[k];
}
static napi_value Init(napi_env env, napi_callback_info info) {
  size_t argc = 2; napi_value argv[2]; CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1) { napi_throw_type_error(env, NULL, "missing arguments"); return NULL; }
  int32_t dev = 0, nctx = 0; napi_get_value_int32(env, argv[0], &dev);
  napi_valuetype t1 = napi_undefined; if (argc > 1) napi_typeof(env, argv[1], &t1);
  if (t1 == napi_number) napi_get_value_int32(env, argv[1], &nctx);
  else { const char* e = getenv("NBLS_CONTEXTS"); nctx = e ? atoi(e) : 1; }
  if (multi) { p_nbls_destroy_multi(multi); multi = NULL; ctx = NULL; }
  pool_clear();
  if (ctx) { p_nbls_destroy(ctx); ctx = NULL; }
  int r = p_nbls_init(dev, &ctx); if (r) return throw_code(env, r);
  pool[0] = ctx; pool_dev = dev; pool_size = nctx < 1 ? 1 : (nctx > MAX_POOL ? MAX_POOL : nctx);
  napi_value t; napi_get_boolean(env, true, &t); return t;
}
/* initMulti(Int32Array of device ids | null for every visible device) -> number of devices.  pairingBatch, millerProduct and verifyBatch(Async)
 * then shard over all of them (nbls_multi_*, include/nbls.h); every other call runs on the first device. */
static napi_value InitMulti(napi_env env, napi_callback_info info) {
  ARGS(1); napi_valuetype t; napi_typeof(env, argv[0], &t);
  int ids[64]; int n = 0;
  if (t != napi_null && t != napi_undefined) {
    uint8_t* d; size_t l; if (!get_bytes(env, argv[0], &d, &l) || l % 4 || l / 4 > 64) { napi_throw_type_error(env, NULL, "expected Int32Array of at most 64 device ids or null"); return NULL; }
    n = (int)(l / 4); memcpy(ids, d, l);
  }
  if (multi) { p_nbls_destroy_multi(multi); multi = NULL; ctx = NULL; }
  pool_clear(); pool_size = 1;   /* asynchronous calls run on the multi-device handle */
  if (ctx) { p_nbls_destroy(ctx); ctx = NULL; }
  int r = p_nbls_init_multi(n, n ? ids : NULL, &multi); if (r) return throw_code(env, r);
  ctx = p_nbls_multi_context(multi, 0);
  napi_value v; napi_create_int32(env, p_nbls_multi_device_count(multi), &v); return v;
}
/* decodePoints(kind, bytes, len) -> {out, status}: kind 0 PointG1.fromHex, 1 PointG2.fromHex, 2 PointG2.fromSignature; len = bytes per encoded point */
static napi_value DecodePoints(napi_env env, napi_callback_info info) {
  ARGS(3); NEED_CTX(); int32_t kind = 0, len = 0; napi_get_value_int32(env, argv[0], &kind); BYTES(1, in, l); napi_get_value_int32(env, argv[2], &len);
  if (len <= 0 || l % (size_t)len) { napi_throw_range_error(env, NULL, "bad encoded point length"); return NULL; }
  size_t n = l / (size_t)len, a = kind == 0 ? 96 : 192;
  uint8_t *out, *st; napi_value vo = new_u8(env, n * a, &out), vs = new_u8(env, n, &st); ALLOCATED(vo); ALLOCATED(vs);
  int r = kind == 0 ? p_nbls_g1_from_hex_batch(ctx, n, in, (size_t)len, out, (int8_t*)st) : kind == 1 ? p_nbls_g2_from_hex_batch(ctx, n, in, (size_t)len, out, (int8_t*)st)
                    : p_nbls_g2_from_signature_batch(ctx, n, in, (size_t)len, out, (int8_t*)st);
  if (r) return throw_code(env, r); return result2(env, vo, vs);
}
/* clearCofactor(g2, affine points) -> {out, status} */
static napi_value ClearCofactor(napi_env env, napi_callback_info info) {
  ARGS(2); NEED_CTX(); bool g2; napi_get_value_bool(env, argv[0], &g2); BYTES(1, in, l); size_t a = g2 ? 192 : 96, n = l / a;
  if (l != n * a) { napi_throw_range_error(env, NULL, "bad point array length"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, n * a, &out), vs = new_u8(env, n, &st); ALLOCATED(vo); ALLOCATED(vs);
  int r = g2 ? p_nbls_g2_clear_cofactor_batch(ctx, n, in, out, (int8_t*)st) : p_nbls_g1_clear_cofactor_batch(ctx, n, in, out, (int8_t*)st);
  if (r) return throw_code(env, r); return result2(env, vo, vs);
}
/* g2Prepare(g2 affine n*192) -> Uint8Array n*19584: PointG2.pairingPrecomputes() as 68 x [Fp2, Fp2, Fp2] in Fp2.toBytes order */
static napi_value G2Prepare(napi_env env, napi_callback_info info) {
  ARGS(1); NEED_CTX(); BYTES(0, in, l); size_t n = l / 192; if (l != n * 192) { napi_throw_range_error(env, NULL, "bad point array length"); return NULL; }
  uint8_t* out; napi_value vo = new_u8(env, n * NBLS_LINE_WIRE_BYTES, &out); ALLOCATED(vo);
  int r = p_nbls_g2_prepare(ctx, n, in, out); if (r) return throw_code(env, r); return vo;
}
/* pairingPrepared(g1 affine n*96, tables (n or 1)*19584, withFinalExp, product) -> Uint8Array n*576 (or 576 for product) */
static napi_value PairingPrepared(napi_env env, napi_callback_info info) {
  ARGS(4); NEED_CTX(); BYTES(0, g1, l1); BYTES(1, tab, lt); bool fe, prod; napi_get_value_bool(env, argv[2], &fe); napi_get_value_bool(env, argv[3], &prod);
  size_t n = l1 / 96, nt = lt / NBLS_LINE_WIRE_BYTES; if (l1 != n * 96 || lt != nt * NBLS_LINE_WIRE_BYTES || (n && nt != 1 && nt != n)) { napi_throw_range_error(env, NULL, "bad array lengths"); return NULL; }
  uint8_t* out; napi_value vo = new_u8(env, prod ? 576 : n * 576, &out); ALLOCATED(vo);
  int r = p_nbls_pairing_prepared(ctx, n, g1, tab, nt, fe, prod, out); if (r) return throw_code(env, r); return vo;
}
/* pairingBatch(g1, g2, withFinalExp, validate) -> {out, status} */
static napi_value PairingBatch(napi_env env, napi_callback_info info) {
  ARGS(4); NEED_CTX(); BYTES(0, g1, l1); BYTES(1, g2, l2); bool fe, val; napi_get_value_bool(env, argv[2], &fe); napi_get_value_bool(env, argv[3], &val);
  size_t n = l1 / 96; if (l1 != n * 96 || l2 != n * 192) { napi_throw_range_error(env, NULL, "bad point array lengths"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, n * 576, &out), vs = new_u8(env, n, &st);
  ALLOCATED(vo); ALLOCATED(vs);
  int r = MULTI() ? p_nbls_multi_pairing_batch(multi, n, g1, g2, fe, val, out, (int8_t*)st) : p_nbls_pairing_batch(ctx, n, g1, g2, fe, val, out, (int8_t*)st); if (r) return throw_code(env, r);
  return result2(env, vo, vs);
}
/* millerProduct(g1, g2, finalExp, validate) -> {out, status, code} */
static napi_value MillerProduct(napi_env env, napi_callback_info info) {
  ARGS(4); NEED_CTX(); BYTES(0, g1, l1); BYTES(1, g2, l2); bool fe, val; napi_get_value_bool(env, argv[2], &fe); napi_get_value_bool(env, argv[3], &val);
  size_t n = l1 / 96; if (l1 != n * 96 || l2 != n * 192) { napi_throw_range_error(env, NULL, "bad point array lengths"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, 576, &out), vs = new_u8(env, n, &st);
  ALLOCATED(vo); ALLOCATED(vs);
  int r = MULTI() ? p_nbls_multi_miller_product(multi, n, g1, g2, fe, val, out, (int8_t*)st) : p_nbls_miller_product(ctx, n, g1, g2, fe, val, out, (int8_t*)st); if (r && r != NBLS_EDECODE) return throw_code(env, r);
  napi_value o = result2(env, vo, vs), c; napi_create_int32(env, r, &c); napi_set_named_property(env, o, "code", c); return o;
}
static napi_value FinalExpBatch(napi_env env, napi_callback_info info) {
  ARGS(1); NEED_CTX(); BYTES(0, in, l); size_t n = l / 576; uint8_t* out; napi_value vo = new_u8(env, n * 576, &out);
  int r = p_nbls_final_exp_batch(ctx, n, in, out); if (r) return throw_code(env, r); return vo;
}
#define POINT_FN(NAME, CALL, IN_SZ, OUT_SZ) \
  static napi_value NAME(napi_env env, napi_callback_info info) { ARGS(1); NEED_CTX(); BYTES(0, in, l); size_t n = l / (IN_SZ); \
    uint8_t *out, *st; napi_value vo = new_u8(env, n * (OUT_SZ), &out), vs = new_u8(env, n, &st); \
    int r = CALL; if (r) return throw_code(env, r); return result2(env, vo, vs); }
POINT_FN(G1Decompress, p_nbls_g1_decompress_batch(ctx, n, in, out, (int8_t*)st), 48, 96)
POINT_FN(G2Decompress, p_nbls_g2_decompress_batch(ctx, n, in, out, (int8_t*)st), 96, 192)
POINT_FN(G1Validate, p_nbls_g1_validate_batch(ctx, n, in, (int8_t*)st), 96, 0)
POINT_FN(G2Validate, p_nbls_g2_validate_batch(ctx, n, in, (int8_t*)st), 192, 0)
static napi_value G1Sum(napi_env env, napi_callback_info info) { ARGS(1); NEED_CTX(); BYTES(0, in, l); uint8_t *out, *st; napi_value vo = new_u8(env, 96, &out), vs = new_u8(env, 1, &st);
  int r = p_nbls_g1_sum(ctx, l / 96, in, out, (int8_t*)st); if (r) return throw_code(env, r); return result2(env, vo, vs); }
static napi_value G2Sum(napi_env env, napi_callback_info info) { ARGS(1); NEED_CTX(); BYTES(0, in, l); uint8_t *out, *st; napi_value vo = new_u8(env, 192, &out), vs = new_u8(env, 1, &st);
  int r = p_nbls_g2_sum(ctx, l / 192, in, out, (int8_t*)st); if (r) return throw_code(env, r); return result2(env, vo, vs); }
/* hashToG2(msgs, offsets(Uint32Array n+1), dst) -> Uint8Array n*192 */
static napi_value HashToG2(napi_env env, napi_callback_info info) {
  ARGS(3); NEED_CTX(); BYTES(0, msgs, lm); BYTES(1, offs, lo); BYTES(2, dst, ld); COUNT_FROM_OFFSETS(n, lo); (void)lm;
  uint8_t* out; napi_value vo = new_u8(env, n * 192, &out);
  int r = p_nbls_hash_to_g2_batch(ctx, n, msgs, (const uint32_t*)offs, dst, ld, out); if (r) return throw_code(env, r); return vo;
}
/* g1Mul(points96 | null, scalars32) / g2Mul(points192, scalars32) -> {out, status}: [k_i]P_i, G1 generator when points is null */
static napi_value G1Mul(napi_env env, napi_callback_info info) {
  ARGS(2); NEED_CTX(); napi_valuetype t; napi_typeof(env, argv[0], &t); uint8_t* pts = NULL; size_t lp = 0;
  if (t != napi_null && t != napi_undefined && !get_bytes(env, argv[0], &pts, &lp)) { napi_throw_type_error(env, NULL, "expected Uint8Array or null"); return NULL; }
  BYTES(1, sc, ls); size_t n = ls / 32; if (pts && lp != n * 96) { napi_throw_range_error(env, NULL, "bad point array length"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, n * 96, &out), vs = new_u8(env, n, &st);
  int r = p_nbls_g1_mul_batch(ctx, n, pts, sc, out, (int8_t*)st); if (r) return throw_code(env, r); return result2(env, vo, vs);
}
static napi_value G2Mul(napi_env env, napi_callback_info info) {
  ARGS(2); NEED_CTX(); BYTES(0, pts, lp); BYTES(1, sc, ls); size_t n = ls / 32; if (lp != n * 192) { napi_throw_range_error(env, NULL, "bad point array length"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, n * 192, &out), vs = new_u8(env, n, &st);
  int r = p_nbls_g2_mul_batch(ctx, n, pts, sc, out, (int8_t*)st); if (r) return throw_code(env, r); return result2(env, vo, vs);
}
/* g1Msm(points96, scalars32) / g2Msm(points192, scalars32) -> {out: one affine point, status}: sum_i [k_i]P_i (status 1 = zero point) */
static napi_value G1Msm(napi_env env, napi_callback_info info) {
  ARGS(2); NEED_CTX(); BYTES(0, pts, lp); BYTES(1, sc, ls); size_t n = ls / 32; if (lp != n * 96) { napi_throw_range_error(env, NULL, "bad point array length"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, 96, &out), vs = new_u8(env, 1, &st);
  int r = p_nbls_g1_msm(ctx, n, pts, sc, out, (int8_t*)st); if (r) return throw_code(env, r); return result2(env, vo, vs);
}
static napi_value G2Msm(napi_env env, napi_callback_info info) {
  ARGS(2); NEED_CTX(); BYTES(0, pts, lp); BYTES(1, sc, ls); size_t n = ls / 32; if (lp != n * 192) { napi_throw_range_error(env, NULL, "bad point array length"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, 192, &out), vs = new_u8(env, 1, &st);
  int r = p_nbls_g2_msm(ctx, n, pts, sc, out, (int8_t*)st); if (r) return throw_code(env, r); return result2(env, vo, vs);
}
/* signBatch(msgs, offsets(Uint32Array n+1), dst, keys32) -> {out: n*192 affine signature points, status} */
static napi_value SignBatch(napi_env env, napi_callback_info info) {
  ARGS(4); NEED_CTX(); BYTES(0, msgs, lm); BYTES(1, offs, lo); BYTES(2, dst, ld); BYTES(3, keys, lk); (void)lm;
  COUNT_FROM_OFFSETS(n, lo); if (lk != n * 32) { napi_throw_range_error(env, NULL, "bad key array length"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, n * 192, &out), vs = new_u8(env, n, &st);
  int r = p_nbls_sign_batch(ctx, n, msgs, (const uint32_t*)offs, dst, ld, keys, out, (int8_t*)st); if (r) return throw_code(env, r); return result2(env, vo, vs);
}
/* hashToCurve(mode, msgs, offsets, dst): mode 0 = G1 hashToCurve, 1 = G1 encodeToCurve, 2 = G2 encodeToCurve -> Uint8Array n*96 / n*192 */
static napi_value HashToCurve(napi_env env, napi_callback_info info) {
  ARGS(4); NEED_CTX(); int32_t mode = 0; napi_get_value_int32(env, argv[0], &mode); BYTES(1, msgs, lm); BYTES(2, offs, lo); BYTES(3, dst, ld); (void)lm;
  COUNT_FROM_OFFSETS(n, lo); size_t a = mode == 2 ? 192 : 96; uint8_t* out; napi_value vo = new_u8(env, n * a, &out);
  int r = mode == 0 ? p_nbls_hash_to_g1_batch(ctx, n, msgs, (const uint32_t*)offs, dst, ld, out) : mode == 1 ? p_nbls_encode_to_g1_batch(ctx, n, msgs, (const uint32_t*)offs, dst, ld, out)
                    : p_nbls_encode_to_g2_batch(ctx, n, msgs, (const uint32_t*)offs, dst, ld, out);
  if (r) return throw_code(env, r); return vo;
}
/* verifyBatch(sig96, msgs, offsets, pks48, dst) -> {code, ok} */
static napi_value VerifyBatch(napi_env env, napi_callback_info info) {
  ARGS(5); NEED_CTX(); BYTES(0, sig, ls); BYTES(1, msgs, lm); BYTES(2, offs, lo); BYTES(3, pks, lp); BYTES(4, dst, ld); (void)lm; (void)ls;
  COUNT_FROM_OFFSETS(n, lo); if (lp != n * 48) { napi_throw_range_error(env, NULL, "bad public key array length"); return NULL; }
  int ok = 0; int r = MULTI() ? p_nbls_multi_verify_batch(multi, n, sig, msgs, (const uint32_t*)offs, pks, dst, ld, &ok) : p_nbls_verify_batch(ctx, n, sig, msgs, (const uint32_t*)offs, pks, dst, ld, &ok);
  if (r && r != NBLS_EDECODE) return throw_code(env, r);
  napi_value o, c, k; napi_create_object(env, &o); napi_create_int32(env, r, &c); napi_get_boolean(env, ok != 0, &k);
  napi_set_named_property(env, o, "code", c); napi_set_named_property(env, o, "ok", k); return o;
}

/* verifyBatchAsync(sig96, msgs, offsets, pks48, dst) -> Promise<{code, ok}>: the same call on a libuv worker thread (napi_create_async_work),
 * so that the event loop keeps running during the ~1-100 ms a batch takes.  The typed arrays are kept alive by references until
 * the work completes; the engine context serialises concurrent calls itself. */
typedef struct {
  napi_async_work work; napi_deferred deferred; napi_ref refs[5];
  const uint8_t *sig, *msgs, *pks, *dst; const uint32_t* offs; size_t n, dst_len;
  nbls_ctx* c;      /* the pool context this call runs on */
  int rc, ok;
} verify_job;
static void verify_execute(napi_env env, void* data) { verify_job* j = (verify_job*)data; (void)env;
  j->rc = MULTI() ? p_nbls_multi_verify_batch(multi, j->n, j->sig, j->msgs, j->offs, j->pks, j->dst, j->dst_len, &j->ok) : p_nbls_verify_batch(j->c, j->n, j->sig, j->msgs, j->offs, j->pks, j->dst, j->dst_len, &j->ok); }
static void verify_complete(napi_env env, napi_status status, void* data) {
  verify_job* j = (verify_job*)data;
  for (int i = 0; i < 5; i++) napi_delete_reference(env, j->refs[i]);
  if (status != napi_ok || (j->rc && j->rc != NBLS_EDECODE)) {
    char m[128]; snprintf(m, sizeof m, "nbls: %s (code %d)", p_nbls_strerror ? p_nbls_strerror(j->rc) : "error", j->rc);
    napi_value msg, err; napi_create_string_utf8(env, m, NAPI_AUTO_LENGTH, &msg); napi_create_error(env, NULL, msg, &err); napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value o, c, k; napi_create_object(env, &o); napi_create_int32(env, j->rc, &c); napi_get_boolean(env, j->ok != 0, &k);
    napi_set_named_property(env, o, "code", c); napi_set_named_property(env, o, "ok", k); napi_resolve_deferred(env, j->deferred, o);
  }
  napi_delete_async_work(env, j->work); free(j);
}
static napi_value VerifyBatchAsync(napi_env env, napi_callback_info info) {
  ARGS(5); NEED_CTX(); BYTES(0, sig, ls); BYTES(1, msgs, lm); BYTES(2, offs, lo); BYTES(3, pks, lp); BYTES(4, dst, ld); (void)lm; (void)ls;
  COUNT_FROM_OFFSETS(n, lo); if (lp != n * 48) { napi_throw_range_error(env, NULL, "bad public key array length"); return NULL; }
  verify_job* j = (verify_job*)calloc(1, sizeof *j); if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  j->sig = sig; j->msgs = msgs; j->offs = (const uint32_t*)offs; j->pks = pks; j->dst = dst; j->dst_len = ld; j->n = n; j->c = pool_take();
  for (int i = 0; i < 5; i++) napi_create_reference(env, argv[i], 1, &j->refs[i]);
  napi_value promise, name; napi_create_promise(env, &j->deferred, &promise); napi_create_string_utf8(env, "nbls_verify_batch", NAPI_AUTO_LENGTH, &name);
  if (napi_create_async_work(env, NULL, name, verify_execute, verify_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
    for (int i = 0; i < 5; i++) napi_delete_reference(env, j->refs[i]); free(j); napi_throw_error(env, NULL, "napi_create_async_work failed"); return NULL; }
  return promise;
}


/* verifyMultipleAsync(sigs96, msgs, offsets, pks48, dst) -> Promise<{ok, status}>: nbls_verify_multiple (n independent sets, one random linear combination; weights
 * seeded from the OS) on a libuv worker thread with a context of the pool, like verifyBatchAsync.  status: one byte per set (include/nbls.h), made here on the main thread. */
typedef struct {
  napi_async_work work; napi_deferred deferred; napi_ref refs[6];
  const uint8_t *sigs, *msgs, *pks, *dst; const uint32_t* offs; size_t n, dst_len; int8_t* st;
  nbls_ctx* c; int rc, ok;
} multi_verify_job;
static void multi_verify_execute(napi_env env, void* data) { multi_verify_job* j = (multi_verify_job*)data; (void)env;
  j->rc = p_nbls_verify_multiple(j->c, j->n, j->sigs, j->msgs, j->offs, j->pks, j->dst, j->dst_len, NULL, &j->ok, j->st); }
static void multi_verify_complete(napi_env env, napi_status status, void* data) {
  multi_verify_job* j = (multi_verify_job*)data;
  napi_value st = NULL; napi_get_reference_value(env, j->refs[5], &st);
  for (int i = 0; i < 6; i++) napi_delete_reference(env, j->refs[i]);
  if (status != napi_ok || j->rc) {
    char m[128]; snprintf(m, sizeof m, "nbls: %s (code %d)", p_nbls_strerror ? p_nbls_strerror(j->rc) : "error", j->rc);
    napi_value msg, err; napi_create_string_utf8(env, m, NAPI_AUTO_LENGTH, &msg); napi_create_error(env, NULL, msg, &err); napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value o, k; napi_create_object(env, &o); napi_get_boolean(env, j->ok != 0, &k);
    napi_set_named_property(env, o, "ok", k); napi_set_named_property(env, o, "status", st); napi_resolve_deferred(env, j->deferred, o);
  }
  napi_delete_async_work(env, j->work); free(j);
}
static napi_value VerifyMultipleAsync(napi_env env, napi_callback_info info) {
  ARGS(5); NEED_CTX(); BYTES(0, sigs, ls); BYTES(1, msgs, lm); BYTES(2, offs, lo); BYTES(3, pks, lp); BYTES(4, dst, ld); (void)lm;
  COUNT_FROM_OFFSETS(n, lo); if (lp != n * 48 || ls != n * 96) { napi_throw_range_error(env, NULL, "bad signature or public key array length"); return NULL; }
  uint8_t* st; napi_value vst = new_u8(env, n ? n : 1, &st); ALLOCATED(vst);
  multi_verify_job* j = (multi_verify_job*)calloc(1, sizeof *j); if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  j->sigs = sigs; j->msgs = msgs; j->offs = (const uint32_t*)offs; j->pks = pks; j->dst = dst; j->dst_len = ld; j->n = n; j->st = (int8_t*)st; j->c = pool_take();
  for (int i = 0; i < 5; i++) napi_create_reference(env, argv[i], 1, &j->refs[i]);
  napi_create_reference(env, vst, 1, &j->refs[5]);
  napi_value promise, name; napi_create_promise(env, &j->deferred, &promise); napi_create_string_utf8(env, "nbls_verify_multiple", NAPI_AUTO_LENGTH, &name);
  if (napi_create_async_work(env, NULL, name, multi_verify_execute, multi_verify_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
    for (int i = 0; i < 6; i++) napi_delete_reference(env, j->refs[i]); free(j); napi_throw_error(env, NULL, "napi_create_async_work failed"); return NULL; }
  return promise;
}

/* verifyAggregatesAsync(sigs96, msgs, offsets, pks48, keyOffsets, dst) -> Promise<{ok, status}>: nbls_verify_aggregates (set j: the keys pks48[keyOffsets[j] .. keyOffsets[j+1]),
 * one random linear combination over the sets, weights seeded from the OS) on a libuv worker thread with a context of the pool, like verifyMultipleAsync. */
typedef struct {
  napi_async_work work; napi_deferred deferred; napi_ref refs[7];
  const uint8_t *sigs, *msgs, *pks, *dst; const uint32_t *offs, *koffs; size_t n, dst_len; int8_t* st;
  nbls_ctx* c; int rc, ok;
} agg_verify_job;
static void agg_verify_execute(napi_env env, void* data) { agg_verify_job* j = (agg_verify_job*)data; (void)env;
  j->rc = p_nbls_verify_aggregates(j->c, j->n, j->sigs, j->msgs, j->offs, j->pks, j->koffs, j->dst, j->dst_len, NULL, &j->ok, j->st); }
static void agg_verify_complete(napi_env env, napi_status status, void* data) {
  agg_verify_job* j = (agg_verify_job*)data;
  napi_value st = NULL; napi_get_reference_value(env, j->refs[6], &st);
  for (int i = 0; i < 7; i++) napi_delete_reference(env, j->refs[i]);
  if (status != napi_ok || j->rc) {
    char m[128]; snprintf(m, sizeof m, "nbls: %s (code %d)", p_nbls_strerror ? p_nbls_strerror(j->rc) : "error", j->rc);
    napi_value msg, err; napi_create_string_utf8(env, m, NAPI_AUTO_LENGTH, &msg); napi_create_error(env, NULL, msg, &err); napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value o, k; napi_create_object(env, &o); napi_get_boolean(env, j->ok != 0, &k);
    napi_set_named_property(env, o, "ok", k); napi_set_named_property(env, o, "status", st); napi_resolve_deferred(env, j->deferred, o);
  }
  napi_delete_async_work(env, j->work); free(j);
}
static napi_value VerifyAggregatesAsync(napi_env env, napi_callback_info info) {
  ARGS(6); NEED_CTX(); BYTES(0, sigs, ls); BYTES(1, msgs, lm); BYTES(2, offs, lo); BYTES(3, pks, lp); BYTES(4, koffs, lk); BYTES(5, dst, ld); (void)lm;
  COUNT_FROM_OFFSETS(n, lo);
  if (ls != n * 96 || lk != lo) { napi_throw_range_error(env, NULL, "bad signature or key offset array length"); return NULL; }
  if (n) {   /* the keys the offsets name must be in pks48 (the library checks the rest: order, empty sets, count) */
    const uint32_t* ko = (const uint32_t*)koffs;
    if (ko[n] < ko[0] || (size_t)ko[n] * 48 > lp) { napi_throw_range_error(env, NULL, "key offsets run past the public key array"); return NULL; }
  }
  uint8_t* st; napi_value vst = new_u8(env, n ? n : 1, &st); ALLOCATED(vst);
  agg_verify_job* j = (agg_verify_job*)calloc(1, sizeof *j); if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  j->sigs = sigs; j->msgs = msgs; j->offs = (const uint32_t*)offs; j->pks = pks; j->koffs = (const uint32_t*)koffs; j->dst = dst; j->dst_len = ld; j->n = n; j->st = (int8_t*)st;
  j->c = pool_take();
  for (int i = 0; i < 6; i++) napi_create_reference(env, argv[i], 1, &j->refs[i]);
  napi_create_reference(env, vst, 1, &j->refs[6]);
  napi_value promise, name; napi_create_promise(env, &j->deferred, &promise); napi_create_string_utf8(env, "nbls_verify_aggregates", NAPI_AUTO_LENGTH, &name);
  if (napi_create_async_work(env, NULL, name, agg_verify_execute, agg_verify_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
    for (int i = 0; i < 7; i++) napi_delete_reference(env, j->refs[i]); free(j); napi_throw_error(env, NULL, "napi_create_async_work failed"); return NULL; }
  return promise;
}

/* verifyMultipleSharedAsync(sigs96, msgs, offsets, msgIndex, pks48, dst) and verifyAggregatesSharedAsync(sigs96, msgs, offsets, msgIndex, pks48, keyOffsets, dst)
 * -> Promise<{ok, status}>: nbls_verify_multiple_shared / nbls_verify_aggregates_shared (msgs / offsets hold the DISTINCT messages, set i signs message msgIndex[i]: one hash and one
 * Miller loop per message) on a libuv worker thread with a context of the pool, like their twins.  n = the length of msgIndex (a Uint32Array); the library checks the index itself. */
typedef struct {
  napi_async_work work; napi_deferred deferred; napi_ref refs[8]; int nrefs;
  const uint8_t *sigs, *msgs, *pks, *dst; const uint32_t *offs, *idx, *koffs /* NULL: one key per set */; size_t n, n_msgs, dst_len; int8_t* st;
  nbls_ctx* c; int rc, ok;
} shared_verify_job;
static void shared_verify_execute(napi_env env, void* data) { shared_verify_job* j = (shared_verify_job*)data; (void)env;
  j->rc = j->koffs ? p_nbls_verify_aggregates_shared(j->c, j->n, j->sigs, j->n_msgs, j->msgs, j->offs, j->idx, j->pks, j->koffs, j->dst, j->dst_len, NULL, &j->ok, j->st)
                   : p_nbls_verify_multiple_shared(j->c, j->n, j->sigs, j->n_msgs, j->msgs, j->offs, j->idx, j->pks, j->dst, j->dst_len, NULL, &j->ok, j->st); }
static void shared_verify_complete(napi_env env, napi_status status, void* data) {
  shared_verify_job* j = (shared_verify_job*)data;
  napi_value st = NULL; napi_get_reference_value(env, j->refs[j->nrefs - 1], &st);
  for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
  if (status != napi_ok || j->rc) {
    char m[128]; snprintf(m, sizeof m, "nbls: %s (code %d)", p_nbls_strerror ? p_nbls_strerror(j->rc) : "error", j->rc);
    napi_value msg, err; napi_create_string_utf8(env, m, NAPI_AUTO_LENGTH, &msg); napi_create_error(env, NULL, msg, &err); napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value o, k; napi_create_object(env, &o); napi_get_boolean(env, j->ok != 0, &k);
    napi_set_named_property(env, o, "ok", k); napi_set_named_property(env, o, "status", st); napi_resolve_deferred(env, j->deferred, o);
  }
  napi_delete_async_work(env, j->work); free(j);
}
static napi_value shared_verify_queue(napi_env env, shared_verify_job* j, napi_value* argv, int nargs, napi_value vst, const char* what) {
  j->c = pool_take(); j->nrefs = nargs + 1;
  for (int i = 0; i < nargs; i++) napi_create_reference(env, argv[i], 1, &j->refs[i]);
  napi_create_reference(env, vst, 1, &j->refs[nargs]);
  napi_value promise, name; napi_create_promise(env, &j->deferred, &promise); napi_create_string_utf8(env, what, NAPI_AUTO_LENGTH, &name);
  if (napi_create_async_work(env, NULL, name, shared_verify_execute, shared_verify_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
    for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]); free(j); napi_throw_error(env, NULL, "napi_create_async_work failed"); return NULL; }
  return promise;
}
static napi_value VerifyMultipleSharedAsync(napi_env env, napi_callback_info info) {
  ARGS(6); NEED_CTX(); BYTES(0, sigs, ls); BYTES(1, msgs, lm); BYTES(2, offs, lo); BYTES(3, idx, li); BYTES(4, pks, lp); BYTES(5, dst, ld); (void)lm;
  COUNT_FROM_OFFSETS(n_msgs, lo);
  const size_t n = li / 4;
  if (li % 4 || lp != n * 48 || ls != n * 96) { napi_throw_range_error(env, NULL, "bad message index, signature or public key array length"); return NULL; }
  uint8_t* st; napi_value vst = new_u8(env, n ? n : 1, &st); ALLOCATED(vst);
  shared_verify_job* j = (shared_verify_job*)calloc(1, sizeof *j); if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  j->sigs = sigs; j->msgs = msgs; j->offs = (const uint32_t*)offs; j->idx = (const uint32_t*)idx; j->pks = pks; j->dst = dst; j->dst_len = ld; j->n = n; j->n_msgs = n_msgs; j->st = (int8_t*)st;
  return shared_verify_queue(env, j, argv, 6, vst, "nbls_verify_multiple_shared");
}
static napi_value VerifyAggregatesSharedAsync(napi_env env, napi_callback_info info) {
  ARGS(7); NEED_CTX(); BYTES(0, sigs, ls); BYTES(1, msgs, lm); BYTES(2, offs, lo); BYTES(3, idx, li); BYTES(4, pks, lp); BYTES(5, koffs, lk); BYTES(6, dst, ld); (void)lm;
  COUNT_FROM_OFFSETS(n_msgs, lo);
  const size_t n = li / 4;
  if (li % 4 || ls != n * 96 || lk != (n + 1) * 4) { napi_throw_range_error(env, NULL, "bad message index, signature or key offset array length"); return NULL; }
  {   /* the keys the offsets name must be in pks48 (the library checks the rest: order, empty sets, count) */
    const uint32_t* ko = (const uint32_t*)koffs;
    if (ko[n] < ko[0] || (size_t)ko[n] * 48 > lp) { napi_throw_range_error(env, NULL, "key offsets run past the public key array"); return NULL; }
  }
  uint8_t* st; napi_value vst = new_u8(env, n ? n : 1, &st); ALLOCATED(vst);
  shared_verify_job* j = (shared_verify_job*)calloc(1, sizeof *j); if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  j->sigs = sigs; j->msgs = msgs; j->offs = (const uint32_t*)offs; j->idx = (const uint32_t*)idx; j->pks = pks; j->koffs = (const uint32_t*)koffs; j->dst = dst; j->dst_len = ld; j->n = n;
  j->n_msgs = n_msgs; j->st = (int8_t*)st;
  return shared_verify_queue(env, j, argv, 7, vst, "nbls_verify_aggregates_shared");
}

/* signBatchAsync(msgs, offsets, dst, keys32) -> Promise<{out: n*192 affine signature points, status}>: nbls_sign_batch on a libuv worker thread (the reference's
 * sign is async, index.ts:744-752).  The output arrays are created here, on the main thread, and kept alive by references like the inputs. */
typedef struct {
  napi_async_work work; napi_deferred deferred; napi_ref refs[6];
  const uint8_t *msgs, *dst, *keys; const uint32_t* offs; size_t n, dst_len; uint8_t *out; int8_t* st;
  nbls_ctx* c; int rc;
} sign_job;
static void sign_execute(napi_env env, void* data) { sign_job* j = (sign_job*)data; (void)env;
  j->rc = p_nbls_sign_batch(j->c, j->n, j->msgs, j->offs, j->dst, j->dst_len, j->keys, j->out, j->st); }
static void sign_complete(napi_env env, napi_status status, void* data) {
  sign_job* j = (sign_job*)data;
  if (status != napi_ok || j->rc) {
    char m[128]; snprintf(m, sizeof m, "nbls: %s (code %d)", p_nbls_strerror ? p_nbls_strerror(j->rc) : "error", j->rc);
    napi_value msg, err; napi_create_string_utf8(env, m, NAPI_AUTO_LENGTH, &msg); napi_create_error(env, NULL, msg, &err); napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value vo, vs; napi_get_reference_value(env, j->refs[4], &vo); napi_get_reference_value(env, j->refs[5], &vs);
    napi_resolve_deferred(env, j->deferred, result2(env, vo, vs));
  }
  for (int i = 0; i < 6; i++) napi_delete_reference(env, j->refs[i]);
  napi_delete_async_work(env, j->work); free(j);
}
static napi_value SignBatchAsync(napi_env env, napi_callback_info info) {
  ARGS(4); NEED_CTX(); BYTES(0, msgs, lm); BYTES(1, offs, lo); BYTES(2, dst, ld); BYTES(3, keys, lk); (void)lm;
  COUNT_FROM_OFFSETS(n, lo); if (lk != n * 32) { napi_throw_range_error(env, NULL, "bad key array length"); return NULL; }
  sign_job* j = (sign_job*)calloc(1, sizeof *j); if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, n * 192, &out), vs = new_u8(env, n, &st);
  j->msgs = msgs; j->offs = (const uint32_t*)offs; j->dst = dst; j->dst_len = ld; j->keys = keys; j->n = n; j->out = out; j->st = (int8_t*)st; j->c = pool_take();
  for (int i = 0; i < 4; i++) napi_create_reference(env, argv[i], 1, &j->refs[i]);
  napi_create_reference(env, vo, 1, &j->refs[4]); napi_create_reference(env, vs, 1, &j->refs[5]);
  napi_value promise, name; napi_create_promise(env, &j->deferred, &promise); napi_create_string_utf8(env, "nbls_sign_batch", NAPI_AUTO_LENGTH, &name);
  if (napi_create_async_work(env, NULL, name, sign_execute, sign_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
    for (int i = 0; i < 6; i++) napi_delete_reference(env, j->refs[i]); free(j); napi_throw_error(env, NULL, "napi_create_async_work failed"); return NULL; }
  return promise;
}

/* The scalar field and threshold recombination (nbls_fr_op_batch, nbls_lagrange_at_zero, nbls_g2_combine_shares / nbls_g1_combine_shares), each as a synchronous native and an
 * *Async twin on a libuv worker thread with a context of the pool -> {out, status}:
 *   frOp(op, a32, b32 | null)                          n = a32.length / 32 elements; status[i] = 5 where inv / div meets 0 mod r
 *   lagrangeAtZero(groupOffsets, ids32)                groupOffsets: Uint32Array of groups + 1 entries; out = one coefficient per identifier, status per group
 *   combineShares(g2, groupOffsets, ids32, shares)     g2 != 0: 96-byte signature shares, else 48-byte public-key shares; out = one compressed point per group, status per group
 *   polyEval(g2, coefOffsets, coefs, idOffsets, ids32) nbls_g*_poly_eval: commitment polynomials (g2 != 0: 96-byte coefficients, else 48-byte ones, lowest degree first) at the
 *                                                      identifiers of their groups; out = one compressed point per identifier, status per identifier
 * The offsets must name identifiers and shares that are in the arrays (checked here); the library checks the rest. */
typedef struct {
  napi_async_work work; napi_deferred deferred; napi_ref refs[12]; int nrefs;
  int kind /* 0 frOp, 1 lagrangeAtZero, 2 combineShares, 3 polyEval, 4 kzgVerifyProofs, 5 kzgVerifyBlobs, 6 .. 8 kzgProve, 9 frNtt, 10 kzgComputeCells, 11 kzgCellsAndProofs, 12 kzgVerifyCells, 13 kzgRecoverCells, 14 kzgRecoverCellsAndProofs, 15 groth16Verify */, op, g2; const uint8_t *a, *b, *shares; const uint32_t *offs, *coffs; size_t n;
  uint8_t* out; int8_t* st;
  const uint8_t *proofs, *tau, *seed; int per_item;   /* KZG: a = commitments, b = z (proofs) or the blobs, shares = y, op = log2_n; out = the verdict as one int */
  const nbls_kzg_setup* su;   /* kzgProve: b = the blobs, a = the points z (7) or the given commitments (8; may be NULL), out = two arrays of n entries one behind the other */
  const nbls_kzg_monomial* mo; size_t proofs_at;   /* PeerDAS: op = log2_n, g2 = the direction (9) or log2_cell (10, 11), b = the rows or the blobs, a = the shifts (9; may be NULL); 11: out = the cells, then at proofs_at the proofs; 12: a = the commitments (proofs_at of them), offs / coffs = the commitment and cell indices, b = the cells, proofs / tau / seed / per_item as the other verifiers; 13, 14: offs / coffs = the cell offsets (n + 1) and the cell indices, b = the given cells, out as 10 / 11 */
  const nbls_groth16_vk* vk;   /* groth16Verify: proofs = the n proofs of 192 bytes, b = the n rows of inputs, seed / per_item as the KZG verifiers; out = the verdict as one int */
  nbls_ctx* c; int rc;
} thr_job;
static void thr_execute(napi_env env, void* data) { thr_job* j = (thr_job*)data; (void)env;
  j->rc = j->kind == 0 ? p_nbls_fr_op_batch(j->c, j->op, j->n, j->a, j->b, j->out, j->st)
        : j->kind == 1 ? p_nbls_lagrange_at_zero(j->c, j->n, j->offs, j->a, j->out, j->st)
        : j->kind == 4 ? p_nbls_kzg_verify_proofs(j->c, j->n, j->a, j->b, j->shares, j->proofs, j->tau, j->seed, (int*)j->out, j->per_item ? j->st : NULL)
        : j->kind == 5 ? p_nbls_kzg_verify_blobs(j->c, (unsigned)j->op, j->n, j->b, j->a, j->proofs, j->tau, j->seed, (int*)j->out, j->per_item ? j->st : NULL)
        : j->kind == 6 ? p_nbls_kzg_commit_blobs(j->c, j->su, j->n, j->b, j->out, j->st)
        : j->kind == 7 ? p_nbls_kzg_compute_proofs(j->c, j->su, j->n, j->b, j->a, j->out, j->out + 48 * j->n, j->st)
        : j->kind == 8 ? p_nbls_kzg_compute_blob_proofs(j->c, j->su, j->n, j->b, j->a, j->out, j->out + 48 * j->n, j->st)
        : j->kind == 9 ? p_nbls_fr_ntt(j->c, (unsigned)j->op, j->g2, j->n, j->b, j->a, j->out, j->st)
        : j->kind == 10 ? p_nbls_kzg_compute_cells(j->c, (unsigned)j->op, (unsigned)j->g2, j->n, j->b, j->out, j->st)
        : j->kind == 11 ? p_nbls_kzg_compute_cells_and_proofs(j->c, j->mo, (unsigned)j->g2, j->n, j->b, j->out, j->out + j->proofs_at, j->st)
        : j->kind == 12 ? p_nbls_kzg_verify_cells(j->c, j->mo, (unsigned)j->g2, j->proofs_at, j->a, j->n, j->offs, j->coffs, j->b, j->proofs, j->tau, j->seed, (int*)j->out, j->per_item ? j->st : NULL)
        : j->kind == 13 ? p_nbls_kzg_recover_cells(j->c, (unsigned)j->op, (unsigned)j->g2, j->n, j->offs, j->coffs, j->b, j->out, j->st)
        : j->kind == 14 ? p_nbls_kzg_recover_cells_and_proofs(j->c, j->mo, (unsigned)j->g2, j->n, j->offs, j->coffs, j->b, j->out, j->out + j->proofs_at, j->st)
        : j->kind == 15 ? p_nbls_groth16_verify(j->c, j->vk, j->n, j->proofs, j->b, j->seed, (int*)j->out, j->per_item ? j->st : NULL)
        : j->kind == 3 ? (j->g2 ? p_nbls_g2_poly_eval : p_nbls_g1_poly_eval)(j->c, j->n, j->coffs, j->shares, j->offs, j->a, j->out, j->st)
        : (j->g2 ? p_nbls_g2_combine_shares : p_nbls_g1_combine_shares)(j->c, j->n, j->offs, j->a, j->shares, j->out, j->st); }
/* the Error of a failed call of this family: the message of throw_code, and the library's return code as the number `nblsCode` (what the facade reads: never the text) */
static napi_value thr_error(napi_env env, int rc) {
  char m[128]; snprintf(m, sizeof m, "nbls: %s (code %d)", p_nbls_strerror ? p_nbls_strerror(rc) : "error", rc);
  napi_value msg, err, code; napi_create_string_utf8(env, m, NAPI_AUTO_LENGTH, &msg); napi_create_error(env, NULL, msg, &err);
  napi_create_int32(env, rc, &code); napi_set_named_property(env, err, "nblsCode", code);
  return err;
}
static void thr_complete(napi_env env, napi_status status, void* data) {
  thr_job* j = (thr_job*)data;
  if (status != napi_ok || j->rc) {
    napi_reject_deferred(env, j->deferred, thr_error(env, j->rc));
  } else {
    napi_value vo, vs; napi_get_reference_value(env, j->refs[j->nrefs - 2], &vo); napi_get_reference_value(env, j->refs[j->nrefs - 1], &vs);
    napi_resolve_deferred(env, j->deferred, result2(env, vo, vs));
  }
  for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
  napi_delete_async_work(env, j->work); free(j);
}
/* runs the job here (async == 0) or queues it; vo / vs: the output arrays, made by the caller on the main thread */
static napi_value thr_run(napi_env env, thr_job* job, int async, napi_value* argv, int nargs, napi_value vo, napi_value vs) {
  if (!async) { job->c = ctx; thr_execute(env, job); if (job->rc) { napi_throw(env, thr_error(env, job->rc)); return NULL; } return result2(env, vo, vs); }
  thr_job* j = (thr_job*)calloc(1, sizeof *j); if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  *j = *job; j->c = pool_take(); j->nrefs = nargs + 2;
  for (int i = 0; i < nargs; i++) napi_create_reference(env, argv[i], 1, &j->refs[i]);
  napi_create_reference(env, vo, 1, &j->refs[nargs]); napi_create_reference(env, vs, 1, &j->refs[nargs + 1]);
  napi_value promise, name; napi_create_promise(env, &j->deferred, &promise); napi_create_string_utf8(env, "nbls_threshold", NAPI_AUTO_LENGTH, &name);
  if (napi_create_async_work(env, NULL, name, thr_execute, thr_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
    for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]); free(j); napi_throw_error(env, NULL, "napi_create_async_work failed"); return NULL; }
  return promise;
}
static napi_value fr_op_call(napi_env env, napi_callback_info info, int async) {
  ARGS(3); NEED_CTX(); BYTES(1, a, la);
  int32_t op; if (napi_get_value_int32(env, argv[0], &op) != napi_ok) { napi_throw_type_error(env, NULL, "expected an operation number"); return NULL; }
  uint8_t* b = NULL; size_t lb = 0;
  napi_valuetype t; napi_typeof(env, argv[2], &t);
  if (t != napi_null && t != napi_undefined && !get_bytes(env, argv[2], &b, &lb)) { napi_throw_type_error(env, NULL, "expected Uint8Array or null"); return NULL; }
  if (la % 32 || (b && lb != la)) { napi_throw_range_error(env, NULL, "operands are 32 bytes each, as many second operands as first ones"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 0; job.op = op; job.a = a; job.b = b; job.n = la / 32;
  napi_value vo = new_u8(env, la ? la : 1, &job.out), vs = new_u8(env, job.n ? job.n : 1, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  return thr_run(env, &job, async, argv + 1, b ? 2 : 1, vo, vs);   /* references to the arrays only */
}
static napi_value FrOp(napi_env env, napi_callback_info info) { return fr_op_call(env, info, 0); }
static napi_value FrOpAsync(napi_env env, napi_callback_info info) { return fr_op_call(env, info, 1); }
/* groups + 1 offsets whose last entry stays inside `have` items */
static int thr_offsets_ok(const uint8_t* offs, size_t lo, size_t have, size_t* groups) {
  if (lo < 8 || lo % 4) return 0;
  *groups = lo / 4 - 1;
  return (size_t)((const uint32_t*)offs)[*groups] <= have;
}
static napi_value lagrange_call(napi_env env, napi_callback_info info, int async) {
  ARGS(2); NEED_CTX(); BYTES(0, offs, lo); BYTES(1, ids, li);
  size_t m;
  if (li % 32 || !thr_offsets_ok(offs, lo, li / 32, &m)) { napi_throw_range_error(env, NULL, "bad group offsets or identifier array length"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 1; job.offs = (const uint32_t*)offs; job.a = ids; job.n = m;
  napi_value vo = new_u8(env, li ? li : 1, &job.out), vs = new_u8(env, m, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  return thr_run(env, &job, async, argv, 2, vo, vs);
}
static napi_value LagrangeAtZero(napi_env env, napi_callback_info info) { return lagrange_call(env, info, 0); }
static napi_value LagrangeAtZeroAsync(napi_env env, napi_callback_info info) { return lagrange_call(env, info, 1); }
static napi_value combine_call(napi_env env, napi_callback_info info, int async) {
  ARGS(4); NEED_CTX(); BYTES(1, offs, lo); BYTES(2, ids, li); BYTES(3, shares, ls);
  int32_t g2; if (napi_get_value_int32(env, argv[0], &g2) != napi_ok) { napi_throw_type_error(env, NULL, "expected 0 (G1) or 1 (G2)"); return NULL; }
  const size_t e = g2 ? 96 : 48; size_t m;
  if (li % 32 || ls != li / 32 * e || !thr_offsets_ok(offs, lo, li / 32, &m)) { napi_throw_range_error(env, NULL, "bad group offsets, identifier or share array length"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 2; job.g2 = g2 != 0; job.offs = (const uint32_t*)offs; job.a = ids; job.shares = shares; job.n = m;
  napi_value vo = new_u8(env, m * e, &job.out), vs = new_u8(env, m, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  return thr_run(env, &job, async, argv + 1, 3, vo, vs);
}
static napi_value CombineShares(napi_env env, napi_callback_info info) { return combine_call(env, info, 0); }
static napi_value CombineSharesAsync(napi_env env, napi_callback_info info) { return combine_call(env, info, 1); }
static napi_value poly_call(napi_env env, napi_callback_info info, int async) {
  ARGS(5); NEED_CTX(); BYTES(1, coffs, lc); BYTES(2, coefs, lf); BYTES(3, offs, lo); BYTES(4, ids, li);
  int32_t g2; if (napi_get_value_int32(env, argv[0], &g2) != napi_ok) { napi_throw_type_error(env, NULL, "expected 0 (G1) or 1 (G2)"); return NULL; }
  const size_t e = g2 ? 96 : 48; size_t m, mc;
  if (li % 32 || lf % e || !thr_offsets_ok(offs, lo, li / 32, &m) || !thr_offsets_ok(coffs, lc, lf / e, &mc) || mc != m) {
    napi_throw_range_error(env, NULL, "bad coefficient or identifier offsets, coefficient or identifier array length"); return NULL; }
  const size_t n = li / 32;
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 3; job.g2 = g2 != 0; job.coffs = (const uint32_t*)coffs; job.shares = coefs; job.offs = (const uint32_t*)offs; job.a = ids; job.n = m;
  napi_value vo = new_u8(env, n ? n * e : 1, &job.out), vs = new_u8(env, n ? n : 1, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  return thr_run(env, &job, async, argv + 1, 4, vo, vs);
}
static napi_value PolyEval(napi_env env, napi_callback_info info) { return poly_call(env, info, 0); }
static napi_value PolyEvalAsync(napi_env env, napi_callback_info info) { return poly_call(env, info, 1); }

/* KZG (nbls_kzg_verify_proofs / nbls_kzg_verify_blobs), synchronous and *Async -> {out, status}: out = the verdict (4 bytes, a native int: non-zero = every item verified),
 * status = one byte per item (all-zero when perItem is 0 and the call stopped after the combined check)
 *   kzgVerifyProofs(commitments48, z32, y32, proofs48, tauG2, seed32 | null, perItem)
 *   kzgVerifyBlobs(log2n, blobs, commitments48, proofs48, tauG2, seed32 | null, perItem) */
static int kzg_seed(napi_env env, napi_value v, const uint8_t** seed) {
  napi_valuetype t; napi_typeof(env, v, &t);
  *seed = NULL;
  if (t == napi_null || t == napi_undefined) return 1;
  uint8_t* p; size_t l;
  if (!get_bytes(env, v, &p, &l) || l != 32) { napi_throw_type_error(env, NULL, "expected a 32-byte seed or null"); return 0; }
  *seed = p; return 1;
}
static napi_value kzg_proofs_call(napi_env env, napi_callback_info info, int async) {
  ARGS(7); NEED_CTX(); BYTES(0, cs, lc); BYTES(1, z, lz); BYTES(2, y, ly); BYTES(3, ps, lp); BYTES(4, tau, lt);
  const uint8_t* seed; if (!kzg_seed(env, argv[5], &seed)) return NULL;
  int32_t per; if (napi_get_value_int32(env, argv[6], &per) != napi_ok) { napi_throw_type_error(env, NULL, "expected 0 or 1"); return NULL; }
  const size_t n = lc / 48;
  if (!n || lc != n * 48 || lp != lc || lz != n * 32 || ly != lz || lt != 96) { napi_throw_range_error(env, NULL, "n commitments and proofs of 48 bytes, n points and values of 32 bytes, 96 bytes of [tau]G2"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 4; job.a = cs; job.b = z; job.shares = y; job.proofs = ps; job.tau = tau; job.seed = seed; job.per_item = per != 0; job.n = n;
  napi_value vo = new_u8(env, 4, &job.out), vs = new_u8(env, n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.out, 0, 4); memset(job.st, 0, n);
  return thr_run(env, &job, async, argv, seed ? 6 : 5, vo, vs);
}
static napi_value KzgVerifyProofs(napi_env env, napi_callback_info info) { return kzg_proofs_call(env, info, 0); }
static napi_value KzgVerifyProofsAsync(napi_env env, napi_callback_info info) { return kzg_proofs_call(env, info, 1); }
static napi_value kzg_blobs_call(napi_env env, napi_callback_info info, int async) {
  ARGS(7); NEED_CTX(); BYTES(1, blobs, lb); BYTES(2, cs, lc); BYTES(3, ps, lp); BYTES(4, tau, lt);
  int32_t log2n, per;
  if (napi_get_value_int32(env, argv[0], &log2n) != napi_ok || napi_get_value_int32(env, argv[6], &per) != napi_ok) { napi_throw_type_error(env, NULL, "expected numbers for log2n and perItem"); return NULL; }
  const uint8_t* seed; if (!kzg_seed(env, argv[5], &seed)) return NULL;
  const size_t n = lc / 48;
  if (log2n < 1 || log2n > 12 || !n || lc != n * 48 || lp != lc || lb != (n * 32) << log2n || lt != 96) {
    napi_throw_range_error(env, NULL, "log2n in 1 .. 12, n blobs of 32 << log2n bytes, n commitments and proofs of 48 bytes, 96 bytes of [tau]G2"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 5; job.op = log2n; job.b = blobs; job.a = cs; job.proofs = ps; job.tau = tau; job.seed = seed; job.per_item = per != 0; job.n = n;
  napi_value vo = new_u8(env, 4, &job.out), vs = new_u8(env, n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.out, 0, 4); memset(job.st, 0, n);
  return thr_run(env, &job, async, argv + 1, seed ? 5 : 4, vo, vs);
}
static napi_value KzgVerifyBlobs(napi_env env, napi_callback_info info) { return kzg_blobs_call(env, info, 0); }
static napi_value KzgVerifyBlobsAsync(napi_env env, napi_callback_info info) { return kzg_blobs_call(env, info, 1); }

/* The KZG prover (nbls_kzg_setup_*, nbls_kzg_commit_blobs / _compute_proofs / _compute_blob_proofs):
 *   kzgSetupCreate(log2n, lagrange48) -> a handle (the setup's Lagrange basis on the device; freed by kzgSetupDestroy or with the handle); a refused setup throws with the
 *                                        per-entry decoder statuses as the Error's `status`
 *   kzgSetupDestroy(handle)              frees it now; the handle is dead afterwards.  Not while an asynchronous call uses it
 *   kzgProve(kind, handle, blobs, aux)   kind 0: commitments (aux null) -> out = n x 48; 1: proofs at the points aux = z32 -> out = n x 48 proofs, then n x 32 values y;
 *                                        2: blob proofs, aux = the commitments or null -> out = n x 48 commitments, then n x 48 proofs.  status = one byte per blob.  + Async */
/* The device handles (a Lagrange setup, a monomial setup, a Groth16 verifying key, a Groth16 proving key) travel as one kind of external: a box that knows which destroy function its handle takes.  h == NULL:
 * destroyed already.  box_wrap is the tail of the three create calls: a refused create throws the library's error with the statuses as `status`; else the handle is wrapped,
 * or destroyed where it cannot be */
typedef enum { BOX_SETUP, BOX_MONOMIAL, BOX_G16_VK, BOX_G16_PK } box_kind;
typedef struct { void* h; box_kind kind; } handle_box;
static void box_destroy(handle_box* b) {
  if (!b->h) return;
  if (b->kind == BOX_SETUP) { if (p_nbls_kzg_setup_destroy) p_nbls_kzg_setup_destroy((nbls_kzg_setup*)b->h); }
  else if (b->kind == BOX_MONOMIAL) { if (p_nbls_kzg_monomial_destroy) p_nbls_kzg_monomial_destroy((nbls_kzg_monomial*)b->h); }
  else if (b->kind == BOX_G16_PK) { if (p_nbls_groth16_pk_destroy) p_nbls_groth16_pk_destroy((nbls_groth16_pk*)b->h); }
  else if (p_nbls_groth16_vk_destroy) p_nbls_groth16_vk_destroy((nbls_groth16_vk*)b->h);
  b->h = NULL;
}
static void box_finalize(napi_env env, void* data, void* hint) { (void)env; (void)hint; box_destroy((handle_box*)data); free(data); }
static handle_box* box_new(napi_env env, box_kind kind) {
  handle_box* box = (handle_box*)calloc(1, sizeof *box);
  if (!box) napi_throw_error(env, NULL, "out of memory"); else box->kind = kind;
  return box;
}
static napi_value box_wrap(napi_env env, handle_box* box, int rc, napi_value vs) {
  if (rc) { free(box); napi_value err = thr_error(env, rc); napi_set_named_property(env, err, "status", vs); napi_throw(env, err); return NULL; }
  napi_value h;
  if (napi_create_external(env, box, box_finalize, NULL, &h) != napi_ok) { box_destroy(box); free(box); napi_throw_error(env, NULL, "napi_create_external failed"); return NULL; }
  return h;
}
static napi_value box_destroy_call(napi_env env, napi_callback_info info, const char* expected) {
  ARGS(1);
  handle_box* box = NULL;
  if (napi_get_value_external(env, argv[0], (void**)&box) != napi_ok || !box) { napi_throw_type_error(env, NULL, expected); return NULL; }
  box_destroy(box);
  return NULL;
}
static napi_value KzgSetupCreate(napi_env env, napi_callback_info info) {
  ARGS(2); NEED_CTX(); BYTES(1, pts, lp);
  int32_t log2n; if (napi_get_value_int32(env, argv[0], &log2n) != napi_ok) { napi_throw_type_error(env, NULL, "expected a number for log2n"); return NULL; }
  if (log2n < 1 || log2n > 12 || lp != (size_t)48 << log2n) { napi_throw_range_error(env, NULL, "log2n in 1 .. 12 and 48 << log2n bytes of compressed points"); return NULL; }
  uint8_t* st; napi_value vs = new_u8(env, (size_t)1 << log2n, &st); ALLOCATED(vs);
  handle_box* box = box_new(env, BOX_SETUP); if (!box) return NULL;
  nbls_kzg_setup* su = NULL;
  const int rc = p_nbls_kzg_setup_create(ctx, (unsigned)log2n, pts, (int8_t*)st, &su);
  box->h = su;
  return box_wrap(env, box, rc, vs);
}
static napi_value KzgSetupDestroy(napi_env env, napi_callback_info info) { return box_destroy_call(env, info, "expected a setup handle"); }
static napi_value kzg_prove_call(napi_env env, napi_callback_info info, int async) {
  ARGS(4); NEED_CTX(); BYTES(2, blobs, lb);
  int32_t kind; if (napi_get_value_int32(env, argv[0], &kind) != napi_ok || kind < 0 || kind > 2) { napi_throw_type_error(env, NULL, "expected the kind 0, 1 or 2"); return NULL; }
  handle_box* box = NULL;
  if (napi_get_value_external(env, argv[1], (void**)&box) != napi_ok || !box || !box->h) { napi_throw_type_error(env, NULL, "expected a live setup handle"); return NULL; }
  unsigned log2n = 0; p_nbls_kzg_setup_log2n((nbls_kzg_setup*)box->h, &log2n);
  uint8_t* aux = NULL; size_t la = 0;
  napi_valuetype t; napi_typeof(env, argv[3], &t);
  if (t != napi_null && t != napi_undefined && !get_bytes(env, argv[3], &aux, &la)) { napi_throw_type_error(env, NULL, "expected Uint8Array or null"); return NULL; }
  const size_t n = lb >> (5 + log2n);
  if (!n || lb != (n * 32) << log2n || (kind == 0 && aux) || (kind == 1 && (!aux || la != n * 32)) || (kind == 2 && aux && la != n * 48)) {
    napi_throw_range_error(env, NULL, "n blobs of 32 << log2n bytes; n points of 32 bytes (proofs) or n commitments of 48 bytes or null (blob proofs)"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 6 + kind; job.su = (nbls_kzg_setup*)box->h; job.b = blobs; job.a = aux; job.n = n;
  const size_t lo = kind == 0 ? n * 48 : kind == 1 ? n * 80 : n * 96;
  napi_value vo = new_u8(env, lo, &job.out), vs = new_u8(env, n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.out, 0, lo); memset(job.st, 0, n);
  return thr_run(env, &job, async, argv + 1, aux ? 3 : 2, vo, vs);   /* the handle stays referenced while the call runs */
}
static napi_value KzgProve(napi_env env, napi_callback_info info) { return kzg_prove_call(env, info, 0); }
static napi_value KzgProveAsync(napi_env env, napi_callback_info info) { return kzg_prove_call(env, info, 1); }

/* PeerDAS (nbls_fr_ntt, nbls_kzg_compute_cells, nbls_kzg_monomial_*, nbls_kzg_compute_cells_and_proofs), synchronous and *Async -> {out, status}:
 *   frNtt(log2n, dir, rows, shifts32 | null)          dir 0: values -> coefficients, 1: the way back; out = the transformed rows, status per polynomial
 *   kzgComputeCells(log2n, log2cell, blobs)            out = per blob its 2 N elements in cell order, status per blob
 *   kzgMonomialCreate(log2n, monomial48) -> a handle   (the setup's monomial basis on the device; kzgMonomialDestroy(handle) or the handle's end frees it); a refused basis
 *                                                      throws with the per-entry decoder statuses as the Error's `status`
 *   kzgCellsAndProofs(handle, log2cell, blobs)         out = the cells of every blob, then n * (2 N / c) proofs of 48 bytes; status per blob
 *   kzgVerifyCells(handle, log2cell, commitments48, commitmentIndex, cellIndex, cells, proofs48, tauCG2, seed32 | null, perItem)
 *                                                      nbls_kzg_verify_cells: the two index arrays are Uint32Arrays of one entry per cell; out = the verdict (4 bytes, a native
 *                                                      int), status per cell, as kzgVerifyProofs
 *   kzgRecoverCells(log2n, log2cell, cellOffsets, cellIndex, cells)
 *   kzgRecoverCellsAndProofs(handle, log2cell, cellOffsets, cellIndex, cells)
 *                                                      nbls_kzg_recover_cells / _and_proofs: cellOffsets = Uint32Array of blobs + 1 entries, cellIndex = Uint32Array of one
 *                                                      entry per given cell (checked here: the offsets start at 0, do not decrease and name cells that are in the arrays); out
 *                                                      and status as kzgComputeCells / kzgCellsAndProofs */
static napi_value fr_ntt_call(napi_env env, napi_callback_info info, int async) {
  ARGS(4); NEED_CTX(); BYTES(2, rows, lr);
  int32_t log2n, dir;
  if (napi_get_value_int32(env, argv[0], &log2n) != napi_ok || napi_get_value_int32(env, argv[1], &dir) != napi_ok) { napi_throw_type_error(env, NULL, "expected numbers for log2n and the direction"); return NULL; }
  uint8_t* sh = NULL; size_t ls = 0;
  napi_valuetype t; napi_typeof(env, argv[3], &t);
  if (t != napi_null && t != napi_undefined && !get_bytes(env, argv[3], &sh, &ls)) { napi_throw_type_error(env, NULL, "expected Uint8Array or null"); return NULL; }
  if (log2n < 1 || log2n > 12 || (dir != 0 && dir != 1) || lr % ((size_t)32 << log2n) || (sh && ls != (lr >> log2n))) {
    napi_throw_range_error(env, NULL, "log2n in 1 .. 12, direction 0 or 1, rows of 32 << log2n bytes, one shift of 32 bytes per row or null"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 9; job.op = log2n; job.g2 = dir; job.b = rows; job.a = sh; job.n = lr >> (5 + log2n);
  napi_value vo = new_u8(env, lr ? lr : 1, &job.out), vs = new_u8(env, job.n ? job.n : 1, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.st, 0, job.n ? job.n : 1);
  return thr_run(env, &job, async, argv + 2, sh ? 2 : 1, vo, vs);
}
static napi_value FrNtt(napi_env env, napi_callback_info info) { return fr_ntt_call(env, info, 0); }
static napi_value FrNttAsync(napi_env env, napi_callback_info info) { return fr_ntt_call(env, info, 1); }
static napi_value kzg_cells_call(napi_env env, napi_callback_info info, int async) {
  ARGS(3); NEED_CTX(); BYTES(2, blobs, lb);
  int32_t log2n, log2c;
  if (napi_get_value_int32(env, argv[0], &log2n) != napi_ok || napi_get_value_int32(env, argv[1], &log2c) != napi_ok) { napi_throw_type_error(env, NULL, "expected numbers for log2n and log2cell"); return NULL; }
  if (log2n < 1 || log2n > 12 || log2c < 0 || log2c > log2n || !lb || lb % ((size_t)32 << log2n)) { napi_throw_range_error(env, NULL, "log2n in 1 .. 12, log2cell in 0 .. log2n, blobs of 32 << log2n bytes"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 10; job.op = log2n; job.g2 = log2c; job.b = blobs; job.n = lb >> (5 + log2n);
  napi_value vo = new_u8(env, 2 * lb, &job.out), vs = new_u8(env, job.n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.st, 0, job.n);
  return thr_run(env, &job, async, argv + 2, 1, vo, vs);
}
static napi_value KzgComputeCells(napi_env env, napi_callback_info info) { return kzg_cells_call(env, info, 0); }
static napi_value KzgComputeCellsAsync(napi_env env, napi_callback_info info) { return kzg_cells_call(env, info, 1); }
static napi_value KzgMonomialCreate(napi_env env, napi_callback_info info) {
  ARGS(2); NEED_CTX(); BYTES(1, pts, lp);
  int32_t log2n; if (napi_get_value_int32(env, argv[0], &log2n) != napi_ok) { napi_throw_type_error(env, NULL, "expected a number for log2n"); return NULL; }
  if (log2n < 1 || log2n > 12 || lp != (size_t)48 << log2n) { napi_throw_range_error(env, NULL, "log2n in 1 .. 12 and 48 << log2n bytes of compressed points"); return NULL; }
  uint8_t* st; napi_value vs = new_u8(env, (size_t)1 << log2n, &st); ALLOCATED(vs);
  handle_box* box = box_new(env, BOX_MONOMIAL); if (!box) return NULL;
  nbls_kzg_monomial* mo = NULL;
  const int rc = p_nbls_kzg_monomial_create(ctx, (unsigned)log2n, pts, (int8_t*)st, &mo);
  box->h = mo;
  return box_wrap(env, box, rc, vs);
}
static napi_value KzgMonomialDestroy(napi_env env, napi_callback_info info) { return box_destroy_call(env, info, "expected a monomial setup handle"); }
static napi_value kzg_cells_proofs_call(napi_env env, napi_callback_info info, int async) {
  ARGS(3); NEED_CTX(); BYTES(2, blobs, lb);
  handle_box* box = NULL;
  if (napi_get_value_external(env, argv[0], (void**)&box) != napi_ok || !box || !box->h) { napi_throw_type_error(env, NULL, "expected a live monomial setup handle"); return NULL; }
  unsigned log2n = 0; p_nbls_kzg_monomial_log2n((nbls_kzg_monomial*)box->h, &log2n);
  int32_t log2c; if (napi_get_value_int32(env, argv[1], &log2c) != napi_ok) { napi_throw_type_error(env, NULL, "expected a number for log2cell"); return NULL; }
  const size_t n = lb >> (5 + log2n);
  if (log2c < 0 || (unsigned)log2c > log2n || !n || lb != (n * 32) << log2n) { napi_throw_range_error(env, NULL, "log2cell in 0 .. log2n and n blobs of 32 << log2n bytes"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 11; job.mo = (nbls_kzg_monomial*)box->h; job.g2 = log2c; job.b = blobs; job.n = n; job.proofs_at = 2 * lb;
  const size_t lo = 2 * lb + n * ((size_t)2 << (log2n - log2c)) * 48;
  napi_value vo = new_u8(env, lo, &job.out), vs = new_u8(env, n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.out, 0, lo); memset(job.st, 0, n);
  return thr_run(env, &job, async, argv, 3, vo, vs);   /* the handle stays referenced while the call runs */
}
static napi_value KzgCellsAndProofs(napi_env env, napi_callback_info info) { return kzg_cells_proofs_call(env, info, 0); }
static napi_value KzgCellsAndProofsAsync(napi_env env, napi_callback_info info) { return kzg_cells_proofs_call(env, info, 1); }

static napi_value kzg_verify_cells_call(napi_env env, napi_callback_info info, int async) {
  ARGS(10); NEED_CTX(); BYTES(2, cs, lc); BYTES(3, ci, lci); BYTES(4, ki, lki); BYTES(5, cells, lb); BYTES(6, ps, lp); BYTES(7, tau, lt);
  handle_box* box = NULL;
  if (napi_get_value_external(env, argv[0], (void**)&box) != napi_ok || !box || !box->h) { napi_throw_type_error(env, NULL, "expected a live monomial setup handle"); return NULL; }
  int32_t log2c, per;
  if (napi_get_value_int32(env, argv[1], &log2c) != napi_ok || napi_get_value_int32(env, argv[9], &per) != napi_ok) { napi_throw_type_error(env, NULL, "expected numbers for log2cell and perItem"); return NULL; }
  const uint8_t* seed; if (!kzg_seed(env, argv[8], &seed)) return NULL;
  const size_t n = lp / 48, nc = lc / 48;
  if (log2c < 0 || log2c > 6 || !n || !nc || lp != n * 48 || lc != nc * 48 || lci != n * 4 || lki != n * 4 || ((uintptr_t)ci | (uintptr_t)ki) % 4 || lb != (n * 32) << log2c || lt != 96) {
    napi_throw_range_error(env, NULL, "log2cell in 0 .. 6, commitments of 48 bytes, per cell two 32-bit indices, 32 << log2cell bytes and a proof of 48 bytes, 96 bytes of [tau^c]G2"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 12; job.mo = (nbls_kzg_monomial*)box->h; job.g2 = log2c; job.a = cs; job.proofs_at = nc; job.offs = (const uint32_t*)ci; job.coffs = (const uint32_t*)ki; job.b = cells; job.proofs = ps; job.tau = tau;
  job.seed = seed; job.per_item = per != 0; job.n = n;
  napi_value vo = new_u8(env, 4, &job.out), vs = new_u8(env, n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.out, 0, 4); memset(job.st, 0, n);
  if (!seed) argv[8] = argv[7];   /* (no seed array to keep alive: a second reference to [tau^c]G2 in its place) */
  return thr_run(env, &job, async, argv, 9, vo, vs);   /* the handle and every array stay referenced while the call runs */
}
static napi_value KzgVerifyCells(napi_env env, napi_callback_info info) { return kzg_verify_cells_call(env, info, 0); }
static napi_value KzgVerifyCellsAsync(napi_env env, napi_callback_info info) { return kzg_verify_cells_call(env, info, 1); }

/* proofs == 0: (log2n, log2cell, offsets, index, cells); else (handle, log2cell, offsets, index, cells) */
static napi_value kzg_recover_call(napi_env env, napi_callback_info info, int proofs, int async) {
  ARGS(5); NEED_CTX(); BYTES(2, offs, lo); BYTES(3, idx, li); BYTES(4, cells, lb);
  handle_box* box = NULL; int32_t l2n = 0, log2c;
  if (proofs) {
    if (napi_get_value_external(env, argv[0], (void**)&box) != napi_ok || !box || !box->h) { napi_throw_type_error(env, NULL, "expected a live monomial setup handle"); return NULL; }
    unsigned v = 0; p_nbls_kzg_monomial_log2n((nbls_kzg_monomial*)box->h, &v); l2n = (int32_t)v;
  } else if (napi_get_value_int32(env, argv[0], &l2n) != napi_ok) { napi_throw_type_error(env, NULL, "expected a number for log2n"); return NULL; }
  if (napi_get_value_int32(env, argv[1], &log2c) != napi_ok) { napi_throw_type_error(env, NULL, "expected a number for log2cell"); return NULL; }
  size_t n = 0;
  int ok = l2n >= 1 && l2n <= 12 && log2c >= 0 && log2c <= l2n && !(((uintptr_t)offs | (uintptr_t)idx) % 4) && li % 4 == 0 && thr_offsets_ok(offs, lo, li / 4, &n) && n > 0 &&
           ((const uint32_t*)offs)[0] == 0 && ((const uint32_t*)offs)[n] == li / 4 && lb == (li / 4 * 32) << log2c;
  for (size_t i = 0; ok && i < n; i++) ok = ((const uint32_t*)offs)[i] <= ((const uint32_t*)offs)[i + 1];
  if (!ok) { napi_throw_range_error(env, NULL, "log2n in 1 .. 12, log2cell in 0 .. log2n, blobs + 1 non-decreasing 32-bit offsets from 0, one 32-bit index and 32 << log2cell bytes per given cell"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = proofs ? 14 : 13; job.op = l2n; job.mo = box ? (nbls_kzg_monomial*)box->h : NULL; job.g2 = log2c; job.offs = (const uint32_t*)offs; job.coffs = (const uint32_t*)idx; job.b = cells; job.n = n;
  job.proofs_at = (n * 64) << l2n;
  const size_t lout = job.proofs_at + (proofs ? n * ((size_t)2 << (l2n - log2c)) * 48 : 0);
  napi_value vo = new_u8(env, lout, &job.out), vs = new_u8(env, n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.out, 0, lout); memset(job.st, 0, n);
  return thr_run(env, &job, async, argv, 5, vo, vs);   /* the handle and every array stay referenced while the call runs */
}
static napi_value KzgRecoverCells(napi_env env, napi_callback_info info) { return kzg_recover_call(env, info, 0, 0); }
static napi_value KzgRecoverCellsAsync(napi_env env, napi_callback_info info) { return kzg_recover_call(env, info, 0, 1); }
static napi_value KzgRecoverCellsAndProofs(napi_env env, napi_callback_info info) { return kzg_recover_call(env, info, 1, 0); }
static napi_value KzgRecoverCellsAndProofsAsync(napi_env env, napi_callback_info info) { return kzg_recover_call(env, info, 1, 1); }

/* Groth16 (nbls_groth16_vk_*, nbls_groth16_verify):
 *   groth16VkCreate(alpha48, beta96, gamma96, delta96, ic48) -> a handle (the key on the device; freed by groth16VkDestroy or with the handle); a refused key throws with the
 *                                                          library's code as `nblsCode` and the m + 5 statuses (alpha, beta, gamma, delta, IC_0 ..) as `status`
 *   groth16VkDestroy(handle)                               frees it now; the handle is dead afterwards.  Not while an asynchronous call uses it
 *   groth16Verify(handle, proofs192, inputs32, seed32 | null, perItem), groth16VerifyAsync -> {out, status} as kzgVerifyProofs: out = the verdict (4 bytes, a native int),
 *                                                          status = one byte per proof */
static napi_value Groth16VkCreate(napi_env env, napi_callback_info info) {
  ARGS(5); NEED_CTX(); BYTES(0, alpha, la); BYTES(1, beta, lb); BYTES(2, gamma, lg); BYTES(3, delta, ld); BYTES(4, ic, li);
  if (la != 48 || lb != 96 || lg != 96 || ld != 96 || li % 48 || li < 96 || li / 48 - 1 > 65536) {
    napi_throw_range_error(env, NULL, "48 bytes of alpha, 96 bytes each of beta, gamma, delta, and m + 1 points IC_j of 48 bytes, 1 <= m <= 65536"); return NULL; }
  const size_t m = li / 48 - 1;
  uint8_t* st; napi_value vs = new_u8(env, m + 5, &st); ALLOCATED(vs);
  handle_box* box = box_new(env, BOX_G16_VK); if (!box) return NULL;
  nbls_groth16_vk* vk = NULL;
  const int rc = p_nbls_groth16_vk_create(ctx, m, alpha, beta, gamma, delta, ic, (int8_t*)st, &vk);
  box->h = vk;
  return box_wrap(env, box, rc, vs);
}
static napi_value Groth16VkDestroy(napi_env env, napi_callback_info info) { return box_destroy_call(env, info, "expected a Groth16 key handle"); }
static napi_value groth16_verify_call(napi_env env, napi_callback_info info, int async) {
  ARGS(5); NEED_CTX(); BYTES(1, ps, lp); BYTES(2, xs, lx);
  handle_box* box = NULL;
  if (napi_get_value_external(env, argv[0], (void**)&box) != napi_ok || !box || !box->h) { napi_throw_type_error(env, NULL, "expected a live Groth16 key handle"); return NULL; }
  int32_t per; if (napi_get_value_int32(env, argv[4], &per) != napi_ok) { napi_throw_type_error(env, NULL, "expected a number for perItem"); return NULL; }
  const uint8_t* seed; if (!kzg_seed(env, argv[3], &seed)) return NULL;
  size_t m = 0; p_nbls_groth16_vk_inputs((nbls_groth16_vk*)box->h, &m);
  const size_t n = lp / 192;
  if (!n || lp != n * 192 || lx != n * m * 32) { napi_throw_range_error(env, NULL, "n proofs of 192 bytes and n rows of m inputs of 32 bytes"); return NULL; }
  thr_job job; memset(&job, 0, sizeof job);
  job.kind = 15; job.vk = (nbls_groth16_vk*)box->h; job.proofs = ps; job.b = xs; job.seed = seed; job.per_item = per != 0; job.n = n;
  napi_value vo = new_u8(env, 4, &job.out), vs = new_u8(env, n, (uint8_t**)&job.st); ALLOCATED(vo); ALLOCATED(vs);
  memset(job.out, 0, 4); memset(job.st, 0, n);
  if (!seed) argv[3] = argv[2];   /* (no seed array to keep alive: a second reference to the inputs in its place) */
  return thr_run(env, &job, async, argv, 4, vo, vs);   /* the handle and every array stay referenced while the call runs */
}
static napi_value Groth16Verify(napi_env env, napi_callback_info info) { return groth16_verify_call(env, info, 0); }
static napi_value Groth16VerifyAsync(napi_env env, napi_callback_info info) { return groth16_verify_call(env, info, 1); }

/* The Groth16 prover (nbls_groth16_pk_*, nbls_groth16_prove), synchronous:
 *   groth16PkCreate(dims, aRows, aCols, aVals, bRows, bCols, bVals, cRows, cCols, cVals, alphaG1, betaG1, betaG2, deltaG1, deltaG2, aQuery, bG1Query, bG2Query, lQuery, hQuery)
 *       dims = Uint32Array [log2n, nVars, nPublic, nConstraints]; rows / cols: Uint32Array (CSR), vals: 32 bytes a coefficient; the points compressed -> a handle; a refused
 *       key throws with the library's code as `nblsCode` and the statuses (the descriptor's order) as `status`
 *   groth16PkDestroy(handle)
 *   groth16Prove(handle, witness32, rs64 | null) -> {out: n x 192 bytes, status: n bytes}; the arrays are the caller's to wipe */
static napi_value Groth16PkCreate(napi_env env, napi_callback_info info) {
  ARGS(20); NEED_CTX(); BYTES(0, dims, ldims);
  if (ldims != 16) { napi_throw_type_error(env, NULL, "expected a Uint32Array [log2n, nVars, nPublic, nConstraints]"); return NULL; }
  const uint32_t* dm = (const uint32_t*)dims;
  const size_t L = dm[0], nv = dm[1], m = dm[2], nc = dm[3];
  if (L < 1 || L > 21 || !m || nv <= m || nc > ((size_t)1 << L)) { napi_throw_range_error(env, NULL, "log2n in 1 .. 21, 0 < nPublic < nVars, nConstraints <= 2^log2n"); return NULL; }
  const size_t N = (size_t)1 << L, na = nv - m - 1;
  uint8_t* p[19]; size_t len[19];
  for (int i = 0; i < 19; i++) if (!get_bytes(env, argv[1 + i], &p[i], &len[i])) { napi_throw_type_error(env, NULL, "expected typed arrays"); return NULL; }
  for (int k = 0; k < 3; k++) {   /* the offsets say how long the other two arrays must be; the library checks what they hold */
    if (len[3 * k] != (nc + 1) * 4) { napi_throw_range_error(env, NULL, "a matrix needs nConstraints + 1 offsets"); return NULL; }
    const size_t nnz = ((const uint32_t*)p[3 * k])[nc];
    if (len[3 * k + 1] != nnz * 4 || len[3 * k + 2] != nnz * 32) { napi_throw_range_error(env, NULL, "a matrix needs as many columns and 32-byte coefficients as its last offset says"); return NULL; }
  }
  const size_t want[10] = {48, 48, 96, 48, 96, nv * 48, nv * 48, nv * 96, na * 48, (N - 1) * 48};
  for (int i = 0; i < 10; i++) if (len[9 + i] != want[i]) { napi_throw_range_error(env, NULL, "48 / 96 bytes a point: nVars points a per-variable query, nVars - nPublic - 1 in lQuery, 2^log2n - 1 in hQuery"); return NULL; }
  nbls_groth16_pk_desc d; memset(&d, 0, sizeof d);
  d.log2_n = (unsigned)L; d.n_vars = nv; d.n_public = m; d.n_constraints = nc;
  d.a_rows = (const uint32_t*)p[0]; d.a_cols = (const uint32_t*)p[1]; d.a_vals32 = p[2]; d.b_rows = (const uint32_t*)p[3]; d.b_cols = (const uint32_t*)p[4]; d.b_vals32 = p[5];
  d.c_rows = (const uint32_t*)p[6]; d.c_cols = (const uint32_t*)p[7]; d.c_vals32 = p[8];
  d.alpha_g1_48 = p[9]; d.beta_g1_48 = p[10]; d.beta_g2_96 = p[11]; d.delta_g1_48 = p[12]; d.delta_g2_96 = p[13];
  d.a_query48 = p[14]; d.b_g1_query48 = p[15]; d.b_g2_query96 = p[16]; d.l_query48 = p[17]; d.h_query48 = p[18];
  uint8_t* st; napi_value vs = new_u8(env, 5 + 3 * nv + na + N - 1, &st); ALLOCATED(vs);
  handle_box* box = box_new(env, BOX_G16_PK); if (!box) return NULL;
  nbls_groth16_pk* pk = NULL;
  const int rc = p_nbls_groth16_pk_create(ctx, &d, (int8_t*)st, &pk);
  box->h = pk;
  return box_wrap(env, box, rc, vs);
}
static napi_value Groth16PkDestroy(napi_env env, napi_callback_info info) { return box_destroy_call(env, info, "expected a Groth16 proving key handle"); }
static napi_value Groth16Prove(napi_env env, napi_callback_info info) {
  ARGS(3); NEED_CTX(); BYTES(1, w, lw);
  handle_box* box = NULL;
  if (napi_get_value_external(env, argv[0], (void**)&box) != napi_ok || !box || !box->h || box->kind != BOX_G16_PK) { napi_throw_type_error(env, NULL, "expected a live Groth16 proving key handle"); return NULL; }
  unsigned L = 0; size_t nv = 0, m = 0; p_nbls_groth16_pk_params((nbls_groth16_pk*)box->h, &L, &nv, &m);
  const size_t n = nv ? lw / (nv * 32) : 0;
  uint8_t* rs = NULL; size_t lrs = 0;
  napi_valuetype t; napi_typeof(env, argv[2], &t);
  if (t != napi_null && t != napi_undefined && !get_bytes(env, argv[2], &rs, &lrs)) { napi_throw_type_error(env, NULL, "expected Uint8Array or null for (r, s)"); return NULL; }
  if (!n || n > 65536 || lw != n * nv * 32 || (rs && lrs != n * 64)) { napi_throw_range_error(env, NULL, "1 .. 65536 witnesses of nVars elements of 32 bytes, and 64 bytes of (r, s) a witness or null"); return NULL; }
  uint8_t *out, *st; napi_value vo = new_u8(env, n * 192, &out), vs = new_u8(env, n, &st); ALLOCATED(vo); ALLOCATED(vs);
  const int rc = p_nbls_groth16_prove(ctx, (nbls_groth16_pk*)box->h, n, w, rs, out, (int8_t*)st);
  if (rc) { napi_throw(env, thr_error(env, rc)); return NULL; }
  napi_value res; napi_create_object(env, &res); napi_set_named_property(env, res, "out", vo); napi_set_named_property(env, res, "status", vs);
  return res;
}

static napi_value ModuleInit(napi_env env, napi_value exports) {
  const char* path = getenv("NBLS_LIB");
  char buf[4096];
  if (!path) { Dl_info di; if (dladdr((void*)ModuleInit, &di) && di.dli_fname) { snprintf(buf, sizeof buf, "%s", di.dli_fname); char* s = strrchr(buf, '/'); if (s) { *s = 0; s = strrchr(buf, '/'); if (s) { snprintf(s, sizeof buf - (s - buf), "/libnbls.so"); path = buf; } } } }
  lib = dlopen(path ? path : "libnbls.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) { napi_throw_error(env, NULL, dlerror()); return exports; }
#define LOAD(name) p_##name = (__typeof__(p_##name))dlsym(lib, #name); if (!p_##name) { napi_throw_error(env, NULL, "libnbls.so lacks " #name); return exports; }
  LOAD(nbls_init) LOAD(nbls_destroy) LOAD(nbls_strerror) LOAD(nbls_pairing_batch) LOAD(nbls_miller_product) LOAD(nbls_final_exp_batch)
  LOAD(nbls_g1_validate_batch) LOAD(nbls_g2_validate_batch) LOAD(nbls_g1_decompress_batch) LOAD(nbls_g2_decompress_batch)
  LOAD(nbls_hash_to_g2_batch) LOAD(nbls_g1_sum) LOAD(nbls_g2_sum) LOAD(nbls_verify_batch) LOAD(nbls_g1_mul_batch) LOAD(nbls_g2_mul_batch) LOAD(nbls_sign_batch) LOAD(nbls_hash_to_g1_batch) LOAD(nbls_encode_to_g1_batch) LOAD(nbls_encode_to_g2_batch) LOAD(nbls_g1_msm) LOAD(nbls_g2_msm)
  LOAD(nbls_init_multi) LOAD(nbls_destroy_multi) LOAD(nbls_multi_device_count) LOAD(nbls_multi_context) LOAD(nbls_multi_pairing_batch) LOAD(nbls_multi_miller_product) LOAD(nbls_multi_verify_batch) LOAD(nbls_g2_prepare) LOAD(nbls_pairing_prepared) LOAD(nbls_verify_multiple) LOAD(nbls_verify_aggregates) LOAD(nbls_verify_multiple_shared) LOAD(nbls_verify_aggregates_shared)
  LOAD(nbls_g1_from_hex_batch) LOAD(nbls_g2_from_hex_batch) LOAD(nbls_g2_from_signature_batch) LOAD(nbls_g1_clear_cofactor_batch) LOAD(nbls_g2_clear_cofactor_batch)
  LOAD(nbls_fr_op_batch) LOAD(nbls_lagrange_at_zero) LOAD(nbls_g2_combine_shares) LOAD(nbls_g1_combine_shares) LOAD(nbls_g1_poly_eval) LOAD(nbls_g2_poly_eval) LOAD(nbls_kzg_verify_proofs) LOAD(nbls_kzg_verify_blobs)
  LOAD(nbls_kzg_setup_create) LOAD(nbls_kzg_setup_destroy) LOAD(nbls_kzg_setup_log2n) LOAD(nbls_kzg_commit_blobs) LOAD(nbls_kzg_compute_proofs) LOAD(nbls_kzg_compute_blob_proofs)
  LOAD(nbls_fr_ntt) LOAD(nbls_kzg_compute_cells) LOAD(nbls_kzg_monomial_create) LOAD(nbls_kzg_monomial_destroy) LOAD(nbls_kzg_monomial_log2n) LOAD(nbls_kzg_compute_cells_and_proofs) LOAD(nbls_kzg_verify_cells)
  LOAD(nbls_kzg_recover_cells) LOAD(nbls_kzg_recover_cells_and_proofs)
  LOAD(nbls_groth16_vk_create) LOAD(nbls_groth16_vk_destroy) LOAD(nbls_groth16_vk_inputs) LOAD(nbls_groth16_verify)
  LOAD(nbls_groth16_pk_create) LOAD(nbls_groth16_pk_destroy) LOAD(nbls_groth16_pk_params) LOAD(nbls_groth16_prove)
  {   /* the ABI the addon was written against (include/nbls.h NBLS_ABI_VERSION): an older or newer library is refused at load instead of misread at run time */
    int (*abi)(void) = (int (*)(void))dlsym(lib, "nbls_abi_version");
    if (!abi || abi() != NBLS_ABI_VERSION) { napi_throw_error(env, NULL, "libnbls.so: ABI version differs from the one this addon was built for (include/nbls.h NBLS_ABI_VERSION)"); return exports; }
  }
  napi_property_descriptor d[] = {
    {"init", 0, Init, 0, 0, 0, napi_enumerable, 0}, {"pairingBatch", 0, PairingBatch, 0, 0, 0, napi_enumerable, 0}, {"millerProduct", 0, MillerProduct, 0, 0, 0, napi_enumerable, 0},
    {"finalExpBatch", 0, FinalExpBatch, 0, 0, 0, napi_enumerable, 0}, {"g1Decompress", 0, G1Decompress, 0, 0, 0, napi_enumerable, 0}, {"g2Decompress", 0, G2Decompress, 0, 0, 0, napi_enumerable, 0},
    {"g1Validate", 0, G1Validate, 0, 0, 0, napi_enumerable, 0}, {"g2Validate", 0, G2Validate, 0, 0, 0, napi_enumerable, 0}, {"g1Sum", 0, G1Sum, 0, 0, 0, napi_enumerable, 0},
    {"g2Sum", 0, G2Sum, 0, 0, 0, napi_enumerable, 0}, {"hashToG2", 0, HashToG2, 0, 0, 0, napi_enumerable, 0}, {"verifyBatch", 0, VerifyBatch, 0, 0, 0, napi_enumerable, 0},
    {"g1Mul", 0, G1Mul, 0, 0, 0, napi_enumerable, 0}, {"g2Mul", 0, G2Mul, 0, 0, 0, napi_enumerable, 0}, {"signBatch", 0, SignBatch, 0, 0, 0, napi_enumerable, 0},
    {"hashToCurve", 0, HashToCurve, 0, 0, 0, napi_enumerable, 0}, {"g1Msm", 0, G1Msm, 0, 0, 0, napi_enumerable, 0}, {"g2Msm", 0, G2Msm, 0, 0, 0, napi_enumerable, 0}, {"verifyBatchAsync", 0, VerifyBatchAsync, 0, 0, 0, napi_enumerable, 0}, {"verifyMultipleAsync", 0, VerifyMultipleAsync, 0, 0, 0, napi_enumerable, 0}, {"verifyAggregatesAsync", 0, VerifyAggregatesAsync, 0, 0, 0, napi_enumerable, 0},
    {"verifyMultipleSharedAsync", 0, VerifyMultipleSharedAsync, 0, 0, 0, napi_enumerable, 0}, {"verifyAggregatesSharedAsync", 0, VerifyAggregatesSharedAsync, 0, 0, 0, napi_enumerable, 0}, {"signBatchAsync", 0, SignBatchAsync, 0, 0, 0, napi_enumerable, 0},
    {"initMulti", 0, InitMulti, 0, 0, 0, napi_enumerable, 0}, {"g2Prepare", 0, G2Prepare, 0, 0, 0, napi_enumerable, 0}, {"pairingPrepared", 0, PairingPrepared, 0, 0, 0, napi_enumerable, 0},
    {"decodePoints", 0, DecodePoints, 0, 0, 0, napi_enumerable, 0}, {"clearCofactor", 0, ClearCofactor, 0, 0, 0, napi_enumerable, 0},
    {"frOp", 0, FrOp, 0, 0, 0, napi_enumerable, 0}, {"frOpAsync", 0, FrOpAsync, 0, 0, 0, napi_enumerable, 0}, {"lagrangeAtZero", 0, LagrangeAtZero, 0, 0, 0, napi_enumerable, 0},
    {"lagrangeAtZeroAsync", 0, LagrangeAtZeroAsync, 0, 0, 0, napi_enumerable, 0}, {"combineShares", 0, CombineShares, 0, 0, 0, napi_enumerable, 0},
    {"combineSharesAsync", 0, CombineSharesAsync, 0, 0, 0, napi_enumerable, 0}, {"polyEval", 0, PolyEval, 0, 0, 0, napi_enumerable, 0},
    {"polyEvalAsync", 0, PolyEvalAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgVerifyProofs", 0, KzgVerifyProofs, 0, 0, 0, napi_enumerable, 0},
    {"kzgVerifyProofsAsync", 0, KzgVerifyProofsAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgVerifyBlobs", 0, KzgVerifyBlobs, 0, 0, 0, napi_enumerable, 0},
    {"kzgVerifyBlobsAsync", 0, KzgVerifyBlobsAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgSetupCreate", 0, KzgSetupCreate, 0, 0, 0, napi_enumerable, 0},
    {"kzgSetupDestroy", 0, KzgSetupDestroy, 0, 0, 0, napi_enumerable, 0}, {"kzgProve", 0, KzgProve, 0, 0, 0, napi_enumerable, 0}, {"kzgProveAsync", 0, KzgProveAsync, 0, 0, 0, napi_enumerable, 0},
    {"frNtt", 0, FrNtt, 0, 0, 0, napi_enumerable, 0}, {"frNttAsync", 0, FrNttAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgComputeCells", 0, KzgComputeCells, 0, 0, 0, napi_enumerable, 0},
    {"kzgComputeCellsAsync", 0, KzgComputeCellsAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgMonomialCreate", 0, KzgMonomialCreate, 0, 0, 0, napi_enumerable, 0},
    {"kzgMonomialDestroy", 0, KzgMonomialDestroy, 0, 0, 0, napi_enumerable, 0}, {"kzgCellsAndProofs", 0, KzgCellsAndProofs, 0, 0, 0, napi_enumerable, 0},
    {"kzgCellsAndProofsAsync", 0, KzgCellsAndProofsAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgVerifyCells", 0, KzgVerifyCells, 0, 0, 0, napi_enumerable, 0},
    {"kzgVerifyCellsAsync", 0, KzgVerifyCellsAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgRecoverCells", 0, KzgRecoverCells, 0, 0, 0, napi_enumerable, 0},
    {"kzgRecoverCellsAsync", 0, KzgRecoverCellsAsync, 0, 0, 0, napi_enumerable, 0}, {"kzgRecoverCellsAndProofs", 0, KzgRecoverCellsAndProofs, 0, 0, 0, napi_enumerable, 0},
    {"kzgRecoverCellsAndProofsAsync", 0, KzgRecoverCellsAndProofsAsync, 0, 0, 0, napi_enumerable, 0}, {"groth16VkCreate", 0, Groth16VkCreate, 0, 0, 0, napi_enumerable, 0},
    {"groth16VkDestroy", 0, Groth16VkDestroy, 0, 0, 0, napi_enumerable, 0}, {"groth16Verify", 0, Groth16Verify, 0, 0, 0, napi_enumerable, 0},
    {"groth16VerifyAsync", 0, Groth16VerifyAsync, 0, 0, 0, napi_enumerable, 0}, {"groth16PkCreate", 0, Groth16PkCreate, 0, 0, 0, napi_enumerable, 0},
    {"groth16PkDestroy", 0, Groth16PkDestroy, 0, 0, 0, napi_enumerable, 0}, {"groth16Prove", 0, Groth16Prove, 0, 0, 0, napi_enumerable, 0}};
  napi_define_properties(env, exports, sizeof d / sizeof d[0], d);
  return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, ModuleInit)
