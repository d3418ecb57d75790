/*
 * nbls.h -- C ABI of the MI355X batched BLS12-381 pairing engine (libnbls.so).
 *
 * This is the drop-in boundary beneath the reference's exported TypeScript API (paulmillr/noble-bls12-381 v1.4.0).
 * The reference has no native/FFI layer; every entry point below replaces the part of a reference function that
 * runs between decoding its arguments and encoding its result, and names that function (file:line in the reference).
 * INTEGRATION.md shows the N-API / ctypes stubs that bind these symbols behind noble's names.
 *
 * Conventions
 *  - Wire format = the reference's own byte encodings: field elements are 48-byte big-endian (Fp.toBytes,
 *    math.ts:284-290); Fp2 = c0||c1 (math.ts:540-549); Fp12 = 576 bytes in Fp12.toBytes order (math.ts:875-884).
 *    G1 affine = x||y (96 B); G2 affine = x.c0||x.c1||y.c0||y.c1 (192 B).
 *  - All buffers are caller-owned and contiguous; the library keeps no pointer after a call returns.
 *  - Functions return 0 or a negative NBLS_E* code and never throw or abort.  Per-item `status` (may be NULL):
 *    0 ok, 1 point at infinity, 2 not on curve, 3 not in the prime-order subgroup, 4 bad encoding;
 *    +10 when the offending point is the G2 argument of a pairing.
 *  - `*_dev` variants take DEVICE pointers (HIP) and a hipStream_t (as void*); they enqueue work and do not synchronise.
 *  - A context is bound to one GPU; calls on one context are serialised internally (thread-safe per context).
 */
#ifndef NBLS_H
#define NBLS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbls_ctx nbls_ctx;

#define NBLS_OK 0
#define NBLS_EINVAL (-1)      /* bad argument */
#define NBLS_EHIP (-2)        /* HIP runtime error (nbls_last_hip_error) */
#define NBLS_ENOSUP (-3)      /* not implemented in this build */
#define NBLS_ENOGPU (-4)      /* no usable gfx950 device */
#define NBLS_EDECODE (-5)     /* an input point failed to decode where the reference throws (see per-item status) */

/* Create / destroy an engine context on HIP device `device_id` (compiles the step programs, uploads them). */
int nbls_init(int device_id, nbls_ctx** out);
void nbls_destroy(nbls_ctx* ctx);
const char* nbls_strerror(int code);
int nbls_last_hip_error(nbls_ctx* ctx);

/* pairing(P, Q, withFinalExponent) for n independent pairs -- reference index.ts:715-722.
 * validate != 0 reproduces P.assertValidity()/Q.assertValidity() (index.ts:383-388, 633-638) and the infinity
 * check (index.ts:716) as per-item status; items with a non-zero status get an all-zero output. */
int nbls_pairing_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const uint8_t* g2_aff, int with_final_exp, int validate,
                       uint8_t* out_fp12, int8_t* status);
int nbls_pairing_batch_dev(nbls_ctx* ctx, size_t n, const void* d_g1_aff, const void* d_g2_aff, int with_final_exp,
                           void* d_out_fp12, void* stream);

/* prod_i millerLoop(P_i, Q_i), optionally followed by ONE shared finalExponentiate -- the core of verify
 * (index.ts:763-766) and verifyBatch (index.ts:811-816). */
int nbls_miller_product(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const uint8_t* g2_aff, int final_exp, int validate,
                        uint8_t* out_fp12, int8_t* status);
int nbls_miller_product_dev(nbls_ctx* ctx, size_t n, const void* d_g1_aff, const void* d_g2_aff, int final_exp, void* d_out_fp12, void* stream);

/* Prepared G2 points.  PointG2.pairingPrecomputes() (index.ts:703-711) memoises calcPairingPrecomputes (math.ts:1331-1371): the 68 line
 * triples [Fp2, Fp2, Fp2] of the Miller loop, which depend on Q alone; PointG1.millerLoop (index.ts:452-454) then runs millerLoop
 * (math.ts:1373-1388) over them.  A table lives on the device in the engine's raw limb format (NBLS_LINE_TABLE_BYTES per point) or
 * crosses the ABI as the reference's value, 68 x (c0 || c1 || c2) in Fp2.toBytes order (NBLS_LINE_WIRE_BYTES per point).  Many P
 * against one Q (one message signed by many keys, index.ts:804-812) pass table_stride = 0 / n_tables = 1. */
#define NBLS_LINE_TABLE_BYTES 26112
#define NBLS_LINE_WIRE_BYTES 19584
int nbls_g2_prepare(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, uint8_t* out_tables_wire);
int nbls_g2_prepare_dev(nbls_ctx* ctx, size_t n, const void* d_g2_aff, void* d_tables, void* stream);
int nbls_lines_to_wire_dev(nbls_ctx* ctx, size_t n, const void* d_tables, void* d_tables_wire, void* stream);
int nbls_lines_from_wire_dev(nbls_ctx* ctx, size_t n, const void* d_tables_wire, void* d_tables, void* stream);
/* pairing(P_i, Q_i) / prod_i millerLoop(P_i, Q_i) with prepared Q: table_stride = NBLS_LINE_TABLE_BYTES (a table per item) or 0 (one table) */
int nbls_pairing_prepared_dev(nbls_ctx* ctx, size_t n, const void* d_g1_aff, const void* d_tables, size_t table_stride, int with_final_exp,
                              void* d_out_fp12, void* stream);
int nbls_miller_product_prepared_dev(nbls_ctx* ctx, size_t n, const void* d_g1_aff, const void* d_tables, size_t table_stride, int final_exp,
                                     void* d_out_fp12, void* stream);
/* host buffers: n_tables = n or 1 tables in wire form; product != 0 returns ONE Fp12 (the product, optionally final-exponentiated) */
int nbls_pairing_prepared(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const uint8_t* tables_wire, size_t n_tables, int with_final_exp,
                          int product, uint8_t* out_fp12);

/* Fp12.finalExponentiate for n elements -- reference math.ts:856-874. */
int nbls_final_exp_batch(nbls_ctx* ctx, size_t n, const uint8_t* in_fp12, uint8_t* out_fp12);
int nbls_final_exp_batch_dev(nbls_ctx* ctx, size_t n, const void* d_in_fp12, void* d_out_fp12, void* stream);

/* Single tower operations on the device (round 4): the reference's own unit-test surface for Fp / Fp2 / Fp6 / Fp12 (test/fp.test.ts, fp2.test.ts, fp12.test.ts) as
 * one batched entry point, so that the tower rows of the scope table have known-answer tests of their own on the GPU and not only through pairings.
 * field = 1, 2, 6, 12 (elements of 48 * field wire bytes, Fp.toBytes / Fp2.toBytes / Fp12.toBytes order); op = NBLS_TOP_*; param = the power of a Frobenius map.
 * a: n elements; b: n elements (binary operations) or n Fp2 elements (sparse products); c, d: n Fp2 elements (sparse products); unused operands NULL.
 * Replaces: Fp add / subtract / negate / multiply / square / invert (math.ts:223-273, 134-156), Fp2 ... multiplyByB / mulByNonresidue / frobeniusMap / invert
 * (math.ts:451-539), Fp6 ... multiplyBy1 / multiplyBy01 / frobeniusMap / invert (math.ts:601-688), Fp12 ... multiplyBy014 / conjugate / frobeniusMap / invert /
 * cyclotomicSquare / cyclotomicExp(x) (math.ts:732-852).  Inverting zero is undefined (the reference throws): the output element is then unspecified.
 * Returns NBLS_EINVAL for a combination the reference does not have (e.g. conjugate on Fp6). */
#define NBLS_TOP_ADD 0
#define NBLS_TOP_SUB 1
#define NBLS_TOP_NEG 2
#define NBLS_TOP_MUL 3
#define NBLS_TOP_SQR 4
#define NBLS_TOP_INV 5
#define NBLS_TOP_FROBENIUS 6        /* Fp2, Fp6, Fp12: frobeniusMap(param), 0 <= param <= 11 */
#define NBLS_TOP_CONJUGATE 7        /* Fp2 (= frobeniusMap(1)), Fp12 */
#define NBLS_TOP_MUL_BY_NONRESIDUE 8 /* Fp2: * (1 + u); Fp6: * v */
#define NBLS_TOP_MUL_BY_B 9         /* Fp2: * 4 (1 + u) */
#define NBLS_TOP_MUL_BY_1 10        /* Fp6: multiplyBy1(b) */
#define NBLS_TOP_MUL_BY_01 11       /* Fp6: multiplyBy01(b, c) */
#define NBLS_TOP_MUL_BY_014 12      /* Fp12: multiplyBy014(b, c, d) */
#define NBLS_TOP_CYCLOTOMIC_SQUARE 13 /* Fp12, unitary input */
#define NBLS_TOP_CYCLOTOMIC_EXP 14  /* Fp12, unitary input: cyclotomicExp(CURVE.x) */
int nbls_tower_op_batch(nbls_ctx* ctx, int field, int op, int param, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c, const uint8_t* d, uint8_t* out);


/* Raw device partial product for multi-GPU reductions: prod_i millerLoop(P_i,Q_i) WITHOUT final exponentiation as
 * 576 wire bytes on the device (one per rank; ranks exchange them and finish with nbls_fp12_product_final_dev). */
int nbls_fp12_product_final_dev(nbls_ctx* ctx, size_t n, const void* d_in_fp12, int final_exp, void* d_out_fp12, void* stream);

/* P.assertValidity() for affine points -- reference index.ts:383-388 (G1), 633-638 (G2): status 0 / 2 / 3. */
int nbls_g1_validate_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, int8_t* status);
int nbls_g2_validate_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, int8_t* status);

/* PointG1.fromHex for 48-byte compressed keys (index.ts:298-327) and PointG2.fromSignature for 96-byte compressed
 * signatures (index.ts:500-530): affine output + status (0 ok, 1 zero point, 3 not in subgroup, 4 no square root). */
int nbls_g1_decompress_batch(nbls_ctx* ctx, size_t n, const uint8_t* in48, uint8_t* out96, int8_t* status);
int nbls_g2_decompress_batch(nbls_ctx* ctx, size_t n, const uint8_t* in96, uint8_t* out192, int8_t* status);

/* Every wire form of the reference's point codecs, in bulk.  `len` = bytes per encoded point.
 *   nbls_g1_from_hex_batch        PointG1.fromHex (index.ts:298-327): len 48 compressed | 96 uncompressed (x || y, infinity flag 0x40)
 *   nbls_g2_from_hex_batch        PointG2.fromHex (index.ts:532-579): len 96 compressed -- flag rules, root chosen by the S bit, NO subgroup
 *                                 check, exactly as the reference -- | 192 uncompressed (x.c1 || x.c0 || y.c1 || y.c0, infinity flag 0x40)
 *   nbls_g2_from_signature_batch  PointG2.fromSignature (index.ts:500-530): len 96, or 192 (z1 and z2 read as 96-byte integers)
 * Output: canonical affine wire bytes.  status: 0 ok, 1 zero point, 2 not on curve, 3 not in the prime-order subgroup, 4 no square root,
 * 6 invalid encoding flag (first byte & 0xe0 in {0x20, 0x60, 0xe0}), 7 infinity flag with other bits set, 8 compression bit clear on 96 bytes.
 *   nbls_g*_to_hex_batch          PointG1.toHex / PointG2.toHex (index.ts:359-381, 603-631) of valid points: compressed != 0 -> 48 / 96 bytes,
 *                                 else 96 / 192 bytes (G2 in c1 || c0 order); zero (may be NULL) marks zero points.
 *   nbls_g*_clear_cofactor_batch  PointG1.clearCofactor (index.ts:401-405), PointG2.clearCofactor (index.ts:659-672) for points on the curve. */
int nbls_g1_from_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* in, size_t len, uint8_t* out96, int8_t* status);
int nbls_g2_from_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* in, size_t len, uint8_t* out192, int8_t* status);
int nbls_g2_from_signature_batch(nbls_ctx* ctx, size_t n, const uint8_t* in, size_t len, uint8_t* out192, int8_t* status);
int nbls_g1_to_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const int8_t* zero, int compressed, uint8_t* out);
int nbls_g2_to_hex_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, const int8_t* zero, int compressed, uint8_t* out);
int nbls_g1_clear_cofactor_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, uint8_t* out96, int8_t* status);
int nbls_g2_clear_cofactor_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, uint8_t* out192, int8_t* status);

/* PointG2.hashToCurve(msg, {DST}) for n messages (index.ts:481-490): msgs are concatenated, message i = msgs[offsets[i] ..
 * offsets[i+1]); SHA-256 expand_message_xmd (index.ts:207-231) and everything after it run on the GPU. */
int nbls_hash_to_g2_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out192);

/* PointG1.hashToCurve / PointG1.encodeToCurve (index.ts:331-350) and PointG2.encodeToCurve (index.ts:491-497): hash_to_field with
 * (count, m) = (2, 1) / (1, 1) / (1, 2), simplified SWU on the isogenous curve, isogeny, cofactor clearing.  Messages as above. */
int nbls_hash_to_g1_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out96);
int nbls_encode_to_g1_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out96);
int nbls_encode_to_g2_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out192);

/* The same four maps BEHIND expand_message_xmd, on n items of caller-chosen uniform bytes (for tests: the inputs where the 64-byte -> Fp reduction and the SWU maps branch are not
 * SHA-256 outputs).  kind 0 = PointG2.hashToCurve (256 bytes in, 192 out), 1 = PointG2.encodeToCurve (128 -> 192), 2 = PointG1.hashToCurve (128 -> 96), 3 = PointG1.encodeToCurve
 * (64 -> 96); each field element is 64 big-endian bytes, any value (reduced mod p).  The launches are those of the message calls for the same n.  status (may be NULL): 0 ok,
 * 1 the result is the zero point (output then all-zero).  NBLS_EINVAL before any device work for a NULL context, an unknown kind, or missing buffers with n > 0; n = 0 is NBLS_OK.
 * Items of kinds 0 and 2 whose two field elements satisfy u0 = +-u1 mod p are outside the contract (the reference doubles the SWU point with a formula that is not the
 * isogenous curve's, or maps its zero point's (0, 0) on): the device reports them as the zero point, status 1 with all-zero bytes, and every other item of the call is unaffected. */
int nbls_map_uniform_batch(nbls_ctx* ctx, int kind, size_t n, const uint8_t* uniform, uint8_t* out, int8_t* status);

/* Sum of n affine points: the reduce step of aggregatePublicKeys / aggregateSignatures (index.ts:771-788). *status = 1 when
 * the sum is the zero point (output then all-zero). */
int nbls_g1_sum(nbls_ctx* ctx, size_t n, const uint8_t* pts96, uint8_t* out96, int8_t* status);
int nbls_g2_sum(nbls_ctx* ctx, size_t n, const uint8_t* pts192, uint8_t* out192, int8_t* status);

/* PointG1.toHex(true) / toRawBytes(true) (index.ts:355-371) and PointG2.toSignature (index.ts:586-602) for n NON-ZERO affine points:
 * x with the compression flag (bit 383) and the sign flag (bit 381) = floor(2y / p).  The zero point (not representable as
 * affine wire bytes; the sum / multiplication calls report it as status 1) encodes as 0xc0 00...00 on the caller's side. */
int nbls_g1_compress_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, uint8_t* out48);
int nbls_g2_compress_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff, uint8_t* out96);

/* [k_i]P_i for per-item scalars (32 bytes big-endian each; any value, the reference reduces mod r first: normalizePrivKey
 * index.ts:269-279).  g1_aff == NULL multiplies the G1 generator: the core of getPublicKey / PointG1.fromPrivateKey
 * (index.ts:350-353, 738-740).  Fixed-window ladder with masked table selection: instruction stream and memory access pattern do
 * not depend on the scalar.  status: 0 ok, 1 result is the zero point, 5 scalar is 0 mod r (the reference throws). */
int nbls_g1_mul_batch(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff /* n*96 or NULL */, const uint8_t* scalars32, uint8_t* out96, int8_t* status);
int nbls_g2_mul_batch(nbls_ctx* ctx, size_t n, const uint8_t* g2_aff /* n*192 */, const uint8_t* scalars32, uint8_t* out192, int8_t* status);

/* Multi-scalar multiplication sum_i [k_i]P_i (weighted form of the reference's aggregatePublicKeys / aggregateSignatures,
 * index.ts:771-788, whose unweighted sums are nbls_g1_sum / nbls_g2_sum; the building block of random-linear-combination batch
 * verification of distinct signatures).  Points: affine wire bytes in the prime-order subgroup (nbls_g*_validate_batch); scalars:
 * 32 bytes big-endian each, any value.  Bucket method (12-bit windows) on the device; NOT constant time in the scalars (public
 * coefficients), use nbls_g*_mul_batch for secret ones.  out: one affine point; status: 0 ok, 1 the sum is the zero point (output
 * then all-zero). */
int nbls_g1_msm(nbls_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out96, int8_t* status);
int nbls_g2_msm(nbls_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out192, int8_t* status);
/* the same with points, scalars, result and status resident in device memory; all scalars < 2^nbits (0 = 256) */
int nbls_msm_dev(nbls_ctx* ctx, int g2, size_t n, const void* d_pts, const void* d_scalars32, unsigned nbits, void* d_out, void* d_status, void* stream);
/* Many independent sums in one call (no reference counterpart): weighted aggregates, Feldman / DKG batch checks, commitments of many polynomials to one basis.
 *   _batch   out[g] = sum over i in [group_offsets[g], group_offsets[g + 1]) of [k_i]P_i: n_groups + 1 offsets into the point and the scalar array, NON-DECREASING -- an empty
 *            group is a legitimate empty sum (status 1, as nbls_g*_msm with n = 0); the first offset need not be 0, the entries in front of it are not read.
 *   _rows    n_rows scalar vectors against ONE set of n_pts points: out[r] = sum_j [k[r * n_pts + j]]P_j; the points are converted and split once, not n_rows times (unless n_pts is above
 *            NBLS_TUNE_MSMB_BIG: every row is then a big group and runs through the pipeline of nbls_g*_msm, which converts the points again for each row).
 * Points and scalars exactly as nbls_g*_msm takes them: affine wire bytes in the prime-order subgroup, NOT validated; 32 bytes big-endian, any value.  NOT constant time and not
 * an interface for secrets (nothing is wiped; window width and scalar split depend on the scalars).  out[g]: affine wire bytes; status[g] (may be NULL): 0, or 1 when the sum is
 * the zero point (output all-zero).  Every group's output and status are byte for byte what nbls_g*_msm returns for that group alone.
 * One copy in, one chain on the context's stream, one copy out: conversion and GLV / GLS split of all points and scalars once, then the groups in slabs of whole groups
 * (NBLS_TUNE_MSMB_SLAB bounds the scratch of a slab) through the bucket method with (group, window, digit) keys and a window width chosen per call from {4, 6, 8, 10, 12} by the
 * mean group size (NBLS_TUNE_MSMB_WINDOW forces it); one doubling-and-add chain over the bit positions combines all groups of a slab at once.  A slab whose largest group has
 * more than 8 points after the split reads its longest run back (4 bytes), as nbls_g*_msm does; a group of more than NBLS_TUNE_MSMB_BIG points, and a call of one group, run
 * through the pipeline of nbls_g*_msm on the same stream.
 * Returns NBLS_OK whatever the groups hold; NBLS_EINVAL before any device work for a missing pointer (points and scalars may be NULL only when the call holds none),
 * n_groups = 0 or n_rows = 0, n_pts = 0 (an empty point set is refused: use _batch with empty groups), decreasing offsets, more than 2^22 points or scalars in the call, more
 * than 2^20 groups or rows. */
int nbls_g1_msm_batch(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets /* n_groups + 1 */, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out96 /* n_groups */,
                      int8_t* status /* n_groups, may be NULL */);
int nbls_g2_msm_batch(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets /* n_groups + 1 */, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out192 /* n_groups */,
                      int8_t* status /* n_groups, may be NULL */);
int nbls_g1_msm_rows(nbls_ctx* ctx, size_t n_pts, const uint8_t* pts96, size_t n_rows, const uint8_t* scalars32 /* n_rows * n_pts */, uint8_t* out96 /* n_rows */,
                     int8_t* status /* n_rows, may be NULL */);
int nbls_g2_msm_rows(nbls_ctx* ctx, size_t n_pts, const uint8_t* pts192, size_t n_rows, const uint8_t* scalars32 /* n_rows * n_pts */, uint8_t* out192 /* n_rows */,
                     int8_t* status /* n_rows, may be NULL */);

/* sign(message_i, privateKey_i) -- reference index.ts:744-752: PointG2.hashToCurve(message) multiplied by the key; output is
 * the affine signature point (192 B), which PointG2.toSignature (index.ts:586-602) compresses on the caller's side.
 * Messages as in nbls_hash_to_g2_batch. */
int nbls_sign_batch(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len,
                    const uint8_t* keys32, uint8_t* out192, int8_t* status);
/* Same with everything resident in device memory (round 5): message bytes, n + 1 uint32 offsets into them, 32-byte big-endian keys -> n affine points (192 B) and n status
 * bytes in device memory; SHA-256 expand_message_xmd, hash-to-G2 and the ladder run as one chain on `stream` (NULL = the context's).  status: 0 ok, 1 the result is the zero
 * point, i.e. the key is 0 mod r (the host-buffer call reports 5 there, as normalizePrivKey's message demands; keys >= r are reduced, index.ts:269-279).  Synchronises;
 * NBLS_EINVAL if the offsets decrease somewhere. */
int nbls_sign_batch_dev(nbls_ctx* ctx, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                        const void* d_keys32, void* d_out192, void* d_status, void* stream);

/* verifyBatch(signature, messages, publicKeys) on wire inputs -- reference index.ts:792-821 with every message distinct.
 * *ok = 1/0; returns NBLS_EDECODE where the reference throws while decoding its arguments. */
int nbls_verify_batch(nbls_ctx* ctx, size_t n, const uint8_t* sig96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pk48,
                      const uint8_t* dst, size_t dst_len, int* ok);
/* Same, inputs already in HBM: signature, 256-byte expand_message_xmd outputs, compressed keys.  Synchronises (returns *ok). */
/* Same with the MESSAGES resident in HBM (bytes + n + 1 uint32 offsets relative to d_msgs): expand_message_xmd runs on the device first, on the same stream
 * (the whole of verifyBatch index.ts:792-821 for wire-format inputs with nothing done on the host).  dst_len <= 255. */
int nbls_verify_batch_msgs_dev(nbls_ctx* ctx, size_t n, const void* d_sig96, const void* d_msgs, const void* d_offsets, const void* d_pk48, const uint8_t* dst, size_t dst_len,
                               int* ok, void* stream);
/* d_uniform256: an item whose two field elements satisfy u0 = +-u1 mod p is outside the contract (see nbls_map_uniform_batch): the hash stage yields the zero point for it, handed to
 * the Miller loop as all-zero affine bytes WITHOUT a status of its own, so the call's verdict is unspecified; the hash points of the other items are unaffected. */
int nbls_verify_batch_dev_inputs(nbls_ctx* ctx, size_t n, const void* d_sig96, const void* d_uniform256, const void* d_pk48, int* ok,
                                 int8_t* pk_status /* n, may be NULL */, void* stream);

/* verify(signature_i, message_i, publicKey_i) (index.ts:756-767) for n independent sets, checked together by a random linear combination (no reference counterpart; the
 * MSM's follow-on).  With secret weights r_i = BE64(SHA-256(seed32 || BE64(i))[0..8]) | 2^63 every set is accepted when
 *   prod_i e([r_i]pk_i, H(m_i)) * e(-G1, sum_i [r_i]sig_i) = 1
 * -- n + 1 Miller loops and ONE final exponentiation where n verify calls spend 2n and n.  If some set is invalid the check passes with probability at most 2^-63 over the
 * weights.  A seed an attacker can predict voids that guarantee: pass NULL (32 bytes from getrandom(2) on every call; NBLS_ENOSUP when the OS gives none -- never a fixed seed)
 * unless a reproducible test needs its own.  Messages, offsets and the DST as nbls_verify_batch (a DST over 255 bytes is hashed with H2C-OVERSIZE-DST-; NBLS_EINVAL when the
 * offsets decrease, for n = 0, n > 2^22 or a missing pointer); sigs96 = n compressed signatures, pks48 = n compressed keys.
 * status[i] (may be NULL) = what the reference's verify(sig_i, m_i, pk_i) does, in its order (key, message, signature, pairing): the key decoder's status if >= 2 (3 outside the
 * subgroup, 4 no square root), else 10 + the signature decoder's status if >= 2, else 1 for a zero key and 11 for a zero signature (the reference throws "No pairings at point of
 * Infinity"), else 0 when the set verifies and NBLS_ST_NOT_VERIFIED when it does not.  *all_ok = 1 exactly when every set has status 0.  Where the combined check does not accept
 * (a set failed to decode, the product is not one, the weighted sum of the signatures is zero) a per-set pass judges every set on its own; with status == NULL the call stops
 * after the combined check instead and answers *all_ok = 0 (fast reject).  Returns NBLS_OK whatever the sets hold. */
#define NBLS_ST_NOT_VERIFIED 9
int nbls_verify_multiple(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pks48, const uint8_t* dst, size_t dst_len,
                         const uint8_t* seed32 /* NULL: from the OS */, int* all_ok, int8_t* status /* n, may be NULL */);

/* verify(sig_j, m_j, aggregatePublicKeys(keys_j)) (index.ts:756-778) for n sets, checked together by one random linear combination over the SETS (weights r_j as in
 * nbls_verify_multiple): prod_j e([r_j]apk_j, H(m_j)) * e(-G1, sum_j [r_j]sig_j) = 1 with apk_j the sum of set j's keys.  Set j: sigs96[j], message msgs[offsets[j] .. offsets[j+1]),
 * keys pks48[key_offsets[j] .. key_offsets[j+1]) (48-byte compressed, in 48-byte units).  status[j], in the reference's order: the decoder status of the set's first key that does
 * not decode (3 outside the subgroup, 4 no square root: aggregatePublicKeys throws there), else 10 + the signature decoder's status if >= 2, else 1 when the keys sum to the zero
 * point ({pk, -pk}, only 0xc0... keys: "No pairings at point of Infinity"), else 11 for a zero signature, else 0 or NBLS_ST_NOT_VERIFIED.  A zero key inside a set is valid and adds
 * nothing.  Seed, per-set pass, fast reject (status == NULL), *all_ok and return codes as nbls_verify_multiple; NBLS_EINVAL also for a set without keys (the reference throws
 * "Expected non-empty array"), decreasing key offsets and more than 2^24 keys in one call. */
int nbls_verify_aggregates(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pks48, const uint32_t* key_offsets,
                           const uint8_t* dst, size_t dst_len, const uint8_t* seed32 /* NULL: from the OS */, int* all_ok, int8_t* status /* n, may be NULL */);
/* A table of keys decoded once (PointG1.fromHex, index.ts:298-327) and kept in device memory of ctx's device: nbls_verify_aggregates_indexed names keys by their index in it, so that
 * no key is decoded or subgroup-checked again.  status[i] (may be NULL) = the decoder's status of key i (0, 1 for the zero key, 3, 4); a key that did not decode stays in the table and
 * fails every set that names it with that status.  At most 2^24 keys.  The table belongs to no context: any context on the same device may use it, after its creator is destroyed
 * too; nbls_keyset_destroy must not run while a call uses it. */
typedef struct nbls_keyset nbls_keyset;
int  nbls_keyset_create(nbls_ctx* ctx, size_t n, const uint8_t* pks48, int8_t* status /* n, may be NULL */, nbls_keyset** out);
void nbls_keyset_destroy(nbls_keyset* ks);
int  nbls_keyset_size(const nbls_keyset* ks, size_t* n);
/* The same as nbls_verify_aggregates, with the keys of set j = table entries key_index[key_offsets[j] .. key_offsets[j+1]); NBLS_EINVAL also for an index >= the table's size and
 * for a table created on another device than ctx's. */
int nbls_verify_aggregates_indexed(nbls_ctx* ctx, const nbls_keyset* ks, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* key_index,
                                   const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status);

/* The three calls above for sets that SHARE messages: msgs / offsets hold n_msgs distinct messages (offsets has n_msgs + 1 entries) and set i signs message msg_index[i].  The
 * factors of one message are multiplied together by bilinearity,
 *   prod_{g < n_msgs} e(sum_{i : msg_index[i] = g} [r_i]pk_i, H(m_g)) * e(-G1, sum_i [r_i]sig_i) = 1,
 * n_msgs hashes to G2 and n_msgs + 1 Miller loops instead of n and n + 1, exactly as sound: the weights r_i stay per SET (by set index i, as in nbls_verify_multiple), so two
 * signers of one message whose signatures are exchanged are still caught.  status[i] and *all_ok are byte for byte what the twin without `_shared` returns for the expanded input
 * (set i given the bytes of message msg_index[i]) and the same seed.  Messages may repeat inside msgs; msg_index may be any map onto 0 .. n_msgs - 1, the identity included, and the
 * sets of one message need not be contiguous.  When the weighted keys of one message sum to the zero point the combined check cannot count (like a zero weighted sum of the
 * signatures): the per-set pass judges the sets, and with status == NULL the call answers *all_ok = 0.  Seed, DST rule, fast reject and return codes as the twins; NBLS_EINVAL also
 * for n_msgs = 0, n_msgs > n, a missing msg_index, an index >= n_msgs and a message that no set names -- refused before any device work. */
int nbls_verify_multiple_shared(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* msg_index /* n */,
                                const uint8_t* pks48, const uint8_t* dst, size_t dst_len, const uint8_t* seed32 /* NULL: from the OS */, int* all_ok, int8_t* status /* n, may be NULL */);
int nbls_verify_aggregates_shared(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* msg_index /* n */,
                                  const uint8_t* pks48, const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status);
int nbls_verify_aggregates_indexed_shared(nbls_ctx* ctx, const nbls_keyset* ks, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets,
                                          const uint32_t* msg_index /* n */, const uint32_t* key_index, const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len,
                                          const uint8_t* seed32, int* all_ok, int8_t* status);

/* The scalar field Fr = Z / r (math.ts:295-386) on the device, n elements per call: add / subtract / negate / multiply / square / invert / div / pow (math.ts:317-349).
 * Elements are 32 bytes big-endian, ANY 256-bit value (reduced mod r first, as `new Fr(v)` does, math.ts:301-303); outputs are canonical (< r).  b32: the second operand, or
 * POW's exponent (read as a 256-bit integer, not reduced); NULL for the unary operations.  status (may be NULL): 5 where INV / DIV meets 0 mod r (the reference throws), the
 * output element is then all-zero.  Control flow on the device does not depend on the operands (INV is the fixed chain x^(r - 2)), but the Fr calls are NOT an interface for
 * secrets: nothing is wiped from staging or scratch memory.  Shamir-splitting of keys stays on the caller's side. */
#define NBLS_FROP_ADD 0
#define NBLS_FROP_SUB 1
#define NBLS_FROP_NEG 2
#define NBLS_FROP_MUL 3
#define NBLS_FROP_SQR 4
#define NBLS_FROP_INV 5
#define NBLS_FROP_DIV 6
#define NBLS_FROP_POW 7
int nbls_fr_op_batch(nbls_ctx* ctx, int op, size_t n, const uint8_t* a32, const uint8_t* b32, uint8_t* out32, int8_t* status);

/* Threshold signatures: Lagrange coefficients at zero and the recombination of t-of-n shares (no reference counterpart; the reference's README names the use).  The shares come
 * in n_groups contiguous groups: group g = entries group_offsets[g] .. group_offsets[g + 1] of ids32 and of the share array (n_groups + 1 offsets, strictly increasing: no
 * empty group; the first need not be 0, the entries in front of it are not read), ids32 = one 32-byte big-endian identifier x_k per share (any value, reduced mod r).
 *   nbls_lagrange_at_zero   out32[k] = lambda_k = prod_{j != k} x_j / (x_j - x_k) over the share's group, canonical.  status[g] (may be NULL): 0, or NBLS_ST_BAD_IDS when an
 *                           identifier of the group is 0 mod r or two of them are equal mod r (that group's coefficients are then all-zero).
 *   nbls_g2_combine_shares  out96[g] = compress(sum_k [lambda_k] share_k) for shares that are 96-byte compressed G2 points decoded by PointG2.fromSignature's rules
 *                           (index.ts:500-530): signature shares.  nbls_g1_combine_shares: 48-byte compressed G1 points, PointG1.fromHex's rules (index.ts:298-327): the shares
 *                           of a group public key.  status[g] (may be NULL), in this order: NBLS_ST_BAD_IDS; else what nbls_g*_decompress_batch reports for the group's first
 *                           share that does not decode (>= 2: 3 outside the subgroup, 4 no square root); else 1 when the combination is the zero point (output 0xc0 00..); else 0.
 *                           A zero share (0xc0 00..) is valid and adds nothing.  A group with a status other than 0 / 1 gets all-zero output and never disturbs its neighbours.
 * One chain on the context's stream: one copy in, the decoder, the coefficients, the ladders (the coefficients are public: the G2 ladder is the psi-split one), one sum per group,
 * compression, one copy out.  Returns NBLS_OK whatever the groups hold; NBLS_EINVAL before any device work for a missing pointer, n_groups = 0, offsets that do not strictly
 * increase, more than 2^24 shares in the call and a group of more than 2^16 shares.  Not an interface for secrets (see nbls_fr_op_batch). */
#define NBLS_ST_BAD_IDS 20
int nbls_lagrange_at_zero(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* ids32, uint8_t* out32, int8_t* status /* n_groups, may be NULL */);
int nbls_g2_combine_shares(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* ids32, const uint8_t* shares96, uint8_t* out96, int8_t* status);
int nbls_g1_combine_shares(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* ids32, const uint8_t* shares48, uint8_t* out48, int8_t* status);

/* Share public keys: the commitment polynomial of a DKG / Feldman VSS evaluated in the exponent (no reference counterpart).  F(x) = sum_j [x^j] A_j with the committed
 * coefficients A_j = [a_j]G, A_0 the group key; pk_k = F(x_k) is the public key of share k, and [s]G == F(x_me) is the check a participant runs on a share it receives.
 * n_groups polynomials per call: group g owns the coefficients coef_offsets[g] .. coef_offsets[g + 1] of the coefficient array, LOWEST degree first, and the identifiers
 * id_offsets[g] .. id_offsets[g + 1] of ids32 (n_groups + 1 offsets each, strictly increasing: no empty group; the first need not be 0, the entries in front of it are not read).
 *   coefficients  compressed points decoded as nbls_g*_combine_shares decodes its shares: 48 bytes by PointG1.fromHex's rules, 96 bytes by PointG2.fromSignature's, subgroup
 *                 check included.  A zero coefficient (0xc0 00..) is valid and adds nothing.
 *   identifiers   32 bytes big-endian, ANY value, zero included: F(0) = A_0 is a legitimate question (refusing zero identifiers is nbls_lagrange_at_zero's job); x and x + r
 *                 give the same bytes.
 *   out[k]        compress(F_g(x_k)), one per identifier.  status[k] (may be NULL), in this order: what nbls_g*_decompress_batch reports for the group's FIRST coefficient that
 *                 does not decode (>= 2: 3 outside the subgroup, 4 no square root), for every identifier of that group, with all-zero output; else 1 when F(x_k) is the zero
 *                 point (output 0xc0 00..); else 0.  A bad group never disturbs its neighbours.
 * One chain on the context's stream: one copy in, the decoder, Horner's rule in the exponent (acc <- [x]acc + A_j from the highest coefficient down: one step program per
 * coefficient; a call whose identifiers are all below 2^16 as given runs the 16-bit form of the step), to-affine, compression, one copy out; the identifiers are worked through
 * in slabs (NBLS_TUNE_POLY_SLAB) so that scratch stays bounded.  Returns NBLS_OK whatever the groups hold; NBLS_EINVAL before any device work for a missing pointer, n_groups = 0,
 * offsets that do not strictly increase, more than 2^16 coefficients in one group, more than 2^24 coefficients or more than 2^22 identifiers in the call.  Coefficients and
 * identifiers are public values: like the Fr calls this is NOT an interface for secrets (nothing is wiped, the short form's choice depends on the identifiers). */
int nbls_g1_poly_eval(nbls_ctx* ctx, size_t n_groups, const uint32_t* coef_offsets /* n_groups + 1 */, const uint8_t* coefs48, const uint32_t* id_offsets /* n_groups + 1 */,
                      const uint8_t* ids32, uint8_t* out48 /* one per identifier */, int8_t* status /* one per identifier, may be NULL */);
int nbls_g2_poly_eval(nbls_ctx* ctx, size_t n_groups, const uint32_t* coef_offsets /* n_groups + 1 */, const uint8_t* coefs96, const uint32_t* id_offsets /* n_groups + 1 */,
                      const uint8_t* ids32, uint8_t* out96 /* one per identifier */, int8_t* status /* one per identifier, may be NULL */);

/* KZG on BLS12-381 (EIP-4844; no reference counterpart): the verifier's side of blob commitments here, the prover's side (commitments, proofs, the
 * quotient) below under "KZG, the prover's side".  Field elements are 32 bytes big-endian and must be CANONICAL (bytes_to_bls_field: a value >= r is refused, status NBLS_ST_NON_CANONICAL) --
 * unlike nbls_fr_op_batch, which reduces.  The formulas are EIP-4844's as the project's issue states them; the specification's own test vectors have not been run.
 *
 * nbls_fr_eval_roots: evaluate_polynomial_in_evaluation_form for n polynomials, each at its own point.  With N = 2^log2_n, polynomial i is given by its N values
 * evals32[i N .. i N + N) on the roots of unity in bit-reversed order, w_j = omega^rev(j), omega = 7^((r - 1) / N), rev = the reversal of the log2_n bits of j:
 *   out32[i] = p_i(z_i) = (z^N - 1) / N * sum_j f_j w_j / (z - w_j),   and f_j itself where z = w_j.
 * status[i] (may be NULL): 0, or NBLS_ST_NON_CANONICAL when an element of the polynomial or z_i is >= r (out32[i] is then all-zero; the neighbours are not disturbed).
 * One copy in, one kernel (a workgroup per polynomial, one field inversion per lane), one copy out; the table of roots is built on the device on the first use of a log2_n and
 * kept with the context.  NBLS_EINVAL before any device work for log2_n outside 1 .. 12, a NULL context, missing buffers with n > 0, more than 2^24 elements in the call; n = 0 is
 * NBLS_OK.  Not an interface for secrets (see nbls_fr_op_batch). */
#define NBLS_ST_NON_CANONICAL 21   /* a 32-byte field element is >= r */
int nbls_fr_eval_roots(nbls_ctx* ctx, unsigned log2_n /* 1 .. 12 */, size_t n, const uint8_t* evals32 /* n << log2_n elements */, const uint8_t* z32 /* n */,
                       uint8_t* out32 /* n */, int8_t* status /* n, may be NULL */);
/* verify_kzg_proof_batch: n tuples (commitment C_i, point z_i, value y_i, proof pi_i) against the setup's [tau]G2 (96 bytes compressed, PointG2.fromSignature's rules), checked
 * together by a random linear combination with the weights r_i of nbls_verify_multiple (same seed rule: NULL = 32 bytes from getrandom(2) on every call):
 *   e(-sum_i [r_i]pi_i, [tau]G2) * e(sum_i [r_i]C_i + sum_i [r_i z_i]pi_i - [sum_i r_i y_i]G1, G2) = 1
 * -- MSMs of n points each, two Miller loops against prepared tables and ONE final exponentiation.  Commitments and proofs are 48 bytes compressed, decoded by PointG1.fromHex's rules, subgroup
 * check included.  ZERO POINTS ARE VALID: 0xc0 00.. is the commitment of the zero polynomial and the proof of a constant one; a zero point takes part as the identity and status 1
 * is never reported; either or both combined points may be the zero point (every polynomial of the call constant), which counts as a factor of one.
 * status[i] (may be NULL), in this order: the commitment decoder's status if >= 2 (3 outside the subgroup, 4 no square root); else 10 + the proof decoder's status if >= 2; else
 * NBLS_ST_NON_CANONICAL when z_i or y_i is >= r; else 0, or NBLS_ST_NOT_VERIFIED.  *all_ok = 1 exactly when every status is 0.  Items with one of the first three statuses take
 * part in the combined sums with weight zero, and the combined check never accepts while there is one.  Where it does not accept, a per-item pass judges every tuple,
 *   e(-pi_i, [tau]G2) * e(C_i + [z_i]pi_i - [y_i]G1, G2) = 1,
 * with the two prepared tables shared by all items and one batched final exponentiation; with status == NULL the call stops after the combined check instead and answers
 * *all_ok = 0 (fast reject).  Returns NBLS_OK whatever the tuples hold; NBLS_EDECODE when tau_g2_96 does not decode or is the zero point; NBLS_EINVAL for n = 0, n > 2^22 or a
 * missing pointer.  *all_ok and status are NOT written when the call returns an error, NBLS_EDECODE included (the chain has then run on the undecoded [tau]G2 and is discarded). */
int nbls_kzg_verify_proofs(nbls_ctx* ctx, size_t n, const uint8_t* commitments48, const uint8_t* z32, const uint8_t* y32, const uint8_t* proofs48, const uint8_t* tau_g2_96,
                           const uint8_t* seed32 /* NULL: from the OS */, int* all_ok, int8_t* status /* n, may be NULL */);
/* verify_blob_kzg_proof_batch: blob i = the 2^log2_n values of polynomial i (log2_n = 12: the mainnet blob of 131,072 bytes; smaller sizes exist for tests),
 *   z_i = BE(SHA-256("FSBLOBVERIFY_V1_" || BE128(N) || blob_i || commitment_i)) mod r   (on host threads, behind the copy of the blobs: 2 N + 2 dependent SHA-256 blocks per blob are no work for a GPU lane),
 *   y_i = p_i(z_i)   (on the device, as nbls_fr_eval_roots; the blobs cross the bus once),
 * then the chain, statuses and return codes of nbls_kzg_verify_proofs; a blob with an element >= r gets NBLS_ST_NON_CANONICAL.  NBLS_EINVAL also for log2_n outside 1 .. 12 and
 * more than 2^24 blob elements in the call. */
int nbls_kzg_verify_blobs(nbls_ctx* ctx, unsigned log2_n, size_t n, const uint8_t* blobs /* n * (32 << log2_n) */, const uint8_t* commitments48, const uint8_t* proofs48,
                          const uint8_t* tau_g2_96, const uint8_t* seed32, int* all_ok, int8_t* status);

/* KZG, the prover's side (EIP-4844: blob_to_kzg_commitment, compute_kzg_proof, compute_blob_kzg_proof).  Blobs are public and the MSM is not constant time: NOT an interface
 * for secrets.
 *
 * nbls_kzg_setup: the setup's g1_lagrange in device memory, decoded ONCE.  lagrange48 holds 2^log2_n compressed G1 points in BIT-REVERSED ORDER: entry j is [L_j(tau)]G1 for the
 * root w_j = omega^rev(j) -- the order of nbls_fr_eval_roots and of the blob elements.  Entries are decoded by PointG1.fromHex's rules, subgroup check included; status[j] (may be
 * NULL) is the decoder's status.  An entry with a status >= 2, or a zero point (status 1: no real setup contains one), makes the call return NBLS_EDECODE with *out = NULL; the
 * statuses are written in both cases.  The points are kept as the batched MSM reads them after its conversion (each point and its endomorphism image, raw projective: about
 * 1.5 MB at 4096 points), so decoding, subgroup check and split are never repeated per call.  The object belongs to no context: any context on the same device may use it, also
 * after the creating context is destroyed; nbls_kzg_setup_destroy must not run while a call uses it.  NBLS_EINVAL for log2_n outside 1 .. 12 or a missing pointer.  Parsing
 * the ceremony's file formats stays with the caller. */
typedef struct nbls_kzg_setup nbls_kzg_setup;
int  nbls_kzg_setup_create(nbls_ctx* ctx, unsigned log2_n, const uint8_t* lagrange48 /* 2^log2_n compressed G1 points */, int8_t* status /* 2^log2_n, may be NULL */,
                           nbls_kzg_setup** out);
void nbls_kzg_setup_destroy(nbls_kzg_setup* s);
int  nbls_kzg_setup_log2n(const nbls_kzg_setup* s, unsigned* log2_n);
/* The quotient of an opening in evaluation form, for n polynomials each at its own point (layout, order of the roots and limits as nbls_fr_eval_roots):
 *   out_y32[i] = y = p_i(z_i), exactly what nbls_fr_eval_roots returns;   out_q32[i N + j] = q_j = (f_j - y) / (w_j - z)  for every j with w_j != z;
 *   where z = w_m: q_m = sum_{j != m} (f_j - y) w_j / (z (z - w_j))   (compute_quotient_eval_within_domain; computed as -1 / z * sum_{j != m} q_j w_j).
 * Elements must be canonical: an element of the polynomial >= r, or z_i >= r, gives status[i] = NBLS_ST_NON_CANONICAL, y and the whole quotient row are then all-zero and the
 * neighbouring polynomials are not disturbed.  One copy in, one kernel (a workgroup per polynomial: the batch inversion of the evaluation keeps its inverses), one copy out.
 * NBLS_EINVAL before any device work for log2_n outside 1 .. 12, a NULL context, missing buffers with n > 0, more than 2^24 elements in the call; n = 0 is NBLS_OK. */
int nbls_fr_quotient_roots(nbls_ctx* ctx, unsigned log2_n /* 1 .. 12 */, size_t n, const uint8_t* evals32 /* n << log2_n */, const uint8_t* z32 /* n */, uint8_t* out_y32 /* n */,
                           uint8_t* out_q32 /* n << log2_n */, int8_t* status /* n, may be NULL */);
/* The three prover calls.  Blob i = the 2^log2_n values of polynomial i as in nbls_kzg_verify_blobs; the size comes from the setup.
 *   nbls_kzg_commit_blobs        blob_to_kzg_commitment:  C_i = sum_j [f_ij] L_j, 48 bytes compressed
 *   nbls_kzg_compute_proofs      compute_kzg_proof:       y_i = p_i(z_i), pi_i = sum_j [q_ij] L_j with the quotient of nbls_fr_quotient_roots
 *   nbls_kzg_compute_blob_proofs compute_blob_kzg_proof:  z_i = the FSBLOBVERIFY_V1_ challenge of (blob_i, commitment_i), hashed on up to eight host threads behind the copy of the
 *                                blobs, then as compute_proofs (y_i is not returned).  GIVEN COMMITMENTS ARE ONLY HASHED, NOT DECODED: bytes that are no commitment of the blob
 *                                yield a proof that will not verify.  With commitments48 == NULL the call commits first, on the blobs already on the device, and reads the 48 n
 *                                bytes back (the one synchronisation the challenge needs); they are returned in out_commitments48, which is then required (else it may be NULL).
 * Each call is one chain on the context's stream: one copy in, the canonical check of the blob elements (inside the quotient kernel; a small kernel of its own for commitments),
 * the quotient rows written as 32-byte big-endian scalars straight into the MSM's scalar array, the batched MSM in its rows form (as nbls_g1_msm_rows, split along the
 * endomorphism, window width by its cost model, slabs by NBLS_TUNE_MSMB_SLAB) against the setup's converted points, to-affine, compression, one copy out.
 * status[i] (may be NULL): 0, or NBLS_ST_NON_CANONICAL for a blob element or z_i >= r; that item's outputs are then ALL-ZERO bytes (48 zero bytes are deliberately no valid
 * encoding; a zero y).  ZERO POINTS ARE VALID as in the verifier: the zero polynomial commits to 0xc0 00.., a constant polynomial's proof is 0xc0 00.., both with status 0.
 * Returns NBLS_OK whatever the blobs hold; NBLS_EINVAL before any device work for a missing pointer, n = 0, a setup created on another device, or n << log2_n above 2^22 (the
 * batched MSM's bound on scalars per call: 1024 mainnet blobs fit exactly) or n above 2^20 (its bound on rows: reached only at log2_n = 1). */
int nbls_kzg_commit_blobs(nbls_ctx* ctx, const nbls_kzg_setup* setup, size_t n, const uint8_t* blobs, uint8_t* out_commitments48, int8_t* status /* n, may be NULL */);
int nbls_kzg_compute_proofs(nbls_ctx* ctx, const nbls_kzg_setup* setup, size_t n, const uint8_t* blobs, const uint8_t* z32, uint8_t* out_proofs48, uint8_t* out_y32,
                            int8_t* status /* n, may be NULL */);
int nbls_kzg_compute_blob_proofs(nbls_ctx* ctx, const nbls_kzg_setup* setup, size_t n, const uint8_t* blobs, const uint8_t* commitments48 /* or NULL */,
                                 uint8_t* out_commitments48 /* required when commitments48 == NULL */, uint8_t* out_proofs48, int8_t* status /* n, may be NULL */);

/* PeerDAS (EIP-7594, polynomial-commitments-sampling.md: compute_cells, compute_cells_and_kzg_proofs) and the transform it rests on.  Conventions as above: N = 2^log2_n,
 * omega_N = 7^((r - 1) / N), w_j = omega_N^rev(j), elements 32 bytes big-endian and CANONICAL, blobs = the values on w_j in bit-reversed order.  NOT an interface for secrets.
 *
 * nbls_fr_ntt: the transform between the two forms of n polynomials.  Polynomial i has the coefficients c_0 .. c_(N-1) in natural order, lowest first; its values are
 *   v_j = p_i(s_i w_j)   in the bit-reversed order of nbls_fr_eval_roots,   s_i = shift32[i], or 1 when shift32 == NULL.
 * NBLS_NTT_TO_COEFFS maps values to coefficients, NBLS_NTT_TO_EVALS coefficients to values.  status[i] (may be NULL): 0; NBLS_ST_NON_CANONICAL when an element or the shift
 * is >= r; 5 when the shift is 0 mod r; in both cases row i is all-zero and the neighbours are not disturbed.  One copy in, one kernel (a workgroup per polynomial, the whole
 * polynomial in LDS: a decimation network that takes natural order to bit-reversed order and back, so that no permutation pass exists), one copy out; the tables of the roots
 * and of their inverses are built on first use of a size and kept with the context.  NBLS_EINVAL before any device work for log2_n outside 1 .. 12, an unknown direction, a
 * NULL context, missing buffers with n > 0, more than 2^24 elements in the call; n = 0 is NBLS_OK. */
#define NBLS_NTT_TO_COEFFS 0
#define NBLS_NTT_TO_EVALS 1
int nbls_fr_ntt(nbls_ctx* ctx, unsigned log2_n /* 1 .. 12 */, int dir, size_t n, const uint8_t* in32 /* n << log2_n */, const uint8_t* shift32 /* n, or NULL */,
                uint8_t* out32 /* n << log2_n */, int8_t* status /* n, may be NULL */);
/* nbls_fr_ntt_large / nbls_fr_ntt_dev: the same transform for N = 2^log2_n up to 2^24 elements a polynomial, with nbls_fr_ntt's contract word for word: coefficients in
 * natural order, values p_i(s_i w_j) in bit-reversed order, canonical 32-byte big-endian elements, status 0 / NBLS_ST_NON_CANONICAL / 5 for a zero shift (non-canonical
 * before zero), a refused row all-zero, its neighbours not disturbed.  With t the log size of the tails (12) and K = log2_n - t:
 *   log2_n <= t    the kernel of nbls_fr_ntt, launched as nbls_fr_ntt launches it: the same bytes;
 *   log2_n >  t    towards the values: the first K stages of the same network as launches over runs of at most P consecutive stages (a workgroup holds 2^q rows of 2^c
 *                  contiguous elements in LDS and reads only the table of 2^K roots: T_N[j] = T_(2^K)[j] for j < 2^K, so no table of N roots exists), then one launch of
 *                  2^K tails a polynomial: block B holds p mod (X^(2^t) - T_N[B]), whose values are those of the transform of size 2^t with the shift omega_N^rev_K(B).
 *                  Towards the coefficients: the tails first, then the runs in reverse order, then 1 / N.  The first launch checks the canonical form and multiplies by
 *                  s^i (the last by (1 / s)^i); a refused polynomial raises a flag word in scratch that the last launch turns into zeros and the status.
 * t and P are NBLS_TUNE_NTT_TAIL_BITS / _PASS_BITS; the bytes never depend on them.  K <= 12 is required (NBLS_EINVAL otherwise: a tail size below log2_n - 12).
 * NBLS_EINVAL before any device work for log2_n outside 1 .. 24, an unknown direction, a NULL context, missing buffers with n > 0, more than 2^24 elements in the call;
 * n = 0 is NBLS_OK.
 * nbls_fr_ntt_dev works on device memory and is asynchronous: ordered on `stream` (NULL: the context's) like the other _dev calls.  d_in32 and d_out32 are 16-byte
 * aligned; d_out32 may equal d_in32 (every launch reads and writes the same disjoint set of elements per workgroup), any other overlap is NBLS_EINVAL.  d_shift32: n x 32
 * bytes or NULL; d_status: n bytes or NULL.  At 2^24 elements a host-buffer call moves 1 GB over the bus: callers that keep their polynomials on the device want this form. */
int nbls_fr_ntt_large(nbls_ctx* ctx, unsigned log2_n /* 1 .. 24 */, int dir, size_t n, const uint8_t* in32 /* n << log2_n */, const uint8_t* shift32 /* n, or NULL */,
                      uint8_t* out32 /* n << log2_n */, int8_t* status /* n, may be NULL */);
int nbls_fr_ntt_dev(nbls_ctx* ctx, unsigned log2_n /* 1 .. 24 */, int dir, size_t n, const void* d_in32, const void* d_shift32 /* or NULL */, void* d_out32,
                    void* d_status /* n bytes, or NULL */, void* stream);
/* compute_cells for n blobs with c = 2^log2_cell elements per cell (0 <= log2_cell <= log2_n; mainnet: log2_n = 12, log2_cell = 6, 128 cells of 64 elements).  With g = omega_2N
 * and p the blob's polynomial, the extension in bit-reversed order over 2 N is  ext[i] = blob[i],  ext[N + i] = p(g w_i);  cell k is ext[c k .. c k + c), its points are
 * h_k omega_c^rev(j) with h_k = g^rev(k) over log2_n + 1 - log2_cell bits (coset_for_cell).  out_cells holds, per blob, the 2 N elements in cell order: the blob's own bytes,
 * then the coset values.  One chain per blob in ONE kernel: the canonical check, to coefficients, times g^i / N, to values; nothing crosses the host in between.
 * status[i] (may be NULL): 0, or NBLS_ST_NON_CANONICAL for a blob with an element >= r: ALL its cells are then all-zero bytes, the neighbours are not disturbed.
 * NBLS_EINVAL before any device work for log2_n outside 1 .. 12, log2_cell > log2_n, a NULL context, missing buffers with n > 0, more than 2^24 elements in the call; n = 0 is
 * NBLS_OK.  The formulas are the EIP's; the consensus-spec test vectors have not been run against this call. */
int nbls_kzg_compute_cells(nbls_ctx* ctx, unsigned log2_n, unsigned log2_cell, size_t n, const uint8_t* blobs /* n * (32 << log2_n) */,
                           uint8_t* out_cells /* n * (64 << log2_n) */, int8_t* status /* n, may be NULL */);
/* nbls_kzg_monomial: the setup's g1_monomial in device memory, decoded ONCE: monomial48 holds the 2^log2_n compressed points [tau^i]G1, i = 0 .. N - 1, in NATURAL order.
 * Decoding, the subgroup check, status[], NBLS_EDECODE for an entry that does not decode or is the zero point (*out = NULL), lifetime and the device rule are those of
 * nbls_kzg_setup_create; the points are kept in the batched MSM's converted form.  A handle type of its own: the Lagrange setup is not accepted in its place. */
typedef struct nbls_kzg_monomial nbls_kzg_monomial;
int  nbls_kzg_monomial_create(nbls_ctx* ctx, unsigned log2_n, const uint8_t* monomial48 /* 2^log2_n compressed G1 points */, int8_t* status /* 2^log2_n, may be NULL */,
                              nbls_kzg_monomial** out);
void nbls_kzg_monomial_destroy(nbls_kzg_monomial* m);
int  nbls_kzg_monomial_log2n(const nbls_kzg_monomial* m, unsigned* log2_n);
/* compute_cells_and_kzg_proofs: the cells of nbls_kzg_compute_cells and, for every cell k, the proof  sum_i [q_i] [tau^i]G1  of the floor quotient q of p by the cell's
 * vanishing polynomial X^c - s_k (s_k = h_k^c) in coefficient form:  q_i = 0 for i >= N - c,  q_i = p_(i + c) + s_k q_(i + c)  downwards.  The coefficients stay on the device
 * after the transform; a kernel writes the 2 N / c quotient rows of every blob as big-endian scalars straight into the batched MSM's scalar array (one lane per chain of the
 * recurrence), the rows form of the batched MSM runs against the converted basis, then to-affine, compression and the closing kernel of the prover calls.  No FK20 (see nbls_kzg_compute_cells_and_proofs_fk20): 2 N / c sums
 * of N points per blob.  The batched MSM takes 2^22 scalars and 2^20 rows a pass, so the call works through the blobs in chunks of whole blobs (8 mainnet blobs; fewer with
 * NBLS_TUNE_CELLS_CHUNK) on one stream; the bytes do not depend on the chunks.  out_proofs48: n * (2 N / c) compressed points, blob by blob, cell by cell; ZERO POINTS ARE VALID
 * (0xc0 00.., status 0: a polynomial of degree < c).  status[i] (may be NULL): 0, or NBLS_ST_NON_CANONICAL: that blob's cells are all-zero and its proofs 48 zero bytes each.
 * Returns NBLS_OK whatever the blobs hold; NBLS_EINVAL before any device work for a missing pointer, n = 0, log2_cell > log2_n, a basis created on another device, more than
 * 2^24 elements in the call, or one blob alone above the bounds of a pass: (2 N / c) * N > 2^22. */
int nbls_kzg_compute_cells_and_proofs(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n, const uint8_t* blobs, uint8_t* out_cells,
                                      uint8_t* out_proofs48 /* n * (2 N / c) * 48 */, int8_t* status /* n, may be NULL */);
/* verify_cell_kzg_proof_batch: n_cells cells, each with its proof, against commitments given ONCE each and named by index (the specification deduplicates them the same way;
 * a commitment no cell names is decoded and otherwise ignored; cells may repeat).  N comes from the handle, c = 2^log2_cell; cell k of the call is cell number cell_index[k]
 * (< 2 N / c) of the blob committed to by commitments48[commitment_index[k]]: c elements, byte for byte one cell of nbls_kzg_compute_cells' output, on the coset h <omega_c>,
 * h = g^rev(cell_index[k]), s = h^c.  With I, of degree < c, interpolating the cell, it holds exactly when
 *   e(pi, [tau^c]G2) = e(C - [I(tau)]G1 + [s]pi, G2);
 * the cells are checked together by a random linear combination with the weights r_k of nbls_verify_multiple, indexed by the cell's position k in the call (same seed rule: NULL
 * = 32 bytes from getrandom(2) on every call, never a fixed seed):
 *   e(sum_k [r_k]pi_k, [tau^c]G2) * e(sum_k [r_k]C_k - sum_(i<c) [S_i][tau^i]G1 + sum_k [r_k s_k]pi_k, -G2) = 1,   S_i = sum_k r_k (coefficient i of I_k) mod r.
 * This is the specification's verify_cell_kzg_proof_batch_impl with SECRET WEIGHTS in place of its Fiat-Shamir powers, as nbls_kzg_verify_proofs.  A kernel with c lanes per
 * cell interpolates every cell in registers (a coset inverse transform of size c), weighs and sums: the n_cells * c coefficients never reach memory on the accepting path.  The
 * sum over [tau^i]G1 uses the handle's first c converted points; a Lagrange nbls_kzg_setup is not accepted in the handle's place.  log2_cell <= 6 IS A DELIBERATE LIMIT: the
 * EIP's cell has 64 elements and one wavefront holds one cell (nbls_kzg_compute_cells has larger cells only as test sizes).
 * Commitments and proofs: 48 bytes compressed, PointG1.fromHex's rules, subgroup check included, every commitment decoded once.  tau_c_g2_96: [tau^c]G2 = the setup's
 * g2_monomial[c], 96 bytes compressed, PointG2.fromSignature's rules.  Cell elements must be canonical.  ZERO POINTS ARE VALID: 0xc0 00.. is the zero polynomial's commitment
 * and the proof of any cell of a polynomial of degree < c; a zero point takes part as the identity and status 1 is never reported; either or both combined points may be the
 * zero point (both: accepted; exactly one: rejected).
 * status[k] (may be NULL), in this order: the named commitment's decoder status if >= 2; else 10 + the proof decoder's status if >= 2; else NBLS_ST_NON_CANONICAL when an
 * element of the cell is >= r; else 0, or NBLS_ST_NOT_VERIFIED.  *all_ok = 1 exactly when every status is 0.  A cell with one of the first three statuses has weight zero
 * everywhere, and the combined check never accepts while there is one; a neighbour is never disturbed.  Where the combined check does not accept, a per-cell pass judges every
 * cell with the single-cell equation (the two prepared tables shared by all cells, one batched final exponentiation; a zero proof holds exactly when the G1 point on the right
 * is the zero point); with status == NULL the call stops after the combined check instead and answers *all_ok = 0 (fast reject).
 * Returns NBLS_OK whatever the cells hold; NBLS_EDECODE when tau_c_g2_96 does not decode or is the zero point; NBLS_EINVAL before any device work for a missing pointer,
 * n_cells = 0 or n_commitments = 0, a handle created on another device, log2_cell > 6 or > log2_n, log2_n + 1 - log2_cell > 12 (more cells per blob than the largest table of
 * roots has entries), a cell_index >= 2 N / c, a commitment_index >= n_commitments, n_cells > 2^20 or n_cells << log2_cell > 2^22 (one pass of the batched MSM, which the
 * per-cell pass needs), n_commitments > 2^22.  *all_ok and status are NOT written when the call returns an error, NBLS_EDECODE included.  NOT an interface for secrets.  The
 * consensus-spec test vectors have not been run. */
int nbls_kzg_verify_cells(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n_commitments, const uint8_t* commitments48, size_t n_cells,
                          const uint32_t* commitment_index /* n_cells */, const uint32_t* cell_index /* n_cells */, const uint8_t* cells /* n_cells * (32 << log2_cell) */,
                          const uint8_t* proofs48 /* n_cells */, const uint8_t* tau_c_g2_96, const uint8_t* seed32 /* NULL: from the OS */, int* all_ok,
                          int8_t* status /* n_cells, may be NULL */);
/* recover_cells_and_kzg_proofs: every cell of n blobs (and, in the second form, every cell proof) from at least half of each blob's cells.  Blob i owns the entries
 * cell_offsets[i] .. cell_offsets[i + 1] of cell_index and of cells (non-decreasing offsets, the first 0); entry e is cell number cell_index[e] of that blob, c = 2^log2_cell
 * elements, byte for byte one cell of nbls_kzg_compute_cells' output.  The indices of a blob may come in ANY ORDER (a caller who wants the stricter rule of some libraries,
 * ascending order, checks it itself).  out_cells is laid out exactly as nbls_kzg_compute_cells lays it out (the blob first, then the coset values), out_proofs48 exactly as
 * nbls_kzg_compute_cells_and_proofs; for a blob with status 0 both are byte for byte what those two calls return for the recovered blob.  ZERO POINTS ARE VALID, as there:
 * 0xc0 00.. with status 0.
 * The route never transforms at size 2 N (a row of 2 N elements does not fit the LDS of a compute unit): the vanishing polynomial Z of the missing cells is constant on
 * every cell, so a blob takes M = 2 N / c values of it and M / 2 inversions, and six transforms of size N: E Z on H and on gH to the two halves A + B and A - B of
 * P Z = A + x^N B, their combination A + 7^N B to the values on the coset 7 H, divided block by block, back to the coefficients of P, and from those the cells (fr_exec.h).
 * The index sets are checked on the host before the copy; everything else happens on the device between one copy in and one copy out, in two launches whatever n is, then
 * the proofs exactly as nbls_kzg_compute_cells_and_proofs makes them from the coefficients (chunks of whole blobs, NBLS_TUNE_CELLS_CHUNK; the bytes do not depend on them).
 * After the coefficients are found the call compares the recomputed cells with EVERY given cell: with more than half of the cells an input can contradict itself, and is then
 * refused, not answered with route-dependent bytes.  (With exactly half, every canonical input is consistent: N points always interpolate.)
 * status[i] (may be NULL), the first that applies: NBLS_ST_BAD_CELLS; NBLS_ST_NON_CANONICAL: a given element is >= r; NBLS_ST_INCONSISTENT; 0.  Any non-zero status leaves
 * that blob's cells all-zero and its proofs 48 zero bytes each; a neighbour is never disturbed.  Returns NBLS_OK whatever the blobs hold; NBLS_EINVAL before any device work
 * for a missing pointer (cell_index and cells may be NULL only when no cell is given at all: every blob is then NBLS_ST_BAD_CELLS), decreasing offsets or a first offset
 * other than 0, log2_n outside 1 .. 12, log2_cell > log2_n, log2_n + 1 - log2_cell > 12 (the table of the 2 N / c roots), more than 2^24 elements of blobs in the call;
 * the proofs form also for n = 0 (the cells form answers NBLS_OK, as nbls_kzg_compute_cells), a basis created on another device, or one blob alone above a pass of the
 * batched MSM: (2 N / c) * N > 2^22.  NOT an interface for secrets.  The consensus-spec test vectors have not been run. */
#define NBLS_ST_BAD_CELLS 22      /* recovery: fewer than half of the blob's cells given, a cell index >= 2 N / c, or a cell given twice */
#define NBLS_ST_INCONSISTENT 23   /* recovery: no polynomial of degree < N has all the given cells */
int nbls_kzg_recover_cells(nbls_ctx* ctx, unsigned log2_n, unsigned log2_cell, size_t n /* blobs */, const uint32_t* cell_offsets /* n + 1 */,
                           const uint32_t* cell_index /* cell_offsets[n] entries */, const uint8_t* cells /* cell_offsets[n] * (32 << log2_cell) */,
                           uint8_t* out_cells /* n * (64 << log2_n) */, int8_t* status /* n, may be NULL */);
int nbls_kzg_recover_cells_and_proofs(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, size_t n, const uint32_t* cell_offsets,
                                      const uint32_t* cell_index, const uint8_t* cells, uint8_t* out_cells, uint8_t* out_proofs48 /* n * (2 N / c) * 48 */,
                                      int8_t* status /* n, may be NULL */);
/* FK20 (Feist-Khovratovich): all 2 N / c cell proofs of a blob together, from two small passes of the batched MSM.  THE CONTRACT: for every input the two *_fk20 calls return
 * byte for byte what nbls_kzg_compute_cells_and_proofs and nbls_kzg_recover_cells_and_proofs return -- cells, proofs, statuses, return codes: NBLS_ST_NON_CANONICAL (cells
 * all-zero, proofs 48 zero bytes), NBLS_ST_BAD_CELLS, NBLS_ST_INCONSISTENT, zero points as 0xc0 00.. with status 0, status == NULL -- and make the same refusals, with the
 * handle in the monomial's place and log2_cell taken from the handle.  With n' = N / c, M = 2 n', w_i = omega_M^rev(i) (the order of the Fr network's output):
 *   proof_k = sum_(u <= n' - 2) [s_k^u] h_u,  h_u = sum_(j < c) sum_t [p_(j + c (t + u + 1))] [tau^(j + c t)]G1 = IDFT_M(y^)_(n' - 1 + u),
 *   y^_i = sum_(j < c) [a^[j][i]] X^[j][i],  a^[j] = DFT_M of stripe j of the coefficients, X^[j] = DFT_M of stripe j of the basis reversed (both zero-padded: no wrap-around);
 *   proof_k = sum_i [B[k][i]] y^_i with the fixed matrix B[k][i] = 1 / M sum_u s_k^u w_i^(-(n' - 1 + u)).
 * No butterfly network over G1: pass A is M groups of c terms per blob (2 N scalars: 2^22 a pass), pass B M groups of M terms per blob (M^2 scalars a blob), 2^20 groups a
 * pass either way: 256 mainnet blobs a chunk, fewer with NBLS_TUNE_CELLS_CHUNK (the same key; the bytes do not depend on it).  The sums of pass A stay projective between the
 * passes (the identity is an ordinary point there).
 * The handle holds the c M points X^ (converted as the batched MSM reads them, index i c + j) and B (split), about 4 MB at the mainnet size; created on the device from the
 * monomial handle by ONE batched MSM of c M groups of n' - 1 terms and two kernels.  Lifetime and device rules: nbls_kzg_setup_create's.  nbls_kzg_fk20_create returns
 * NBLS_EINVAL before any device work, with *out = NULL (as on every failure), for a missing pointer, a basis on another device, log2_cell > log2_n, log2_n + 1 - log2_cell > 12,
 * or (2 N / c) * N > 2^22 (the size of the creation MSM, and the bound of the other form).  n' = 1 (every proof the zero point) and n' = 2 are legal. */
typedef struct nbls_kzg_fk20 nbls_kzg_fk20;
int  nbls_kzg_fk20_create(nbls_ctx* ctx, const nbls_kzg_monomial* monomial, unsigned log2_cell, nbls_kzg_fk20** out);
void nbls_kzg_fk20_destroy(nbls_kzg_fk20* fk);
int  nbls_kzg_fk20_params(const nbls_kzg_fk20* fk, unsigned* log2_n, unsigned* log2_cell);
int  nbls_kzg_compute_cells_and_proofs_fk20(nbls_ctx* ctx, const nbls_kzg_fk20* fk, size_t n, const uint8_t* blobs, uint8_t* out_cells,
                                            uint8_t* out_proofs48 /* n * (2 N / c) * 48 */, int8_t* status /* n, may be NULL */);
int  nbls_kzg_recover_cells_and_proofs_fk20(nbls_ctx* ctx, const nbls_kzg_fk20* fk, size_t n, const uint32_t* cell_offsets, const uint32_t* cell_index, const uint8_t* cells,
                                            uint8_t* out_cells, uint8_t* out_proofs48 /* n * (2 N / c) * 48 */, int8_t* status /* n, may be NULL */);

/* ---- Groth16 over BLS12-381: n proofs against one verifying key in one call (the shape of Zcash Sapling and Filecoin batches).  The key holds alpha in G1, beta, gamma, delta
 * in G2 and IC_0 .. IC_m in G1, m = the number of public inputs.  Proof i = (A_i, B_i, C_i) with inputs x_i1 .. x_im holds when, with L_i = IC_0 + sum_j [x_ij]IC_j,
 *   e(A_i, B_i) * e(L_i, -gamma) * e(C_i, -delta) * e(alpha, -beta) = 1.
 * n proofs are checked together with the secret weights r_i of nbls_verify_multiple (r_i = BE64(SHA-256(seed || BE64(i))[0..8]) | 2^63; the same seed rule: NULL = 32 bytes
 * from the OS on every call, never a fixed seed):
 *   prod_i e([r_i]A_i, B_i) * e(sum_j [S_j]IC_j, -gamma) * e(sum_i [r_i]C_i, -delta) * e([S_0]alpha, -beta) = 1,   S_0 = sum_i r_i,  S_j = sum_i r_i x_ij mod r:
 * n + 3 Miller loops and ONE final exponentiation where the per-proof equation takes 4 n and n.  The signs sit on the fixed G2 points: no point is negated on the device.
 * ENCODINGS: G1 points are 48 bytes compressed by PointG1.fromHex's rules, G2 points 96 bytes compressed by PointG2.fromSignature's rules, both with the subgroup check, as
 * everywhere in this header; a proof is A || B || C, 192 bytes (bellman's Proof::write); inputs are 32 bytes big-endian and must be canonical, as in the KZG calls.  Parsing
 * bellman's uncompressed verifying-key file (VerifyingKey::write) into these points stays with the caller.
 *   nbls_groth16_vk_create       decodes the key once and keeps, in memory of ctx's device: alpha affine; the prepared line tables of -beta, -gamma, -delta; the IC points affine
 *                                and in the batched MSM's converted form.  status[] (m + 5, may be NULL), in the order alpha, beta, gamma, delta, IC_0 .. IC_m: the decoder's
 *                                status.  An entry that does not decode, or is the zero point (status 1), makes the call return NBLS_EDECODE with *out = NULL; the statuses are
 *                                written in both cases, as nbls_kzg_setup_create does.  Lifetime and device rules: nbls_kzg_setup_create's (any context on the same device may
 *                                use the handle, also after its creator is destroyed).  NBLS_EINVAL for a missing pointer, m = 0 or m > 2^16.
 *   nbls_groth16_verify          status[i] (n, may be NULL), the first that applies: A's decoder status if >= 1 (1 = the zero point, which bellman's reader refuses too; 3; 4);
 *                                10 + B's decoder status if >= 1; NBLS_ST_G16_C + C's decoder status if >= 1; NBLS_ST_NON_CANONICAL for an input >= r; else 0 or
 *                                NBLS_ST_NOT_VERIFIED.  *all_ok = 1 exactly when every status is 0.  A proof with one of the first four statuses has weight zero everywhere,
 *                                the combined check never accepts while there is one, and a neighbour is never disturbed.  The combined check does not count either when one of
 *                                its three combined G1 points is the zero point (nbls_verify_multiple's rule for a zero weighted signature sum).  Where it does not accept:
 *                                with status == NULL the call stops and answers *all_ok = 0 (fast reject); else a per-proof pass judges every proof with the single-proof
 *                                equation -- L_i from the rows form of the batched MSM against the handle's converted points plus IC_0 (a zero L_i is a factor of one),
 *                                Miller loops against the three shared tables, one batched final exponentiation -- in chunks of whole proofs under the batched MSM's bounds
 *                                of 2^22 scalars and 2^20 rows (NBLS_TUNE_G16_CHUNK: fewer; the bytes do not depend on the chunks).  Returns NBLS_OK whatever the proofs hold;
 *                                NBLS_EINVAL before any device work for a missing pointer, n = 0, n > 2^20, n * m > 2^24, a key on another device.  *all_ok and status are
 *                                NOT written on an error return.  One chain on the context's stream; nothing is decided on the host before the one read-back of verdict,
 *                                zero flags and statuses.
 *   nbls_groth16_prepare_inputs  out48[i] = compress(L_i); status[i] (n, may be NULL): 0; 1 when L_i is the zero point (bytes 0xc0 00..); NBLS_ST_NON_CANONICAL (48 zero bytes).
 *                                The same chunks, bounds and refusals.
 *   nbls_groth16_input_sums      the folding kernel on caller-chosen weights (it exists for tests, as nbls_map_uniform_batch exposes the maps): out32[0] = sum w_i,
 *                                out32[j] = sum w_i x_ij mod r, over the rows with pre[i] == 0 and all inputs canonical; status[i] = pre[i], else NBLS_ST_NON_CANONICAL, else 0.
 *                                NBLS_EINVAL for a weight >= 2^64, n or m = 0, n * m > 2^24, a missing pointer.
 * NOT an interface for secrets: proofs, inputs and keys are public, and nothing is wiped. */
#define NBLS_ST_G16_C 30          /* nbls_groth16_verify: NBLS_ST_G16_C + the decoder's status of C */
typedef struct nbls_groth16_vk nbls_groth16_vk;
int  nbls_groth16_vk_create(nbls_ctx* ctx, size_t m, const uint8_t* alpha_g1_48, const uint8_t* beta_g2_96, const uint8_t* gamma_g2_96, const uint8_t* delta_g2_96,
                            const uint8_t* ic48 /* m + 1 */, int8_t* status /* m + 5, may be NULL */, nbls_groth16_vk** out);
void nbls_groth16_vk_destroy(nbls_groth16_vk* vk);
int  nbls_groth16_vk_inputs(const nbls_groth16_vk* vk, size_t* m);
int  nbls_groth16_verify(nbls_ctx* ctx, const nbls_groth16_vk* vk, size_t n, const uint8_t* proofs192, const uint8_t* inputs32 /* n * m */, const uint8_t* seed32 /* NULL: from the OS */,
                         int* all_ok, int8_t* status /* n, may be NULL */);
int  nbls_groth16_prepare_inputs(nbls_ctx* ctx, const nbls_groth16_vk* vk, size_t n, const uint8_t* inputs32, uint8_t* out48 /* n */, int8_t* status /* n, may be NULL */);
int  nbls_groth16_input_sums(nbls_ctx* ctx, size_t n, size_t m, const uint8_t* inputs32, const uint8_t* weights32 /* n, each < 2^64 */, const int8_t* pre /* n, may be NULL */,
                             uint8_t* out32 /* m + 1 */, int8_t* status /* n, may be NULL */);

/* The Groth16 prover: from a witness to the 192 bytes nbls_groth16_verify reads, against a proving key kept on the device.  Conventions as above: N = 2^log2_n,
 * omega = omega_N = 7^((r - 1) / N), Fr elements 32 bytes big-endian and CANONICAL, G1 points 48 bytes compressed (PointG1.fromHex), G2 points 96 bytes compressed
 * (PointG2.fromSignature), both decoders with the subgroup check, a proof A || B || C; "values in bit-reversed order" is nbls_fr_ntt's order: position i holds the value at
 * omega^rev(i).
 * The statement: an R1CS instance of three sparse N-row matrices A, B, C over Fr with n_vars columns -- the first n_constraints <= N rows given in CSR form, the others
 * empty, row j belonging to the domain point omega^j -- and the assignment z = (1, x_1 .. x_m, aux ..) with m = n_public inputs.  With a = A z, b = B z, c = C z, their
 * interpolants a(X), b(X), c(X) and Z = X^N - 1, the quotient is h = (a b - c) / Z: N coefficients, the top one zero.  The proof for the blinding scalars (r, s):
 *   A = alpha_g1 + sum_i [z_i] a_query_i + [r] delta_g1
 *   B = beta_g2 + sum_i [z_i] b_g2_query_i + [s] delta_g2          (B1: the same in G1, with beta_g1 / b_g1_query / delta_g1)
 *   C = sum_{i > m} [z_i] l_query_(i-m-1) + sum_{k < N-1} [h_k] h_query_k + [s] A + [r] B1 - [r s] delta_g1
 * This is meant to be bellman's ProvingKey -- h_query_k = [tau^k Z(tau) / delta]G1, l_query = [(beta A_i + alpha B_i + C_i)(tau) / delta]G1, omega and the row <-> omega^j
 * rule its EvaluationDomain's -- but NO bellman key or proof has been run against these calls: the compatibility is intended and untested; what is tested
 * is that nbls_groth16_verify accepts the proofs, and their bytes against a key with a known trapdoor.
 *   nbls_groth16_pk_create   decodes every point once and keeps in memory of its own on ctx's device: the three matrices with their coefficients in Montgomery limb form
 *                            and the rows ordered by length; the points as the four contiguous affine arrays the sums read (a_query | alpha_g1 | delta_g1; b_g1_query |
 *                            beta_g1 | delta_g1; b_g2_query | beta_g2 | delta_g2; l_query | h_query | [slot A] | [slot B1] | delta_g1); one mask byte per query point; and
 *                            the whole workspace of a proof (z in limb form, the three N-element vectors, the three scalar arrays, flags, result points).  status (may be
 *                            NULL): 5 + 3 n_vars + n_aux + N - 1 decoder statuses in the order of the descriptor's point fields, n_aux = n_vars - n_public - 1.  A ZERO POINT
 *                            (0xc0 00..) IS VALID in the four per-variable queries (a variable no constraint of that matrix names): status 1, the point masked -- a fixed
 *                            point of the subgroup stands in the array and its scalar is forced to zero.  A zero point among the five fixed points or in h_query, or any
 *                            entry that does not decode: NBLS_EDECODE, *out = NULL, the statuses written all the same (as nbls_groth16_vk_create).  NBLS_EINVAL before any
 *                            device work for a missing pointer, log2_n outside 1 .. 21, n_public = 0 or n_vars <= n_public, n_constraints > N, n_aux + N + 2 or n_vars + 2
 *                            above 2^22 (the bound of nbls_msm_dev on one sum), more than 2^24 entries in one matrix, offsets that decrease or do not start at 0, a column
 *                            >= n_vars, a non-canonical coefficient, b_g1_query[i] and b_g2_query[i] that disagree on being the zero point.  Lifetime and device rules are
 *                            nbls_groth16_vk_create's; the handle carries a lock: two contexts never prove on it at once.
 *   nbls_groth16_prove       n witnesses (1 .. 2^16), one chain each on the context's stream: one copy in -> the canonical check of z and (r, s), z to limb form, z_0 == 1 ->
 *                            a, b, c by g16p_spmv_kernel (rows of at least NBLS_TUNE_G16P_ROW_WAVE entries summed by a wavefront, the others by a lane; all three matrices of
 *                            a row in one place, so a_j b_j == c_j is checked there) -> the quotient as below (nbls_fr_ntt_dev, in place) -> the three scalar arrays with the
 *                            masks applied -> four sums by the bucket MSM of nbls_msm_dev (A and B1 written straight into their slots of the fourth array) -> compression.
 *                            One copy out of all proofs and statuses behind the last.  status[i] (may be NULL), the first that applies: NBLS_ST_NON_CANONICAL for an element
 *                            of z_i, r_i or s_i >= r; NBLS_ST_G16_UNSATISFIED; 1 when A or B is the zero point (the verifier refuses such a proof anyway); 0.  A proof whose
 *                            status is not 0 is 192 ZERO BYTES and never disturbs its neighbours; the call returns NBLS_OK whatever the witnesses hold.  rs32 == NULL: r_i and
 *                            s_i are drawn uniformly below r from getrandom(2) (32 bytes masked to 255 bits, redrawn while >= r); NBLS_ENOSUP when the OS gives none, never a
 *                            fixed value.  NBLS_EINVAL before any device work for a missing pointer, n = 0, n > 2^16, a key on another device.
 *                            THE WITNESS AND (r, s) ARE SECRETS: before the call returns the handle's copies of z, h and the scalar arrays and the staged block are zeroed on
 *                            the device and the page-locked host block is wiped (as nbls_sign_batch wipes its keys).  The bucket MSM's timing depends on the scalars, as
 *                            bellman's multiexp does: this is the only sense in which the call is not constant time.
 *   nbls_groth16_quotient    the quotient alone on caller-chosen vectors (it exists for tests, as nbls_groth16_input_sums exposes the folding kernel): n independent triples
 *                            a, b, c of N values in bit-reversed order -> h, N coefficients in natural order.  Each vector to coefficients, to the values on the coset
 *                            7 <omega> (any shift g with g^N != 1 gives the same h; 7 is bellman's), (a' b' - c') / (7^N - 1) per element, back to coefficients with the shift 7.
 *                            status[i] (may be NULL): NBLS_ST_NON_CANONICAL for a triple with an element >= r (the output row is then all-zero); NBLS_ST_G16_UNSATISFIED when
 *                            a_j b_j != c_j somewhere -- the output row is then what the same arithmetic gives, UNSPECIFIED bytes and no quotient of anything; 0.
 *                            NBLS_EINVAL for log2_n outside 1 .. 22 (or more than 12 above NBLS_TUNE_NTT_TAIL_BITS), more than 2^24 elements in a row set (n << log2_n), a
 *                            NULL context, missing buffers with n > 0; n = 0 is NBLS_OK.  Nothing here is wiped. */
#define NBLS_ST_G16_UNSATISFIED 24     /* z_0 != 1, or a row j with (Az)_j (Bz)_j != (Cz)_j */
typedef struct {
  unsigned log2_n; size_t n_vars, n_public /* m */, n_constraints /* <= N */;
  const uint32_t *a_rows, *a_cols; const uint8_t* a_vals32;      /* CSR: n_constraints + 1 offsets from 0, non-decreasing; columns < n_vars; canonical coefficients */
  const uint32_t *b_rows, *b_cols; const uint8_t* b_vals32;
  const uint32_t *c_rows, *c_cols; const uint8_t* c_vals32;
  const uint8_t *alpha_g1_48, *beta_g1_48, *beta_g2_96, *delta_g1_48, *delta_g2_96;
  const uint8_t *a_query48 /* n_vars */, *b_g1_query48 /* n_vars */, *b_g2_query96 /* n_vars */, *l_query48 /* n_vars - m - 1 */, *h_query48 /* N - 1 */;
} nbls_groth16_pk_desc;
typedef struct nbls_groth16_pk nbls_groth16_pk;
int  nbls_groth16_pk_create(nbls_ctx* ctx, const nbls_groth16_pk_desc* desc, int8_t* status /* 5 + 3 n_vars + n_aux + N - 1, may be NULL */, nbls_groth16_pk** out);
void nbls_groth16_pk_destroy(nbls_groth16_pk* pk);
int  nbls_groth16_pk_params(const nbls_groth16_pk* pk, unsigned* log2_n, size_t* n_vars, size_t* n_public);
int  nbls_groth16_pk_wiped(nbls_ctx* ctx, nbls_groth16_pk* pk, int* wiped);   /* for tests: *wiped = 1 when the handle's secret arrays (the staged witness and (r, s), z, a | b | c and h, the three scalar arrays) read back as zeros */
int  nbls_groth16_prove(nbls_ctx* ctx, nbls_groth16_pk* pk, size_t n, const uint8_t* witness32 /* n * n_vars, z_0 = 1 first */,
                        const uint8_t* rs32 /* n * 64: r_i || s_i; NULL: from the OS */, uint8_t* out_proofs192, int8_t* status /* n, may be NULL */);
int  nbls_groth16_quotient(nbls_ctx* ctx, unsigned log2_n, size_t n, const uint8_t* a32, const uint8_t* b32, const uint8_t* c32 /* n << log2_n each, values in bit-reversed order */,
                           uint8_t* out_h32 /* n << log2_n coefficients, natural order */, int8_t* status /* n, may be NULL */);

/* One rank's share of a verifyBatch spread over several GPUs (one process per GPU): the Miller product of this rank's n
 * (key, message) pairs, times millerLoop(-G, S) on the ONE rank that passes the signature (d_sig96 = NULL elsewhere), WITHOUT the
 * final exponentiation, as 576 wire bytes in device memory.  Ranks all-gather their partials and finish with
 * nbls_fp12_product_final_dev (product + shared finalExponentiate, index.ts:811-817), then compare with Fp12.ONE.
 * *zero_flag = 1: a zero point was met (verifyBatch answers false).  NBLS_EDECODE as nbls_verify_batch.  ABI 3: the call decides nothing on the host before its end, so d_out_fp12 IS
 * written in both cases -- with a meaningless product; look at the return code and the flag first. */
/* d_uniform256: an item whose two field elements satisfy u0 = +-u1 mod p is outside the contract (see nbls_map_uniform_batch): the hash stage yields the zero point for it, handed to
 * the Miller loop as all-zero affine bytes and NOT reported through *zero_flag, so the partial product is unspecified; the hash points of the other items are unaffected. */
int nbls_verify_batch_partial_dev(nbls_ctx* ctx, size_t n, const void* d_sig96 /* or NULL */, const void* d_uniform256, const void* d_pk48,
                                  void* d_out_fp12, int* zero_flag, int8_t* pk_status /* n, may be NULL */, void* stream);

/* The same as one device's share of a product that is spread over several GPUs, from HOST inputs: on return *d_partial points at 576 wire
 * bytes on the context's device, ready for hipMemcpyPeer / a collective; the call returns when the partial is complete.  *d_partial is a pure
 * OUT parameter (ABI 2; ABI 1 of round 3 read it as well): it receives a buffer owned by the context, valid only until the context's next
 * *_partial call.  The `_into` forms write the partial to a caller-owned 576-byte device buffer on the context's device instead -- required when
 * several threads may use the context, because each call then owns its partial; a pointer that is not device memory of that device is refused
 * (NBLS_EINVAL).  An empty shard (n = 0, product only) yields the unit element. */
int nbls_miller_product_partial(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const uint8_t* g2_aff, int validate, void** d_partial, int8_t* status);
int nbls_verify_batch_partial(nbls_ctx* ctx, size_t n, const uint8_t* sig96 /* or NULL */, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pk48,
                              const uint8_t* dst, size_t dst_len, void** d_partial, int* zero_flag, int8_t* pk_status /* n, may be NULL */);
int nbls_miller_product_partial_into(nbls_ctx* ctx, size_t n, const uint8_t* g1_aff, const uint8_t* g2_aff, int validate, void* d_dst576, int8_t* status);
int nbls_verify_batch_partial_into(nbls_ctx* ctx, size_t n, const uint8_t* sig96 /* or NULL */, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pk48,
                                   const uint8_t* dst, size_t dst_len, void* d_dst576, int* zero_flag, int8_t* pk_status /* n, may be NULL */);
const char* nbls_config_describe(void);   /* "NBLS_X=value(env|default) ...": every environment switch the library has read so far and the value in force -- print it next to an A/B result */
/* 5: nbls_verify_multiple, NBLS_ST_NOT_VERIFIED, scratch slots 20 .. 43 (additions only); then nbls_verify_aggregates, nbls_verify_aggregates_indexed, nbls_keyset_create /
   _destroy / _size, scratch slots 44 .. 47 (additions only, same version); then nbls_verify_multiple_shared, nbls_verify_aggregates_shared,
   nbls_verify_aggregates_indexed_shared, scratch slots 48 .. 50 (additions only, same version); then nbls_fr_op_batch, nbls_lagrange_at_zero, nbls_g2_combine_shares,
   nbls_g1_combine_shares, NBLS_FROP_*, NBLS_ST_BAD_IDS, scratch slots 51 .. 56 (additions only, same version); then nbls_field_kernel_raw (addition only, same version); then nbls_g1_poly_eval,
   nbls_g2_poly_eval, nbls_extra_program_kernel, NBLS_TUNE_POLY_SLAB, scratch slots 57 .. 61 (additions only, same version); then nbls_g1_msm_batch, nbls_g2_msm_batch,
   nbls_g1_msm_rows, nbls_g2_msm_rows, NBLS_TUNE_MSMB_WINDOW / _BIG / _SLAB, the names "dbladd_g1" / "dbladd_g2" of nbls_extra_program_kernel, scratch slots 62 .. 63 (additions only, same version); then nbls_map_uniform_batch (addition only, same version); then nbls_fr_eval_roots, nbls_kzg_verify_proofs, nbls_kzg_verify_blobs, NBLS_ST_NON_CANONICAL, scratch slots 64 .. 68 (additions only, same version); then nbls_kzg_setup_create / _destroy / _log2n, nbls_fr_quotient_roots, nbls_kzg_commit_blobs, nbls_kzg_compute_proofs, nbls_kzg_compute_blob_proofs, scratch slots 69 .. 70 (additions only, same version); then nbls_fr_ntt, NBLS_NTT_*, nbls_kzg_compute_cells, nbls_kzg_monomial_create / _destroy / _log2n, nbls_kzg_compute_cells_and_proofs, NBLS_TUNE_CELLS_CHUNK, scratch slots 71 .. 73 (additions only, same version); then nbls_kzg_verify_cells, scratch slots 74 .. 78 (addition only, same version); then nbls_kzg_recover_cells, nbls_kzg_recover_cells_and_proofs, NBLS_ST_BAD_CELLS, NBLS_ST_INCONSISTENT, scratch slot 79 (additions only, same version); with the MSM calls ONE CHANGE TO EXISTING CALLS, same version: nbls_g1_msm / nbls_g2_msm write all-zero output bytes when the status is 1 (the sum is the
   zero point).  The bytes were unspecified there before (what the affine conversion made of a Z that is 0 mod p: in G1 a zero x and an arbitrary y); the status, and every output with status 0, are unchanged.
   nbls_msm_dev, which leaves its result on the device, is not changed.
   Then nbls_kzg_fk20_create / _destroy / _params, nbls_kzg_compute_cells_and_proofs_fk20, nbls_kzg_recover_cells_and_proofs_fk20, the name "endo_g1" of nbls_extra_program_kernel, scratch slots 80 .. 81 (additions only, same version). Then nbls_groth16_vk_create / _destroy / _inputs,
   nbls_groth16_verify, nbls_groth16_prepare_inputs, nbls_groth16_input_sums, NBLS_ST_G16_C, NBLS_TUNE_G16_CHUNK, scratch slots 82 .. 86 (additions only, same version).
   Then NBLS_TUNE_FE_TAIL_CHAIN, nbls_chain_launches and the name "fe_final12" of nbls_extra_program_kernel (additions only, same version).
   Then NBLS_TUNE_FE_HEAD_CHAIN, NBLS_TUNE_INV_PRIO and the name "fe_easy12" of nbls_extra_program_kernel (additions only, same version).
   Then nbls_fr_ntt_large, nbls_fr_ntt_dev, NBLS_TUNE_NTT_TAIL_BITS / _PASS_BITS, scratch slot 87 (additions only, same version).
   Then nbls_groth16_pk_create / _destroy / _params / _wiped, nbls_groth16_prove, nbls_groth16_quotient, NBLS_ST_G16_UNSATISFIED, NBLS_TUNE_G16P_ROW_WAVE, no scratch slot (additions only, same version).
   Then nbls_pool_init_ex, NBLS_POOL_SPREAD_PRIORITIES, nbls_pool_stream_priority (additions only, same version).
   Then NBLS_POOL_BALANCE, nbls_pool_outstanding (additions only, same version).
   4 (round 6): nbls_hw_queues, NBLS_TUNE_WIDE_MAX, NBLS_TUNE_H2C_NORM_MIN, NBLS_TUNE_INV_WIDE_MAX, NBLS_TUNE_LS_MAX / _LS2_MAX (additions only); the library sets GPU_MAX_HW_QUEUES = 22 at load when the variable is unset (see nbls_pool_init below).
   3 (round 5): nbls_program_kernel, nbls_pool_*, nbls_sign_batch_dev, NBLS_TUNE_VERIFY_* / _SAC_MAX / _PT_LS2_MAX (additions only); nbls_verify_batch_partial_dev writes d_out_fp12 even when it reports a zero point or a decode error
   (contents then meaningless); 2: *_partial take *d_partial as OUT only, *_partial_into added, nbls_tower_op_batch, nbls_verify_batch_msgs_dev.  The bindings check it at load. */
#define NBLS_ABI_VERSION 5
int nbls_abi_version(void);
int nbls_context_device(nbls_ctx* ctx);

/* ---- several calls in flight on ONE device (round 5): `depth` contexts, each with its own stream and scratch, fed round-robin (what noble-bls12-381_amd/pipeline.py does, for C
 * callers).  A 4096-pairing call alone fills the chip one wavefront deep and runs at ~0.27 of the multiply-add roofline; twelve overlapping calls (nbls_pool_*) reach ~0.45.
 * nbls_pool_pairing_batch_dev enqueues pairing(P_i, Q_i) (reference index.ts:715-722) for n device-resident pairs on the next context's stream and returns at once;
 * *slot (may be NULL) = the context used -- keep one output buffer per slot; nbls_pool_next_slot tells it in advance.
 * Hardware queues: the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), read once when the runtime initialises; streams that share a queue
 * serialise (a pool of twelve on four queues: 2.50 M instead of 2.98 M pairings/s, tests/c/pool_rate.c).  Round 6: libnbls.so sets GPU_MAX_HW_QUEUES = 22 when it is loaded and the variable is unset
 * (NBLS_KEEP_HW_QUEUES=1: never), which is in time for every process that loads the library before its first HIP call -- a C program linked against it, the N-API addon, a Python
 * process that imports the binding first.  A process that initialised HIP earlier sets the variable itself; nbls_pool_init warns on stderr when `depth` exceeds the value in force.
 * nbls_hw_queues: the value in the environment (0 = unset: the runtime's default of 4); *set_by_library (may be NULL) = 1 when the library put it there. */
int nbls_hw_queues(int* set_by_library);
typedef struct nbls_pool nbls_pool;
int nbls_pool_init(int device_id, int depth /* 1 .. 64 */, nbls_pool** out);      /* = nbls_pool_init_ex(device_id, depth, 0, out) */
/* Stream priorities against a queue cap.  The runtime's limit of GPU_MAX_HW_QUEUES hardware queues holds PER STREAM PRIORITY, not per process: streams of another priority
 * level get queues of their own.  A process that cannot raise the variable (HIP was initialised before the library was loaded, or the host fixes the value) asks for
 * NBLS_POOL_SPREAD_PRIORITIES: when `depth` exceeds the queues in force, context i's stream is created at priority level i mod L of the L levels of
 * hipDeviceGetStreamPriorityRange (level 0 = the default priority), so twelve contexts on three levels run on eleven hardware queues under a cap of four (the null stream holds one queue of the default level): 3.03 M pairings/s against 2.68 M,
 * and 3.10 M with 22 queues.  The levels are not served alike: the high level's streams finish a saturated burst first.  With depth <= queues, or one
 * level, every stream keeps the default priority (the flag is a no-op); with depth > L x queues the surplus streams share queues as before, and the warning says so.  The priority
 * is the QUEUE's: all contexts run the same kernels, the bytes do not depend on it.  Environment: NBLS_POOL_SPREAD = 0 / 1 overrides the flag (A/B runs), NBLS_POOL_SPREAD_LEVELS caps L.
 * nbls_pool_stream_priority: *priority = hipStreamGetPriority of context i's stream (0 = default, negative = higher). */
#define NBLS_POOL_SPREAD_PRIORITIES 1u
/* Who gets the next batch.  Round-robin gives every context the same number of batches whatever the rate its queue is served at (under a queue cap the priority levels are
 * not served alike, above), so a burst ends on the slowest queue alone and a service builds backlog on the slow contexts while the fast ones idle.  With NBLS_POOL_BALANCE
 * a context has at most K batches outstanding (default 2; environment NBLS_POOL_MAX_OUTSTANDING = 1 .. 8, anything else is NBLS_EINVAL at init) and a batch goes to the
 * context with the fewest, ties round-robin behind the context used last -- a pool nobody waits on still visits its contexts in index order.  Completion is seen through
 * one event per batch, recorded on the context's stream inside the library.  SUBMIT MAY NOW WAIT: with every context at K, nbls_pool_pairing_batch_dev -- and
 * nbls_pool_next_slot, which makes the same choice in advance -- blocks (polling, 50 us between rounds, no device synchronisation) until a batch completes; a HIP error seen
 * while waiting is returned as NBLS_EHIP (next_slot: -1) and nothing is submitted.  nbls_pool_next_slot latches its choice: called twice it returns the same slot, and the
 * submit that follows uses it; a submit with no next_slot before it chooses for itself.  Pair the two calls from one thread at a time.  Without the flag nothing changes
 * (strict round-robin, submit never waits); plain nbls_pool_init never sets it.  The bytes do not depend on it.  Environment: NBLS_POOL_BALANCE = 0 / 1 overrides the flag.
 * nbls_pool_outstanding: *n = batches enqueued on context i whose completion has not been seen yet (0 .. K; always 0 without the flag). */
#define NBLS_POOL_BALANCE 2u
int nbls_pool_init_ex(int device_id, int depth /* 1 .. 64 */, unsigned flags, nbls_pool** out);
int nbls_pool_stream_priority(nbls_pool* p, int i, int* priority);
int nbls_pool_outstanding(nbls_pool* p, int i, int* n);
void nbls_pool_destroy(nbls_pool* p);
int nbls_pool_depth(const nbls_pool* p);
nbls_ctx* nbls_pool_context(nbls_pool* p, int i);
int nbls_pool_next_slot(nbls_pool* p);
int nbls_pool_pairing_batch_dev(nbls_pool* p, size_t n, const void* d_g1, const void* d_g2, int with_final_exp, void* d_out, int* slot);
int nbls_pool_synchronize(nbls_pool* p);   /* everything submitted so far is complete (synchronises the device) */

/* Several GPUs of one node behind one handle (one context, host thread and stream per device; contiguous shards).  n_devices = 0 takes every
 * visible device; device_ids = NULL means 0 .. n_devices-1.  Independent pairings need no exchange; the product paths reduce every shard
 * to a 576-byte Fp12 partial, gather the partials on the first device with hipMemcpyPeer (xGMI) and run ONE shared final exponentiation
 * there.  Same arguments, results and error behaviour as the single-device calls of the same name. */
typedef struct nbls_multi nbls_multi;
int nbls_init_multi(int n_devices, const int* device_ids, nbls_multi** out);
void nbls_destroy_multi(nbls_multi* m);
int nbls_multi_device_count(const nbls_multi* m);
nbls_ctx* nbls_multi_context(nbls_multi* m, int i);
int nbls_multi_peer_access(const nbls_multi* m, int i);   /* 1: copies between device i and the reducing (first listed) device go peer to peer over xGMI; 0: staged by the runtime; -1: bad index */
int nbls_multi_pairing_batch(nbls_multi* m, size_t n, const uint8_t* g1_aff, const uint8_t* g2_aff, int with_final_exp, int validate,
                             uint8_t* out_fp12, int8_t* status);
int nbls_multi_miller_product(nbls_multi* m, size_t n, const uint8_t* g1_aff, const uint8_t* g2_aff, int final_exp, int validate,
                              uint8_t* out_fp12, int8_t* status);
int nbls_multi_verify_batch(nbls_multi* m, size_t n, const uint8_t* sig96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pk48,
                            const uint8_t* dst, size_t dst_len, int* ok);

/* Introspection for the benchmark / tests. */
int nbls_program_stats(nbls_ctx* ctx, int prog, uint32_t* out8);   /* steps, mul_steps, lin_steps, mul_ops, lin_ops, lin_terms, slots, lds_bytes */
int nbls_device_synchronize(nbls_ctx* ctx);
/* Placement study (tools/placement.py): runs one step program on n scratch items; out_blocks[5b..5b+4] = HW_ID | XCC_ID << 32, start tick, end tick (s_memtime), start, end time (s_memrealtime, 100 MHz) of workgroup b. */
int nbls_placement_probe(nbls_ctx* ctx, size_t n, uint64_t* out_blocks);
/* The stand-alone field kernels on raw operands (tests/test_gpu_field_kernels.py): kind 0 .. 3 = the fixed exponents (p+1)/4, (p^2+7)/16, (p^2-9)/16, (p-3)/4 (Fp.sqrt,
 * Fp2.sqrt, sqrt_div_fp2 and the SWU exponent: math.ts:251-264, 521-538, 1196-1198), kind 4 = the Montgomery inverse (Fp.invert, math.ts:134-156).  form 1: one element per lane
 * (kinds 1, 2: one pair of lanes), form 2: one limb per lane, form 0: what the pipelines' own dispatch takes for this n under the context's tuning.  Elements are the engine's raw
 * scratch elements, 64 bytes each: 14 little-endian 28-bit limbs in 32-bit words, then 8 zero bytes; any representative below 16 p (the inverse: below 2^392).  Kinds 1 and 2 read
 * and write 2 n elements, c0 then c1.  NBLS_EINVAL for an unknown kind or form, missing buffers with n > 0 and n > 2^24; n = 0 is NBLS_OK. */
int nbls_field_kernel_raw(nbls_ctx* ctx, int kind, int form, size_t n, const uint8_t* in_raw, uint8_t* out_raw);
/* Per-kernel HIP-event timing (benchmark roofline leg): ms[i]/counts[i] for program i, last entry = inversion kernel. */
#define NBLS_N_PROGRAMS 128
/* Tuning knobs of a context (defaults are the measured optimum; tests use them to force a code path).
 * NBLS_TUNE_SPLIT_MILLER_MIN: number of pairs from which the Miller loop runs as two programs (line tables through HBM) instead of one. */
#define NBLS_TUNE_SPLIT_MILLER_MIN 1
#define NBLS_TUNE_HALVES_MIN 2         /* pairs from which nbls_pairing_batch_dev runs a batch as two halves on two streams (default 16384 since the end of round 6, 8192 before; 0 = never) */
#define NBLS_TUNE_EXPC_MIN 3           /* items from which the cyclotomic exponentiations of the final exponentiation use Karabina's compressed squarings
                                          (default: never -- 15 % fewer instructions but no faster as measured, see csrc/pipelines_pairing.cpp expx; 0 = always) */
#define NBLS_TUNE_CHAIN_MAX 4          /* items below which EXPX, FE_MID1, EXPX x 3, FE_MID2, EXPX of a final exponentiation are ONE launch (default 8192; 0 = seven launches:
                                          what a caller that keeps several calls in flight on other contexts wants, csrc/runtime.cpp run_chain) */
#define NBLS_TUNE_VERIFY_CHUNKS 5      /* verifyBatch as concurrent sub-batches (csrc/pipelines_verify.cpp verify_pipeline): number of sub-batches the signatures are cut into (default 2; 0 or 1 = one) */
#define NBLS_TUNE_VERIFY_LAST_PCT 6    /* ... size of the last sub-batch in per cent of the batch (default 25; the sizes fall linearly from the first to the last) */
#define NBLS_TUNE_VERIFY_PIPE_MIN 7    /* ... signatures from which a call is cut at all (default 32768) */
#define NBLS_TUNE_SAC_MAX 8            /* keys up to which sign's ladder (points known to lie in G2) uses the sign-aligned recoding with one addition per bit (default 6144: every
                                        * wavefront of the launch resident at once; 0 = never: the windowed psi-split ladder at every size) */
#define NBLS_TUNE_PT_LS2_MAX 9         /* items up to which the G2 point chains of verify / sign (clearCofactor's two ladders, sign's ladder) run in their two-lane forms (default 4096; 0 = never) */
#define NBLS_TUNE_WIDE_MAX 10          /* round 6, experiment: items up to which the programs that allow it run on the one-limb-per-lane interpreter (one item per workgroup of three wavefronts, two barriers per step); bit-exact, measured slower than the four-lane forms (0.93 against 0.66 ms for a final exponentiation's five exponentiations), so the default is 0 = never */
#define NBLS_TUNE_H2C_NORM_MIN 11     /* round 6: messages from which hash-to-G2 (also inside sign / verify / verifyBatch) takes the square root of its SWU map by the norm method -- two Fp exponentiations and a short program between them instead of one Fp2 exponentiation of twice the work; the same points; less work but two dependent exponentiations, so it pays where the device is full or the chain runs beside other work: the size compared is the whole call's (default 32768; 0 = always) */
#define NBLS_TUNE_INV_WIDE_MAX 12     /* round 6: elements up to which an Fp inversion launch runs with one limb per lane, four elements per wavefront (shorter for ONE call, eight times the instructions per element: default 4096; nbls_pool_init sets 256 on its contexts; 0 = never) */
#define NBLS_TUNE_LS_MAX 13           /* items up to which the pairing programs run in their four-lane forms (default 1024; nbls_pool_init sets 0 on its contexts: the forms shorten ONE call at up to four times the instructions per item) */
#define NBLS_TUNE_LS2_MAX 14          /* ... in their two-lane forms, above LS_MAX (default 2048; pool contexts 0) */
#define NBLS_TUNE_POLY_SLAB 15        /* identifiers that nbls_g*_poly_eval works through at a time: the per-step coefficient buffer and the accumulators never exceed one slab (default 2^18; 0 = the default) */
#define NBLS_TUNE_MSMB_WINDOW 16      /* window width of nbls_g*_msm_batch / _rows: 4, 6, 8, 10 or 12 bits; 0 (default) = chosen per call: the width that minimises points * windows + windows * c * 2^(c - 1) for the mean group */
#define NBLS_TUNE_MSMB_BIG 17         /* points (as given) above which a group of nbls_g*_msm_batch / _rows runs through the pipeline of nbls_g*_msm on the same stream (default 16384; 0 = the default) */
#define NBLS_TUNE_MSMB_SLAB 18        /* budget of one slab of groups: sum over its groups of (points after the split) * windows + windows * c * 2^(c - 1), the sorted entries and gathered bucket points that are in scratch at a time; a group that exceeds it alone is a slab of its own (default 2^23; 0 = the default) */
#define NBLS_TUNE_CELLS_CHUNK 20      /* (19 stays unassigned: tests/test_msm_batch_abi.py pins it as the first unknown key behind the batched MSM's) blobs that nbls_kzg_compute_cells_and_proofs hands to the batched MSM in one pass; 0 (default) = as many whole blobs as its bounds of 2^22 scalars and 2^20 rows take (8 mainnet blobs); a larger value than that changes nothing.  The bytes do not depend on it: it lets a test cross chunk borders with small blobs */
#define NBLS_TUNE_G16_CHUNK 22        /* (21 stays unassigned: tests/test_kzg_fk20_abi.py pins it as the first unknown key behind NBLS_TUNE_CELLS_CHUNK) proofs that the per-proof pass of nbls_groth16_verify and nbls_groth16_prepare_inputs hand to the batched MSM in one pass; 0 (default) = as many whole proofs as its bounds of 2^22 scalars and 2^20 rows take; a larger value than that changes nothing.  The bytes do not depend on it: it lets a test cross chunk borders with few proofs */
#define NBLS_TUNE_FE_TAIL_CHAIN 24     /* (23 stays unassigned: tests/test_groth16_abi.py pins it as the first unknown key behind NBLS_TUNE_G16_CHUNK) a final exponentiation that runs launch by launch (a pool context, the halves of a large call) ends short programs inside the launch of the cyclotomic exponentiation before them, for the same items: bit 0 the final product (EXPX + FE_FINAL are one launch), bit 1 FE_MID1 and FE_MID2 likewise; 12 launches per pairing batch become 11 (1), 9 (3).  The bytes do not depend on it.  Default 0 (environment: NBLS_FE_TAIL_CHAIN); nbls_pool_init sets 3 on its contexts, whose streams may share hardware queues: there every launch boundary drains a queue */
#define NBLS_TUNE_NTT_TAIL_BITS 26    /* (25 stays unassigned: tests/test_fr_ntt_large_abi.py pins it as the first unknown key behind NBLS_TUNE_FE_TAIL_CHAIN) t, the log size of the tails of nbls_fr_ntt_large / nbls_fr_ntt_dev: 1 .. 12; 0 (default) = 12.  A transform of 2^log2_n elements with log2_n > t runs log2_n - t <= 12 global stages in front of (behind, on the way back) 2^(log2_n - t) transforms of size 2^t.  The bytes do not depend on it: it lets a test drive the split at sizes where Python integers are the oracle */
#define NBLS_TUNE_NTT_PASS_BITS 27    /* P, the global stages one launch of the same calls runs at most: 1 .. 9 (nine stages of rows of 8 elements fill the LDS tile of 2^12 elements); 0 (default) = 8.  The log2_n - t global stages are cut into ceil((log2_n - t) / P) runs whose lengths differ by one at most.  The bytes do not depend on it (28 stays unassigned) */
#define NBLS_TUNE_FE_HEAD_CHAIN 29     /* (25 and 28 stay unassigned: tests pin them as the first unknown keys of their time) 0 / 1: such a final exponentiation runs the easy part at the head of the first exponentiation's launch (FE_EASY + EXPX are one launch, and FE_MID1 with them under bit 1 of NBLS_TUNE_FE_TAIL_CHAIN) instead of as a launch of its own: 9 launches per pairing batch become 8.  The bytes do not depend on it.  Default 0 (environment: NBLS_FE_HEAD_CHAIN); nbls_pool_init sets 1 on its contexts */
#define NBLS_TUNE_INV_PRIO 30          /* 0 .. 3: the issue priority of the wavefronts of the one-element-per-lane Fp inversion kernel (launches above NBLS_TUNE_INV_WIDE_MAX elements); a wavefront of higher priority wins the arbitration for VALU issue against those of other launches on its SIMD.  The bytes do not depend on it.  Default 0 (environment: NBLS_INV_PRIO); nbls_pool_init sets its contexts' (nbls_multi.cpp POOL_INV_PRIO) */
#define NBLS_TUNE_G16P_ROW_WAVE 31     /* matrix entries from which a row is summed by a whole wavefront instead of one lane; 0 = default.  The bytes do not depend on it */
int nbls_set_tuning(nbls_ctx* ctx, int key, long long value);
int nbls_program_count(void);                 /* number of step programs; timing slot nbls_program_count() = the inversion kernel */
const char* nbls_program_name(int prog);
/* the kernel that executes program `prog` in this context: "nbls_aot_<name>" (ahead-of-time specialised, the product path) or "nbls_vm_kernel[_ls4]" (the interpreter:
   NBLS_AOT=0, or the build-time and run-time compilations of the program disagree); NULL on a bad index.  The string is static. */
const char* nbls_program_kernel(nbls_ctx* ctx, int prog);
/* the same for a step program outside the numbered ones, by name: "poly_g1_16", "poly_g1_256", "poly_g2_16", "poly_g2_256" (the Horner steps of nbls_g*_poly_eval, short and
   full form), "dbladd_g1", "dbladd_g2" (the doubling-and-add steps that combine the bit-slices of nbls_g*_msm_batch / _rows), "lines_fe" (the line program of the pairings that end in a
   final exponentiation; NBLS_LINES_FE=0 keeps "lines_pq" for them); NULL for any other name */
const char* nbls_extra_program_kernel(nbls_ctx* ctx, const char* name);
/* launches of such a program in this context so far, -1 for a name that is none (its launches are booked in the timing slot of the numbered program whose stage they serve) */
long long nbls_extra_program_launches(nbls_ctx* ctx, const char* name);
/* launches of this context so far that ran several step programs back to back as ONE launch (a chain: the middle of a final exponentiation, the forms of
   NBLS_TUNE_FE_TAIL_CHAIN); where a chain falls back to one launch per program (checked mode, NBLS_CHAIN=0) it does not count.  -1 without a context. */
long long nbls_chain_launches(nbls_ctx* ctx);
/* private (scratch) memory per lane of ahead-of-time kernel k = 0, 1, ... as loaded, -1 past the last one: 0 for every kernel of this build */
int nbls_aot_kernel_private_bytes(int k);
int nbls_timing_enable(nbls_ctx* ctx, int on);
int nbls_timing_read(nbls_ctx* ctx, float* ms /*[NBLS_N_PROGRAMS+1]*/, uint32_t* counts /*[NBLS_N_PROGRAMS+1]*/);

#ifdef __cplusplus
}
#endif
#endif
