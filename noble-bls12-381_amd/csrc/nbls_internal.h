// nbls_internal.h -- what the translation units of the runtime share (runtime.cpp / tuning.cpp / pipelines_pairing.cpp / pipelines_codec.cpp / pipelines_verify.cpp / pipelines_multi_verify.cpp / pipelines_threshold.cpp /
// pipelines_poly.cpp / pipelines_msm.cpp / kzg_common.cpp / pipelines_kzg.cpp / pipelines_kzg_prove.cpp / pipelines_kzg_cells.cpp / pipelines_kzg_verify_cells.cpp / pipelines_groth16.cpp / pipelines_groth16_prove.cpp; pool and multi-device handles: nbls_multi.cpp): the context, the
// map of its scratch slots (enum Slot: the one place that says which chain owns which slot, checked at compile time), the launch helpers, the staged block of the host-buffer pipelines (staging.h, included at the end) and the
// device-side pipelines the exported entry points are built from.  Internal functions have hidden visibility (csrc/Makefile: -fvisibility=hidden).
#pragma once
#include <hip/hip_runtime.h>
#include "config.h"
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>
#include <initializer_list>
#include <new>
#include "nbls.h"
#include "programs.h"
#include "consts_gen.h"
#include "fp_inv.h"
#include "pow_exec.h"
#include "sha256.h"
#include "curve.h"   // G1_FIXED_WIN and the table geometry of pt_mul_fixed_g1
#include "bufs.h"    // BufArg / B(), BufList, ChainLink, bind_bufs
#include "verifier_frame.h"   // the block formats of the weighted verifiers
#include <thread>

#include "launchers.h"   // every nbls_*_launch of the kernel files, declared once for both sides
#include "wide_exec.h"   // wide_step_supported
#include "aot.h"
#include <map>
#include <tuple>

using namespace nbls;
static_assert(P_COUNT <= NBLS_N_PROGRAMS, "nbls_timing_read's arrays (NBLS_N_PROGRAMS + 1 entries) must cover every step program");
static const size_t RAW = RAW_FP_BYTES;     // one raw field element in HBM scratch (14 limbs + padding)
static const size_t F12 = 12 * RAW;        // raw Fp12
static const size_t LINE_BYTES = (size_t)LINE_ELEMS * RAW;   // one line table: 68 triples of Fp2 as raw elements (26,112 B)
// pairs from which the Miller loop runs as LINES + ACC (see nbls_pairing_batch_dev).  Round 4 measured the two programs ahead from 4096 pairs on; on the round-5 / 6 build a 4096-pair call
// -- exactly one wavefront of the fused program (four items) on each of the 1024 SIMDs -- takes 2.19 ms fused against 2.32 ms split, 3072 pairs likewise, and from 4608 pairs on the split
// form wins (tools/ab_split_min.py, profiles/round6_ab_split_min.txt)
static const size_t SPLIT_MILLER_MIN = 4097;
static const size_t LINES_CHUNK = 131072;   // pairs whose line tables are in HBM at a time (3.4 GB of the 288); larger batches run chunk by chunk on the same stream

// ---- BEGIN scratch slots -----------------------------------------------------------------------------------------------------------------------------------
// The scratch pool of a context (nbls_ctx::sb, handed out by need()) is indexed by these names.  need() frees and reallocates a slot that has to grow, so chains that run side
// by side on different streams of one call must never share a slot, and no slot may be regrown under a kernel in flight.  This block is the whole map: who owns which slot, the
// slots every chain touches (the masks) and the chains that run concurrently (the static_asserts).  A new chain takes new enumerators in front of NSB, gets a mask, and is
// asserted against everything it runs beside.  The numbers are the indices into sb[]: they fix the order of allocation and are never reused for something else.
typedef unsigned __int128 SlotMask;   // one bit per slot
enum Slot {
  // the call's own stream, one pipeline at a time: hash-to-curve (field elements, exponentiation inputs, powers, points), the point sum's two halves, the ladder's points (its
  // digits in SB_WORK_C / SB_WORK_B when the caller brings none), the decoders and the MSM when they run alone (DEC_MAIN, MSM_MAIN)
  SB_WORK_A = 0, SB_WORK_B = 1, SB_WORK_C = 2, SB_WORK_D = 3,
  SB_NORM = 4, SB_NORM_INV = 5,   // norms of projective points and their inverses
  SB_POINT_ST = 6,                // statuses of the affine program that nobody reads (hash-to-curve)
  SB_MSGS = 7,                    // dev_expand: the message bytes; sign_points: the recoded keys, made on side2 beside the hash chain and read by the ladder after it
  SB_UNIFORM = 8,                 // expand_message_xmd output
  SB_STAGED = 9,                  // the one staged input block of verifyBatch and of the multi-verify calls
  SB_VB_PAIRS = 10,               // verifyBatch: pairs (g1 | g2), result, statuses; the two-stage route reads it between its stages, where the context lock is dropped
  SB_POW_TABLE = 11,              // run_pow's table when the caller passes none; hash-to-G2's
  SB_OFFS_DST = 12,               // dev_expand: offsets and domain-separation tag
  SB_CLEAR_S = 13,                // PointG2.clearCofactor's third array (dev_clear_g2 S)
  SB_KEYS_X = 14, SB_KEYS_R = 15, SB_KEYS_C = 16, SB_KEYS_POW = 17,   // DEC_KEYS: key decompression beside the hash chain (verifyBatch, the multi-verify calls)
  SB_SWU_STATE = 18, SB_SWU_POINTS = 19,                              // hash-to-G2: SWU state per message, the two points of a message
  // verify_multiple_pipeline (pipelines_multi_verify.cpp)
  SB_RLC_WEIGHTS = 20,
  SB_RLC_PAIRS = 21,              // the decoded points, the pairs and what is read back
  SB_RLC_PER_SET = 22,            // per-set pass: the interleaved pairs, the n final exponentiations and the verdict bytes
  SB_RLC_KEYS_PROJ = 23, SB_RLC_KEYS_NORM = 24, SB_RLC_KEYS_INV = 25,   // the ladder's projective points (+ the affine program's unused statuses), norms and their inverses
  SB_SIGS_X = 26, SB_SIGS_R = 27, SB_SIGS_C = 28, SB_SIGS_POW = 29,     // DEC_SIGS: signature decompression
  SB_RLC_MSM = 30,                // MSM_RLC: 30 .. 39, 41 and 43 (MsmSlots::Buf); 40 and 42 are unused
  SB_AGG_DECODED = 44, SB_AGG_POINTS = 45, SB_AGG_LABELS = 46, SB_AGG_SUMS = 47,   // SEG_AGG: the per-set key sums of nbls_verify_aggregates (+ the decoded keys in front of them)
  SB_GRP_POINTS = 48, SB_GRP_LABELS = 49, SB_GRP_SUMS = 50,                        // SEG_GRP: the per-message key sums of the shared-message forms
  // combine_pipeline (pipelines_threshold.cpp): the decoded shares and their statuses | identifiers and coefficients in Montgomery form, groups, flags, the canonical
  // coefficients | the affine sums, what is read back | SEG_THR: one sum per group
  SB_THR_SHARES = 51, SB_THR_SCALARS = 52, SB_THR_OUT = 53, SB_THR_POINTS = 54, SB_THR_LABELS = 55, SB_THR_SUMS = 56,
  // poly_pipeline (pipelines_poly.cpp): the decoded coefficients, their statuses and raw projective forms | groups, ranks, first bad positions, the group of every identifier |
  // one slab: accumulators, norms, inverses, affine points, zero flags | one slab: the step's coefficient of every item | the compressed results and statuses (what is read back)
  SB_POLY_COEFS = 57, SB_POLY_LABELS = 58, SB_POLY_ACC = 59, SB_POLY_STEP = 60, SB_POLY_OUT = 61,
  // msm_batch_pipeline (pipelines_msm.cpp), both sized once per call before its first launch: the staged input, the converted points, the split scalars and what is read
  // back | one slab: keys, sorted points, buckets, bit-slices, accumulators.  (Two slots, carved by the pipeline.)
  SB_MSMB_CALL = 62, SB_MSMB_SLAB = 63,
  // kzg_pipeline (pipelines_kzg.cpp): the decoded commitments and proofs (+ the generator), their statuses | weights, the scalars of the MSMs, the products r_i y_i, the
  // values y_i and statuses of the blob evaluation, the challenges | [tau]G2 and -G2, their two line tables, the two combined points, the three parts of B | what is read back | everything of the per-item pass
  SB_KZG_POINTS = 64, SB_KZG_SCALARS = 65, SB_KZG_PAIRS = 66, SB_KZG_OUT = 67, SB_KZG_ITEMS = 68,
  // kzg_prove_pipeline and nbls_fr_quotient_roots (pipelines_kzg_prove.cpp): the quotient rows (the MSM's scalars), the challenges, the values y_i and the statuses of the two
  // canonical checks | the affine sums and their zero flags, then what is read back (compressed points, values, statuses)
  SB_KZGP_SCALARS = 69, SB_KZGP_OUT = 70,
  // cells_pipeline and nbls_fr_ntt (pipelines_kzg_cells.cpp): the coefficients of every blob and the blobs' statuses | one chunk's quotient rows (the MSM's scalars) and the
  // rows' statuses | what is read back (transformed rows or cells, compressed proofs, statuses), then one chunk's affine sums, zero flags and closing statuses
  SB_KZGC_COEFS = 71, SB_KZGC_ROWS = 72, SB_KZGC_OUT = 73,
  // verify_cells_pipeline (pipelines_kzg_verify_cells.cpp): the decoded commitments and proofs, the gathered commitments, their statuses | weights, the scalars of the MSMs,
  // the partial rows and the row of the -S_i, the statuses before the elements are looked at | [tau^c]G2 and -G2, their two line tables, the two combined points, the three
  // parts of B | what is read back | everything of the per-cell pass (the rows of the batched MSM in front)
  SB_KZGV_POINTS = 74, SB_KZGV_SCALARS = 75, SB_KZGV_PAIRS = 76, SB_KZGV_OUT = 77, SB_KZGV_ITEMS = 78,
  // cells_pipeline's recovery front end (nbls_kzg_recover_cells*, pipelines_kzg_cells.cpp): per blob the 2 N / c values of the missing cells' vanishing polynomial and the
  // N / c inverses of its values on the coset of 7; the rest of the call is on cells_pipeline's slots (SB_KZGC_COEFS holds a half's coefficients, then the blob's)
  SB_KZGR_Z = 79,
  // cells_pipeline's FK20 proofs loop (nbls_kzg_*_cells_and_proofs_fk20, pipelines_kzg_cells.cpp): one chunk's scalars of pass A and the rows' statuses | one chunk's sums of
  // pass A in the converted projective form, the points of pass B.  They stand where the quotient rows (SB_KZGC_ROWS) stand in the other form
  SB_KZGF_SCALARS = 80, SB_KZGF_POINTS = 81,
  // groth16_pipeline, nbls_groth16_prepare_inputs and nbls_groth16_input_sums (pipelines_groth16.cpp): the proofs' points split, decoded and weighted, their statuses | weights,
  // the scalars of the MSM over the C_i, the partial rows and the m + 1 sums | the three combined points, the product's final exponentiation | what is read back | everything
  // of one chunk of the per-proof pass (L_i, the final exponentiations, the verdicts)
  SB_G16_POINTS = 82, SB_G16_SCALARS = 83, SB_G16_PAIRS = 84, SB_G16_OUT = 85, SB_G16_ITEMS = 86,
  // fr_ntt_large_dev (nbls_fr_ntt_large, nbls_fr_ntt_dev; pipelines_kzg_cells.cpp): one flag word per polynomial, cleared on the stream in front of the call's first launch,
  // then one element per polynomial: the inverse of the caller's shift on the way to the coefficients.  The host-buffer call stages on nbls_fr_ntt's slots (SB_STAGED, SB_KZGC_OUT)
  SB_NTTL_FLAGS = 87,
  NSB
};
static_assert(NSB == 88, "sb[] indices do not shift");
constexpr SlotMask slot_bit(int i) { return (SlotMask)1 << i; }
template <typename... S> constexpr SlotMask slots(S... s) { return (slot_bit(s) | ...); }
// one instance of dev_decompress: three arrays of field elements and the exponentiation table
struct DecSlots { Slot x, r, c, pow; constexpr SlotMask mask() const { return slots(x, r, c, pow); } };
constexpr DecSlots DEC_MAIN{SB_WORK_A, SB_WORK_B, SB_WORK_C, SB_POW_TABLE}, DEC_KEYS{SB_KEYS_X, SB_KEYS_R, SB_KEYS_C, SB_KEYS_POW}, DEC_SIGS{SB_SIGS_X, SB_SIGS_R, SB_SIGS_C, SB_SIGS_POW};
// one instance of dev_msm: its buffers at fixed distances from a base slot (the gaps keep MSM_MAIN off SB_VB_PAIRS and SB_OFFS_DST)
struct MsmSlots {
  enum Buf { POINTS = 0, SORTED = 1, WINDOW_SUMS = 2, KEYS = 3, NORM = 4, NORM_INV = 5, TEMP = 6, BUCKETS = 7, SLICES = 8, SLICES_HALF = 9, COUNTERS = 11, SPLIT_SCALARS = 13 };
  Slot base;
  constexpr Slot operator[](Buf b) const { return (Slot)(base + b); }
  constexpr SlotMask mask() const { return slots(POINTS, SORTED, WINDOW_SUMS, KEYS, NORM, NORM_INV, TEMP, BUCKETS, SLICES, SLICES_HALF, COUNTERS, SPLIT_SCALARS) << base; }
};
constexpr MsmSlots MSM_MAIN{SB_WORK_A}, MSM_RLC{SB_RLC_MSM};
// one instance of segment_sums (pipelines_multi_verify.cpp): gathered points | ids, ranks, pair lists, counters, statuses | sums, norms, inverses.  zero_with_sums: the zero
// flags of the sums lie behind the inverses (else behind the statuses): the two instances keep the layouts they were written with
struct SegSlots { Slot points, labels, sums; bool zero_with_sums; constexpr SlotMask mask() const { return slots(points, labels, sums); } };
constexpr SegSlots SEG_AGG{SB_AGG_POINTS, SB_AGG_LABELS, SB_AGG_SUMS, false}, SEG_GRP{SB_GRP_POINTS, SB_GRP_LABELS, SB_GRP_SUMS, true}, SEG_THR{SB_THR_POINTS, SB_THR_LABELS, SB_THR_SUMS, true};
// what every chain touches
constexpr SlotMask M_HASH_G2 = slots(SB_WORK_A, SB_WORK_B, SB_WORK_C, SB_WORK_D, SB_NORM, SB_NORM_INV, SB_POINT_ST, SB_POW_TABLE, SB_CLEAR_S, SB_SWU_STATE, SB_SWU_POINTS);   // dev_hash_to_g2
constexpr SlotMask M_LADDER = slots(SB_WORK_A, SB_WORK_B, SB_WORK_C, SB_NORM, SB_NORM_INV);                 // dev_point_mul
constexpr SlotMask M_VB_MAIN = slots(SB_VB_PAIRS, SB_UNIFORM) | M_HASH_G2;                                 // verify_stage / verify_pipeline on the call's stream (and its sub-batch streams)
constexpr SlotMask M_RLC_MAIN = slots(SB_STAGED, SB_UNIFORM, SB_RLC_WEIGHTS, SB_RLC_PAIRS, SB_RLC_PER_SET) | M_HASH_G2;   // verify_multiple_pipeline on the call's stream
constexpr SlotMask M_RLC_SIDE2 = DEC_KEYS.mask() | slots(SB_AGG_DECODED, SB_RLC_KEYS_PROJ, SB_RLC_KEYS_NORM, SB_RLC_KEYS_INV) | SEG_AGG.mask() | SEG_GRP.mask();   // its key chain
constexpr SlotMask M_RLC_SIDE = DEC_SIGS.mask() | MSM_RLC.mask();                                           // its signature chain
constexpr SlotMask M_THR_OWN = slots(SB_STAGED, SB_THR_SHARES, SB_THR_SCALARS, SB_THR_OUT) | SEG_THR.mask();   // combine_pipeline: what outlives the stages it calls
constexpr SlotMask M_POLY_OWN = slots(SB_STAGED, SB_POLY_COEFS, SB_POLY_LABELS, SB_POLY_ACC, SB_POLY_STEP, SB_POLY_OUT);   // poly_pipeline: what outlives the decoder it calls
constexpr SlotMask M_KZG_OWN = slots(SB_STAGED, SB_KZG_POINTS, SB_KZG_SCALARS, SB_KZG_PAIRS, SB_KZG_OUT, SB_KZG_ITEMS);   // kzg_pipeline: what outlives the decoder, the MSMs and the ladders it calls
constexpr SlotMask M_KZGP_OWN = slots(SB_STAGED, SB_KZGP_SCALARS, SB_KZGP_OUT);   // kzg_prove_pipeline: what outlives the batched MSM it calls (msm_rows_dev, on M_MSMB_OWN)
constexpr SlotMask M_KZGC_OWN = slots(SB_STAGED, SB_KZGC_COEFS, SB_KZGC_ROWS, SB_KZGC_OUT);   // cells_pipeline: what outlives the batched MSM of every chunk
constexpr SlotMask M_KZGR_OWN = M_KZGC_OWN | slots(SB_KZGR_Z);   // cells_pipeline behind the recovery front end: the Z values are read before the first chunk's MSM and not again
constexpr SlotMask M_KZGF_OWN = (M_KZGR_OWN & ~slot_bit(SB_KZGC_ROWS)) | slots(SB_KZGF_SCALARS, SB_KZGF_POINTS);   // cells_pipeline with the FK20 proofs loop, behind either front end: what outlives the two MSM passes of every chunk
constexpr SlotMask M_KZGV_OWN = slots(SB_STAGED, SB_KZGV_POINTS, SB_KZGV_SCALARS, SB_KZGV_PAIRS, SB_KZGV_OUT, SB_KZGV_ITEMS);   // verify_cells_pipeline: what outlives the decoder, the MSMs, the batched MSM and the ladder it calls
constexpr SlotMask M_MSMB_OWN = slots(SB_MSMB_CALL, SB_MSMB_SLAB);   // msm_batch_pipeline: what outlives the dev_msm calls of its big groups
// what runs side by side
static_assert(!(M_VB_MAIN & DEC_KEYS.mask()), "verifyBatch decodes its keys (side2, or the sub-batch's own stream) beside the hash chain");
static_assert(!(M_RLC_MAIN & M_RLC_SIDE2) && !(M_RLC_MAIN & M_RLC_SIDE) && !(M_RLC_SIDE & M_RLC_SIDE2), "verify_multiple_pipeline: the chains on s, side and side2 run side by side");
static_assert(!(SEG_AGG.mask() & SEG_GRP.mask()), "the per-message sums follow the per-set sums on side2 with nothing regrown under a kernel in flight");
static_assert(!(slot_bit(SB_MSGS) & (M_HASH_G2 | M_LADDER)), "sign_points: the keys are recoded on side2 beside the hash chain, and the digits outlive it until the ladder has read them");
static_assert(!(slot_bit(SB_VB_PAIRS) & MSM_MAIN.mask()), "verifyBatch keeps its pairs across the calls of its two-stage route: dev_msm on the main slots must not regrow them");
static_assert(!(M_THR_OWN & (DEC_MAIN.mask() | M_LADDER)), "combine_pipeline: the decoder and the ladder regrow their own slots between the stages that read the shares and the coefficients");
static_assert(!(M_POLY_OWN & DEC_MAIN.mask()), "poly_pipeline: the decoder regrows its own slots while the staged coefficients and the decoded points are held");
static_assert(!((M_POLY_OWN & ~slot_bit(SB_STAGED)) & (M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | M_LADDER | MSM_MAIN.mask())),
              "poly_pipeline keeps to slots of its own: no other chain's buffers are regrown or overwritten by it");
static_assert(!(M_MSMB_OWN & (MSM_MAIN.mask() | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | M_LADDER)),
              "msm_batch_pipeline: its big groups run through dev_msm on the main slots between its slabs, which must regrow nothing the call still holds");
static_assert(!(M_KZG_OWN & (DEC_MAIN.mask() | MSM_RLC.mask() | M_LADDER)), "kzg_pipeline: the decoder, the MSMs (on the slots of MSM_RLC: MSM_MAIN holds SB_STAGED) and the ladders of the per-item pass regrow their slots while the call holds its own");
static_assert(!((M_KZG_OWN & ~slot_bit(SB_STAGED)) & (M_MSMB_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | MSM_MAIN.mask())), "kzg_pipeline keeps to slots of its own");
static_assert(!(M_KZGP_OWN & (M_MSMB_OWN | DEC_MAIN.mask())), "kzg_prove_pipeline: the batched MSM sizes its two slots while the staged blobs and the quotient rows are held; nbls_kzg_setup_create decodes on the main slots");
static_assert(!((M_KZGP_OWN & ~slot_bit(SB_STAGED)) & (M_KZG_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | M_LADDER | MSM_MAIN.mask() | MSM_RLC.mask())),
              "kzg_prove_pipeline keeps to slots of its own");
static_assert(!(M_KZGC_OWN & (M_MSMB_OWN | DEC_MAIN.mask())), "cells_pipeline: the batched MSM runs chunk after chunk while the staged blobs, the coefficients and the results are held; nbls_kzg_monomial_create decodes on the main slots");
static_assert(!((M_KZGC_OWN & ~slot_bit(SB_STAGED)) & (M_KZGP_OWN | M_KZG_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | M_LADDER | MSM_MAIN.mask() | MSM_RLC.mask())),
              "cells_pipeline keeps to slots of its own");
static_assert(!(M_KZGR_OWN & (M_MSMB_OWN | DEC_MAIN.mask())), "the recovery front end of cells_pipeline: as cells_pipeline, whose chunks it runs");
static_assert(!(slot_bit(SB_KZGR_Z) & (M_KZGC_OWN | M_KZGV_OWN | M_KZGP_OWN | M_KZG_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | M_LADDER | MSM_MAIN.mask() | MSM_RLC.mask())),
              "the recovery front end keeps to a slot of its own");
static_assert(!(M_KZGF_OWN & (M_MSMB_OWN | DEC_MAIN.mask())), "the FK20 proofs loop: both passes run on the batched MSM's two slots, chunk after chunk, while the scalars of pass A and the points of pass B are held");
static_assert(!(slots(SB_KZGF_SCALARS, SB_KZGF_POINTS) & (M_KZGR_OWN | M_KZGV_OWN | M_KZGP_OWN | M_KZG_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | M_LADDER | MSM_MAIN.mask() | MSM_RLC.mask())),
              "the FK20 proofs loop keeps to slots of its own");
static_assert(!(M_KZGV_OWN & (DEC_MAIN.mask() | MSM_RLC.mask() | M_LADDER | M_MSMB_OWN)),
              "verify_cells_pipeline: the decoder, the MSMs (on the slots of MSM_RLC: MSM_MAIN holds SB_STAGED), the batched MSM and the ladder of the per-cell pass regrow their slots while the call holds the staged block and its own");
static_assert(!((M_KZGV_OWN & ~slot_bit(SB_STAGED)) & (M_KZGC_OWN | M_KZGP_OWN | M_KZG_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | MSM_MAIN.mask())),
              "verify_cells_pipeline keeps to slots of its own");
constexpr SlotMask M_G16_OWN = slots(SB_STAGED, SB_G16_POINTS, SB_G16_SCALARS, SB_G16_PAIRS, SB_G16_OUT, SB_G16_ITEMS);   // groth16_pipeline: what outlives the decoders, the ladders, the MSMs and the batched MSM it calls
static_assert(!(M_G16_OWN & (DEC_MAIN.mask() | MSM_RLC.mask() | M_LADDER | M_MSMB_OWN)),
              "groth16_pipeline: the decoders, the MSMs (on the slots of MSM_RLC: MSM_MAIN holds SB_STAGED), the ladder and the batched MSM of the per-proof pass regrow their slots while the call holds the staged block and its own");
static_assert(!((M_G16_OWN & ~slot_bit(SB_STAGED)) & (M_KZGV_OWN | M_KZGF_OWN | M_KZGR_OWN | M_KZGC_OWN | M_KZGP_OWN | M_KZG_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | MSM_MAIN.mask())),
              "groth16_pipeline keeps to slots of its own");
constexpr SlotMask M_NTTL_OWN = slots(SB_STAGED, SB_KZGC_OUT, SB_NTTL_FLAGS);   // nbls_fr_ntt_large: nbls_fr_ntt's staging and the flags; nbls_fr_ntt_dev touches the flags only
static_assert(!(slot_bit(SB_NTTL_FLAGS) & (M_G16_OWN | M_KZGV_OWN | M_KZGF_OWN | M_KZGR_OWN | M_KZGC_OWN | M_KZGP_OWN | M_KZG_OWN | M_POLY_OWN | M_THR_OWN | M_RLC_MAIN | M_RLC_SIDE | M_RLC_SIDE2 | M_VB_MAIN | M_LADDER | M_MSMB_OWN | MSM_MAIN.mask() | MSM_RLC.mask())),
              "the large transform keeps its flags on a slot of its own: a device-resident call leaves them in flight behind it");
// ---- END scratch slots -------------------------------------------------------------------------------------------------------------------------------------
#define EXPORT extern "C" __attribute__((visibility("default")))
extern std::recursive_mutex g_null_mu;   // locked in place of a context's mutex when the caller passed no context (the call then fails with NBLS_EINVAL)

static const size_t EXPC_MIN_DEFAULT = (size_t)1 << 40;   // items from which the cyclotomic exponentiations run with compressed squarings (expx below): never, unless asked for
struct DevProgram {
  Step* steps = nullptr; u32* descs = nullptr; u32* consts = nullptr;
  const Program* p = nullptr;
  bool wide_ok = false;   // every step is one the one-limb-per-lane interpreter implements (wide_exec.h): launches of at most ctx->wide_max items run on nbls_vm_kernel_wide
  // ahead-of-time kernel of this program (aot.h) and the translated program, when every step's signature is in the kernel's table
  int aot = -1; AotStep* aot_steps = nullptr; u32* aot_descs = nullptr; u32 aot_lds = 0;
  mutable unsigned long long launches = 0;   // launches of this program in this context (run_dev, run_chain): nbls_extra_program_launches tells a test WHICH line program a call took
};

size_t ls_max();      // defaults of the lane-split thresholds (NBLS_LS_MAX / NBLS_LS2_MAX), tuning.cpp
size_t ls2_max();
struct nbls_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::recursive_mutex mu;   // held for the whole of every exported call (host-level calls re-enter it through the *_dev entry points)
  DevProgram prog[P_COUNT];
  std::vector<uint8_t> dst_host; uint8_t* dst_dev = nullptr;   // hash-to-curve domain-separation tag last used by nbls_verify_batch_msgs_dev, and its device copy
  std::map<std::tuple<int, int, int, int>, DevProgram> tower;   // single tower operations (nbls_tower_op_batch), uploaded on first use
  DevProgram extra[XP_COUNT];   // the programs outside ProgId (programs.h ExtraProg), uploaded on first use with their ahead-of-time kernels
  size_t poly_slab = 0;         // nbls_set_tuning(NBLS_TUNE_POLY_SLAB): identifiers per slab of nbls_g*_poly_eval; 0 = the default (pipelines_poly.cpp)
  // nbls_set_tuning(NBLS_TUNE_MSMB_WINDOW / _BIG / _SLAB): the batched MSM's window width, the points from which a group runs through dev_msm, the entries of a slab; 0 = automatic /
  // the defaults (pipelines_msm.cpp)
  size_t msmb_window = 0, msmb_big = 0, msmb_slab = 0;
  size_t cells_chunk = 0;       // nbls_set_tuning(NBLS_TUNE_CELLS_CHUNK): blobs per pass of nbls_kzg_compute_cells_and_proofs; 0 = as many as the batched MSM takes (pipelines_kzg_cells.cpp)
  // nbls_set_tuning(NBLS_TUNE_NTT_TAIL_BITS / _PASS_BITS): the log size of the tails of nbls_fr_ntt_large / nbls_fr_ntt_dev and the global stages a launch runs at most; 0 = the defaults (pipelines_kzg_cells.cpp)
  unsigned ntt_tail_bits = 0, ntt_pass_bits = 0;
  size_t g16_chunk = 0;         // nbls_set_tuning(NBLS_TUNE_G16_CHUNK): proofs per pass of the per-proof pass of nbls_groth16_verify and of nbls_groth16_prepare_inputs; 0 = as many as the batched MSM takes (pipelines_groth16.cpp)
  size_t g16p_row_wave = 0;     // nbls_set_tuning(NBLS_TUNE_G16P_ROW_WAVE): matrix entries from which nbls_groth16_prove sums a row by a whole wavefront; 0 = the default (g16p_exec.h)
  // scratch (device)
  uint8_t *F = nullptr, *N = nullptr, *NI = nullptr, *io_g1 = nullptr, *io_g2 = nullptr, *io_f12 = nullptr, *one12 = nullptr;
  uint8_t* T[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // t1..t7 of the final exponentiation, raw Fp12
  // general scratch pool for the codec / hash / sum pipelines (grown on demand)
  uint8_t* sb[NSB] = {nullptr}; size_t sb_cap[NSB] = {0};
  // staging buffers of the host-buffer entry points (HostIO): kept between calls -- a hipMalloc / hipFree pair per buffer and call cost more than the copies at small batches
  struct IoBlock { void* p; size_t cap; bool busy; }; std::vector<IoBlock> io_pool; size_t io_pool_bytes = 0;
  uint8_t* nib[4] = {nullptr, nullptr, nullptr, nullptr}; int nnib[4] = {0, 0, 0, 0};   // op lists (pow_exec.h) of the exponents (p+1)/4, (p^2+7)/16, (p^2-9)/16, (p-3)/4 and their lengths in ops
  uint8_t* neg_g1 = nullptr;    // -G1 generator, affine wire bytes (verify: e(-G, S))
  uint8_t* gen_g1 = nullptr;    // G1 generator, affine wire bytes (getPublicKey)
  uint8_t* g1_fixed = nullptr;  // fixed-base table of the generator (curve.h pt_mul_fixed_g1): raw projective multiples [d 2^(WIN w)]G, built on first use by the ladder
  // side stream for the one-element chains of verifyBatch (signature decompression: a 758-bit Fp2 exponentiation on a single
  // lane is ~4 ms of pure latency) so that they overlap the batch-wide kernels instead of serialising with them
  hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; uint8_t* side_scratch = nullptr;
  // large pairing batches run as two halves on two streams (nbls_pairing_batch_dev; each half is told its Window): second stream, events
  hipStream_t half_stream = nullptr; hipEvent_t ev_half_fork = nullptr, ev_half_join = nullptr;
  // pairs from which a call runs as two halves on two streams.  16,384 since the end of round 6 (8192 before): on today's kernels one stream is faster up to 15,360 pairs
  // (10,240: 3.91 against 4.73 ms; 12,800 - 15,360: 5.05 - 5.24 against 5.67 - 5.9), the halves from 16,384 (6.1 against 6.45; profiles/round6_ab_halves.txt)
  size_t halves_min = env_long("NBLS_HALVES_MIN", 16384) > 0 ? (size_t)env_long("NBLS_HALVES_MIN", 16384) : (size_t)-1;   // NBLS_HALVES_MIN=0: never (profiles of kernels running alone)
  // verifyBatch as a software pipeline (round 5, verify_pipeline): events of the chunks (two each), the "xmd met non-monotonic offsets" flag lives behind the statuses
  std::vector<hipEvent_t> pipe_ev; hipEvent_t ev_pipe_done = nullptr; std::vector<hipStream_t> pipe_streams;
  // nbls_set_tuning(NBLS_TUNE_VERIFY_*)
  long verify_chunks = env_long("NBLS_VERIFY_CHUNKS", 2), verify_last_pct = env_long("NBLS_VERIFY_LAST_PCT", 25), verify_pipe_min = env_long("NBLS_VERIFY_PIPE_MIN", 32768);
  hipStream_t side2 = nullptr; hipEvent_t ev_join2 = nullptr;   // verifyBatch: key decoding runs beside message hashing (their exponentiation kernels are latency-bound and leave issue slots free)
  uint8_t* ident_g1 = nullptr; uint8_t* ident_g2 = nullptr;   // projective identity (0 : 1 : 0), raw
  size_t cap_F = 0, cap_io = 0;
  size_t split_min = SPLIT_MILLER_MIN;   // nbls_set_tuning(NBLS_TUNE_SPLIT_MILLER_MIN)
  // pairs per product call from which eight line tables share an accumulator (below: four).  Measured (tools/ab_acc8.sh): at 65,537 pairs the halves have 4096 groups of eight = 820
  // wavefronts, less than one per SIMD, and the call is slower (24.5 against 23.4 ms); at 2^18 terms 33.2 against 33.8 ms
  // (round 6, on the kernels as they are now: four per accumulator is faster at 2^17 and 2^18 terms as well -- 16.35 against 16.89 ms, 30.9 against 32.2 ms: never by default)
  size_t acc8_min = (size_t)env_long("NBLS_ACC8_MIN", (long)1 << 40);
  // cyclotomic exponentiation with compressed squarings (expx): scratch per item -- compressed powers, decompression scratch, redo flags and list -- and two redo counters (one per half)
  uint8_t *KS = nullptr, *KD = nullptr, *Kflag = nullptr; uint32_t *Klist = nullptr, *Kcount = nullptr;
  size_t expc_min = (size_t)env_long("NBLS_EXPC_MIN", (long)EXPC_MIN_DEFAULT);   // nbls_set_tuning(NBLS_TUNE_EXPC_MIN)
  // nbls_set_tuning(NBLS_TUNE_PT_LS2_MAX): items up to which the G2 point chains run in their two-lane forms (pt_ls2_variant)
  size_t pt_ls2_max = (size_t)env_long("NBLS_PT_LS2_MAX", 4096);
  size_t sac_max = (size_t)env_long("NBLS_G2_SAC_MAX", 6144);                   // nbls_set_tuning(NBLS_TUNE_SAC_MAX): keys up to which sign's ladder is the sign-aligned form (dev_point_mul)
  // round 6: launches of at most wide_max items run the programs that allow it on the one-limb-per-lane interpreter (vm_wide_kernel.hip: one item per workgroup of ceil(W / 4)
  // wavefronts, the Montgomery reduction spread over a row of lanes, two barriers per step) -- the multi-wavefront item form the round-5 review asked for.  Built, bit-exact
  // (tests/test_wide_sim.py, test_gpu_pairing.py::test_one_limb_per_lane_forms) and MEASURED SLOWER than the four-lane forms: the five exponentiations of one final exponentiation
  // take 0.93 ms against 0.66 ms (tools/wide_time.py, profiles/round6_wide_time.txt).  A step is 350 instructions in its rows + ~190 around them where the four-lane form has 660,
  // but every one of them waits for its predecessor (one column per lane: no independent work), and a lone wavefront then pays ~9-11 clocks per instruction instead of ~5.  Off by
  // default: NBLS_WIDE_MAX / NBLS_TUNE_WIDE_MAX (items; 0 = never), NBLS_WIDE_PROGS = 0: only the final exponentiation's programs.  The fixed-exponent powers, where the same
  // idea removes a 196-multiply-add reduction per squaring from ONE lane, are the case that pays (pow_wide.h: 0.7 -> 0.3 ms).
  size_t wide_max = (size_t)env_long("NBLS_WIDE_MAX", 0);
  // round 6: messages from which hash-to-G2 takes its SWU square root by the norm method (two Fp exponentiations, programs P_H2C_NA / NM / NB) instead of one Fp2 exponentiation;
  // nbls_set_tuning(NBLS_TUNE_H2C_NORM_MIN); 0 = always.  Less work (1.96 against 2.53 ms of exponentiation kernels per 65,536 roots) but two dependent exponentiations where
  // there was one: a launch that does not fill the device pays their latency twice (sign of 8192 keys +0.09 ms), one that does, or that runs beside other work as the sub-batches
  // of verifyBatch do (the size counted there is the whole call's), gains (sign of 65,536 keys -0.7 ms, verifyBatch -0.3 ms alone and -0.5 ms with three calls in flight)
  size_t h2c_norm_min = (size_t)env_long("NBLS_H2C_NORM_MIN", 32768);
  // round 6: elements up to which an inversion launch runs with one limb per lane (fp_inv_wide.h; nbls_set_tuning(NBLS_TUNE_INV_WIDE_MAX)).  The form shortens ONE call (a 4096-pairing
  // call 2.19 -> 2.165 ms, one verify 2.76 -> 2.67 ms) at eight times the instructions per element: contexts that are kept busy side by side (nbls_pool_init) lower it to 256
  // (twelve 4096-pairing calls in flight: 3.03 M pairings/s against 2.97 M with 4096)
  size_t inv_wide_max = (size_t)env_long("NBLS_INV_WIDE_MAX", 4096);
  // items up to which the pairing programs run in their four-lane / two-lane forms (tuning.cpp ls_variant; nbls_set_tuning(NBLS_TUNE_LS_MAX / _LS2_MAX)).  Latency forms as well:
  // shorter for ONE call, up to four times the instructions per item -- nbls_pool_init sets both to 0 on its contexts (twelve 1024-pairing calls in flight: 1.52 -> 1.95 M pairings/s)
  size_t ls_max = ::ls_max(), ls2_max = ::ls2_max();
  size_t chain_max = (size_t)env_long("NBLS_CHAIN_MAX", 8192);                  // nbls_set_tuning(NBLS_TUNE_CHAIN_MAX); see run_chain
  // nbls_set_tuning(NBLS_TUNE_FE_TAIL_CHAIN): which short programs of a final exponentiation that runs launch by launch end inside the launch of the exponentiation before
  // them (final_exp_pipeline: bit 0 the final product, bit 1 FE_MID1 / FE_MID2).  0 for a single context, whose chained middle is one launch already; nbls_pool_init sets it
  unsigned fe_tail_chain = fe_tail_chain_default(0);
  // nbls_set_tuning(NBLS_TUNE_FE_HEAD_CHAIN): such a final exponentiation runs the easy part at the head of the first exponentiation's launch (XP_FE_EASY12) instead of as a
  // launch of P_FE_EASY; nbls_set_tuning(NBLS_TUNE_INV_PRIO): issue priority 0 .. 3 of the wavefronts of nbls_fp_inv_kernel (run_inv_buf).  0 for a single context; nbls_pool_init sets them
  unsigned fe_head_chain = fe_head_chain_default(0), inv_prio = inv_prio_default(0);
  unsigned long long chain_launches = 0;   // launches that ran more than one program (run_chain's fused path), nbls_chain_launches: a test tells a chain from its fallback by it
  u32* qp_table = nullptr;      // multiples of p for the weak reduction (vm_exec.h weak_reduce), device copy
  // kzg_table (kzg_common.cpp): the device tables of kzg_kernels.hip, Montgomery form, 32 bytes an entry, built on first use and freed with the context.  [k]: the 2^k roots of unity in bit-reversed order;
  // [13 + k]: the same for 1 / omega, what nbls_fr_ntt's stages towards the coefficients divide by; [26 + 7 log2_n + log2_cell]: the 2 N / c inverse shifts 1 / h_k of the cells that nbls_kzg_verify_cells interpolates
  uint8_t* kzg_tables[26 + 13 * 7] = {nullptr};
  uint8_t* unit_lines = nullptr;   // a line table whose 68 lines are all 1 (c0 = 1, c1 = c2 = 0): the neutral partner of an odd last pair
  uint8_t* partial = nullptr;   // 576 bytes: the Fp12 partial of the *_partial entry points (multi-GPU reductions)
  uint8_t* L = nullptr; size_t cap_L = 0;   // line tables of the Miller loop (LINE_BYTES each), at most LINES_CHUNK of them
  // the scratch above is shared by every call on this context: a call that uses another stream than its predecessor waits for it (StreamOrder)
  hipStream_t last_stream = nullptr; hipEvent_t ev_last = nullptr; bool ev_last_set = false;
  uint8_t* pinned_out = nullptr; size_t pinned_out_cap = 0;   // the same for the way back (a call's inputs may still be in flight from `pinned` when its outputs are copied)
  uint8_t* pinned = nullptr; size_t pinned_cap = 0;   // page-locked host staging of the host-buffer entry points that pack their inputs (ensure_pinned; nbls_sign_batch)
  int last_hip = 0;
  // optional per-kernel timing (HIP events on the launch stream); slot P_COUNT = inversion kernel
  bool timing = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> tev;
  std::vector<hipEvent_t> ev_pool;   // timing events are recycled (nbls_timing_read returns them here) instead of created per launch
};

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ctx->last_hip = (int)e_; return NBLS_EHIP; } } while (0)
// the same for the extern "C" *_launch wrappers of the .hip files, which return the launch's hipError_t as an int.  They read it with hipGetLastError(), which also CLEARS it: the
// code has to be taken from the wrapper's return value, a second hipGetLastError() at the call site yields 0
#define LAUNCHCHK(call) do { int e_ = (call); if (e_) { ctx->last_hip = e_; return NBLS_EHIP; } } while (0)

// A chain: several programs executed back to back by ONE launch (aot.h): every wavefront runs them in order for its own items, the values between them pass
// through the HBM scratch buffers the separate launches would use.  Falls back to one launch per program when some program is not on an ahead-of-time kernel,
// when the programs do not share a kernel / the lanes per item, or in checked mode (whose per-launch buffer checks live in run()).  (ChainLink: bufs.h)
// Calls on one context share its scratch buffers.  The mutex serialises the host side; on the device, work submitted to the
// SAME stream is ordered anyway, and a call that names a different stream than its predecessor is made to wait for it.
struct StreamOrder {
  nbls_ctx* ctx; hipStream_t s;
  StreamOrder(nbls_ctx* c, hipStream_t st) : ctx(c), s(st) {
    if (!ctx->ev_last) hipEventCreateWithFlags(&ctx->ev_last, hipEventDisableTiming);
    if (ctx->ev_last && ctx->ev_last_set && ctx->last_stream != s) hipStreamWaitEvent(s, ctx->ev_last, 0);
  }
  ~StreamOrder() { if (ctx->ev_last && hipEventRecord(ctx->ev_last, s) == hipSuccess) { ctx->ev_last_set = true; ctx->last_stream = s; } }
};

// A call that has forked work onto other streams of the context (the side streams of verifyBatch, the second half of a large pairing call) and then fails must not return while
// those streams still run: StreamOrder records the call's end on `s` only, and the next call would free, regrow or overwrite scratch the orphaned kernels use.
// Armed right after the fork; every error return in between synchronises the device, the success path disarms it.
// keys: device scratch that holds key material (the recoded digits of sign's ladder), zeroed behind that wait.  The pipelines that stage a block carry the rule in Staged (staging.h).
struct ForkGuard {
  bool armed = true; void* keys = nullptr; size_t key_bytes = 0;
  ~ForkGuard() { if (armed) { (void)hipDeviceSynchronize(); if (keys) (void)hipMemset(keys, 0, key_bytes); } }
};
// The part of a pairing call a function works on.  A call owns items [0, n) of the context's per-item scratch (F, N, NI, T[], L and the compressed-squaring scratch KS, KD,
// Kflag, Klist); a function given a Window and a count uses items [first, first + count) of those arrays and nothing else of them, and every other pointer it is given -- the
// caller's points and outputs, f_raw, in / out -- is bound as it stands: the caller has already moved it to the part's first item.  The default is the whole call.  Offsets, not
// pointers: ensure_scratch / ensure_expc_scratch may still allocate after a Window was made.
struct Window {
  size_t first = 0;      // first item of the part
  int half = 0;          // 0 or 1: which redo counter of the compressed-squaring form (Kcount[half]) the part uses
  bool beside = false;   // another part of the same call runs beside this one on a second stream: their launches fill each other's tails, so the final exponentiation's middle is NOT chained
};
// ---- host-buffer wrappers ------------------------------------------------------------------------------------
// The pipelines that pack all their inputs into ONE page-locked block, send it as one copy and read one block back do so through Staged (staging.h).  The per-array wrappers
// use HostIO: staging buffers on the device for one host-buffer call.  Round 5: taken from a pool the context keeps (best fit among the free blocks of at most four times the size; a miss
// allocates) and handed back when the call returns -- every such call ends with a stream synchronisation and holds the context's mutex throughout, so a block is never reused while
// the device still works on it.  The pool is capped (NBLS_IO_POOL_MB, default 1024): free blocks are released oldest first when it would grow past the cap.
// Round 6: a call that fails half way may leave copies or kernels in flight on its stream, so the destructor synchronises the stream before the blocks
// become free (on the success path the call has just synchronised: a query of an idle stream; nbls_sign_batch declares its Staged AFTER its HostIO, so an error
// return has waited for the whole device before this runs); buffers registered with secret() -- device copies of private keys -- are zeroed on the call's stream before its
// last synchronisation (wipe()), or here when the call did not get that far: the pool hands blocks to later, unrelated calls.  The host copy of such keys is Staged::secret's.
struct HostIO {
  nbls_ctx* ctx; std::vector<size_t> mine; hipStream_t s = nullptr; std::vector<std::pair<void*, size_t>> secrets; bool wiped = false;
  ~HostIO() {
    if (!mine.empty()) (void)hipStreamSynchronize(s ? s : ctx->stream);
    if (!wiped) for (auto& k : secrets) (void)hipMemset(k.first, 0, k.second);
    for (size_t i : mine) ctx->io_pool[i].busy = false;
  }
  void secret(void* p, size_t n) { if (p && n) secrets.push_back({p, n}); }
  // enqueue the zeroing of the key buffers behind the work that reads them (call it before the call's final synchronisation)
  int wipe(hipStream_t st) { for (auto& k : secrets) if (hipMemsetAsync(k.first, 0, k.second, st) != hipSuccess) return NBLS_EHIP; wiped = true; return NBLS_OK; }
  void* alloc(size_t n) {
    if (!n) n = 1;
    auto& pool = ctx->io_pool;
    size_t best = (size_t)-1;
    for (size_t i = 0; i < pool.size(); i++)
      if (!pool[i].busy && pool[i].p && pool[i].cap >= n && pool[i].cap / 4 <= n && (best == (size_t)-1 || pool[i].cap < pool[best].cap)) best = i;
    if (best != (size_t)-1) { pool[best].busy = true; mine.push_back(best); return pool[best].p; }
    static const size_t cap_bytes = (size_t)env_long("NBLS_IO_POOL_MB", 1024) << 20;
    const size_t cap = n + n / 8 + 256;
    for (size_t i = 0; i < pool.size() && ctx->io_pool_bytes + cap > cap_bytes; i++)
      if (!pool[i].busy && pool[i].p) { hipFree(pool[i].p); ctx->io_pool_bytes -= pool[i].cap; pool[i].p = nullptr; pool[i].cap = 0; }
    void* p = nullptr;
    if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    ctx->io_pool_bytes += cap;
    size_t slot = (size_t)-1;
    for (size_t i = 0; i < pool.size(); i++) if (!pool[i].p) { slot = i; break; }
    if (slot == (size_t)-1) { pool.push_back({nullptr, 0, false}); slot = pool.size() - 1; }
    pool[slot] = {p, cap, true};
    mine.push_back(slot);
    return p;
  }
};
// a host-buffer entry point: works on the context's stream, ordered behind the context's previous call like every other call (a device-resident call on a caller's stream returns
// with its work still queued, and the pipelines the host-buffer calls run -- dev_msm, dev_point_mul, dev_expand, ... -- use the same scratch slots)
#define LOCKED(ctx) std::lock_guard<std::recursive_mutex> g_((ctx)->mu); HIPCHK(hipSetDevice((ctx)->device)); hipStream_t s = (ctx)->stream; StreamOrder order_((ctx), s)
// the same for an entry point that works on device pointers and takes the caller's stream (NULL: the context's): `s` is that stream
static inline hipStream_t call_stream(nbls_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }
#define DEV_ENTER(ctx, stream) std::lock_guard<std::recursive_mutex> g_((ctx)->mu); HIPCHK(hipSetDevice((ctx)->device)); hipStream_t s = call_stream((ctx), (stream)); StreamOrder order_((ctx), s)
// first statement of an entry point that makes several locked calls: scratch and I/O staging buffers belong to it until it returns.  Stands in front of the argument check, so it
// has to survive a null context
#define WHOLE_CALL(ctx) std::lock_guard<std::recursive_mutex> whole_call_((ctx) ? (ctx)->mu : g_null_mu)

// ---- internal functions (hidden visibility; defined in runtime.cpp, tuning.cpp and the pipelines_*.cpp files)
struct VerifyIn;
int nbls_init_prio(int device_id, int prio, nbls_ctx** out);   // nbls_init with ctx->stream created at stream priority `prio` (0 = the default: what nbls_init passes)
int nbls_stream_priority(nbls_ctx* ctx, int* prio);            // hipStreamGetPriority of ctx->stream
int nbls_record_event(nbls_ctx* ctx, hipEvent_t ev);           // hipEventRecord(ev, ctx->stream): complete when everything enqueued on the context's stream so far is (the balanced pool's completion events; the stream itself stays inside the context)
bool checked_mode();
bool aot_enabled();
int upload_program(nbls_ctx* ctx, DevProgram& d, const Program& p, const int k);
int upload(nbls_ctx* ctx, ProgId id);
int upload_extra(nbls_ctx* ctx, ExtraProg id);
void free_program(DevProgram& d);
bool wide_applies(const nbls_ctx* ctx, const DevProgram& d, int id, size_t n);
hipEvent_t timing_event(nbls_ctx* ctx);
void aot_seg(AotSeg& g, const DevProgram& d, const IOBuf* bufs);
void kernel_args(KernelArgs& ka, const nbls_ctx* ctx, const DevProgram& d, size_t n);   // everything of a launch that comes from the program; buffers: bind_bufs (bufs.h)
int run_dev(nbls_ctx* ctx, const DevProgram& d, int id, size_t n, const BufList& bufs, hipStream_t s, const uint32_t* n_dev, const uint32_t* item_index);
int run(nbls_ctx* ctx, ProgId id, size_t n, const BufList& bufs, hipStream_t s, const uint32_t* n_dev = nullptr, const uint32_t* item_index = nullptr);
int run_inv(nbls_ctx* ctx, size_t n, const void* in, void* out, hipStream_t s);   // run_inv_buf, booked in the timing slot of the inversion kernel (P_COUNT)
bool chains_enabled();
int run_chain(nbls_ctx* ctx, size_t n, const ChainLink* links, size_t count, hipStream_t s);
int ensure_scratch(nbls_ctx* ctx, size_t n);
int ensure_expc_scratch(nbls_ctx* ctx);
int ensure_io(nbls_ctx* ctx, size_t n);
int ensure_lines(nbls_ctx* ctx, size_t n);
int need(nbls_ctx* ctx, Slot i, size_t bytes, uint8_t** out);
int ensure_fork_event(nbls_ctx* ctx);
int ensure_side(nbls_ctx* ctx);
int ensure_side2(nbls_ctx* ctx);
int ensure_half_stream(nbls_ctx* ctx);
int ensure_pinned(nbls_ctx* ctx, size_t bytes);
int ensure_pinned_out(nbls_ctx* ctx, size_t bytes);
size_t pow_wide_max();
int run_pow(nbls_ctx* ctx, int which, size_t n, const void* in, void* out, hipStream_t s, uint8_t* scratch = nullptr);
int run_inv_buf(nbls_ctx* ctx, size_t n, const void* in, void* out, hipStream_t s);
ProgId ls_variant(nbls_ctx* ctx, ProgId id, size_t n);
ProgId pt_ls2_variant(nbls_ctx* ctx, ProgId id, size_t n);
int reduce_product(nbls_ctx* ctx, size_t n, uint8_t** result, hipStream_t s);
int expx(nbls_ctx* ctx, const Window& w, size_t n, uint8_t* in, uint8_t* out, hipStream_t s);
int final_exp_pipeline(nbls_ctx* ctx, const Window& w, size_t n, uint8_t* f_raw, void* d_out, hipStream_t s);
int finish_single(nbls_ctx* ctx, const Window& w, uint8_t* f_raw, int final_exp, void* d_out, hipStream_t s);
int pairing_core(nbls_ctx* ctx, const Window& w, size_t n, const void* d_g1, const void* d_g2, int with_final_exp, void* d_out, hipStream_t s, bool two_programs);
int lines_acc(nbls_ctx* ctx, size_t c, const uint8_t* g1, const uint8_t* g2, uint8_t* L, size_t GR, uint8_t* acc_out, size_t h, hipStream_t s);
int miller_values(nbls_ctx* ctx, size_t n, const void* d_g1, const void* d_g2, size_t* m_out, hipStream_t s);
int acc_prepared(nbls_ctx* ctx, size_t n, const void* d_g1, const void* d_tables, size_t table_stride, hipStream_t s);
int partial_buffer(nbls_ctx* ctx, void* d_dst, uint8_t** dst);
int miller_product_partial_core(nbls_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, int validate, void* d_dst, void** d_partial, int8_t* status);
int dev_validate(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, void* d_status, hipStream_t s);
int dev_decompress(nbls_ctx* ctx, bool g2, size_t n, const void* d_in, void* d_out, void* d_status, hipStream_t s, const DecSlots& sl = DEC_MAIN, int mode = 0, size_t io = 0,
    size_t ntot = 0);
int dev_clear_g2(nbls_ctx* ctx, size_t n, void* in, uint8_t* base, uint8_t* S, void* out, void* N, hipStream_t s);
int dev_hash_to_g2(nbls_ctx* ctx, size_t n, const void* d_uniform, void* d_out, hipStream_t s, size_t io = 0, size_t ntot = 0, uint8_t** proj = nullptr);
int to_affine(nbls_ctx* ctx, bool g2, size_t n, const void* Pj, void* N, void* NI, void* d_out, void* d_status, hipStream_t s, bool norm = true);
int dev_point_sum(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, void* d_out, void* d_status, hipStream_t s);
int decompress_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* in, uint8_t* out, int8_t* status);
int dev_expand(nbls_ctx* ctx, size_t n, const uint8_t* msgs, const uint32_t* offs, const uint8_t* dst, size_t dst_len, uint8_t** d_uniform, hipStream_t s, unsigned len_in_bytes = 256);
int sum_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* pts, uint8_t* out, int8_t* status);
int dev_hash_to_g1(nbls_ctx* ctx, int count, size_t n, const void* d_uniform, void* d_out, hipStream_t s);
int dev_encode_to_g2(nbls_ctx* ctx, size_t n, const void* d_uniform, void* d_out, hipStream_t s);
int hash_curve_host(nbls_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* dst, size_t dst_len, uint8_t* out);
int compress_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* aff, uint8_t* out);
int decode_host(nbls_ctx* ctx, int kind /* 0 g1.fromHex, 1 g2.fromHex, 2 g2.fromSignature */, size_t n, const uint8_t* in, size_t len, uint8_t* out, int8_t* status);
int encode_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* aff, const int8_t* zero, int compressed, uint8_t* out);
int clear_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* aff, uint8_t* out, int8_t* status);
int dev_point_mul(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, size_t pt_stride, const void* d_scalars, void* d_out, void* d_status, hipStream_t s, bool allow_fixed = true,
    bool in_subgroup = false, uint8_t* recoded = nullptr, uint8_t** proj = nullptr);
bool g2_ladder_takes_projective(const nbls_ctx* ctx, size_t n);   // an in-subgroup G2 dev_point_mul of n items reads raw projective points (stride 6 * RAW), not affine ones
int ensure_g1_fixed(nbls_ctx* ctx, hipStream_t s);
int sign_points(nbls_ctx* ctx, size_t n, const void* d_uniform, void* h, const void* d_keys32, void* d_out192, void* d_status, hipStream_t s);
bool scalar_is_zero_mod_r(const uint8_t* k32);
int mul_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* pts, const uint8_t* scalars32, uint8_t* out, int8_t* status);
int dev_msm(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, const void* d_scalars, unsigned nbits, void* d_out, void* d_status, hipStream_t s, const MsmSlots& sl = MSM_MAIN);
int segmented_sum(nbls_ctx* ctx, bool g2, size_t count, const uint32_t* keys, const uint32_t* rank, uint32_t* list, uint32_t* counters, uint8_t* P, size_t maxrun, hipStream_t s);
// pipelines_multi_verify.cpp: one sum per contiguous segment as affine wire bytes; what the caller's closing status kernel reads comes back in SegSums
struct SegSums { const uint32_t* first; const int8_t* st; uint8_t* zero; };   // per segment: first position with a status >= 2; per position: status; per segment: the sum is the zero point
int segment_sums(nbls_ctx* ctx, bool g2, const SegSlots& sl, size_t count, size_t nseg, const uint32_t* d_off, const uint32_t* d_index, const uint8_t* src, const int8_t* st_src,
                 size_t maxseg, uint8_t* out, SegSums* o, hipStream_t s);
unsigned scalars_bit_length(size_t n, const uint8_t* k32);
// pipelines_msm.cpp, the batched sums: the plan of one call (window width, slabs of whole groups, the carving of a slab's block) and the device core of nbls_g1_msm_rows that the KZG prover
// feeds from device memory.  msm_rows_dev_plan sizes and takes SB_MSMB_CALL / SB_MSMB_SLAB: it comes with the caller's other need() calls, before anything is in flight.
// msm_rows_dev: n_rows sums of n_pts points each; conv_pts = the output of P_G1_MSM_PREP (2 x 3 raw elements per point), d_scalars = n_rows * n_pts scalars of 32 bytes in
// device memory, read as 256-bit values (the split path: they are never on the host for scalars_bit_length) -> affine sums (96 bytes each) and zero flags.  No group takes the
// dev_msm route, whatever NBLS_TUNE_MSMB_BIG says: there are no affine points to give it
static const size_t MSMB_MAX_ITEMS = (size_t)1 << 22, MSMB_MAX_GROUPS = (size_t)1 << 20;   // one pass of the batched MSM: scalars, rows (groups)
struct MsmbPart { size_t g0, g1; bool big; int key_bits; };   // groups [g0, g1): one slab (and the bits of its keys), or one big group
struct MsmbPlan {
  bool g2 = false, split = false; unsigned nbits = 0, dims = 1, kbits = 0, c = 0;
  size_t glen = 0, pt_block = 0, k_mod = 0;   // the wider map of the rows form (msm_map_dev_plan); glen = 0: the rows form itself, or offsets
  size_t n_groups = 0, n_pts = 0, nwin = 0, J = 0, jtop = 0, maxM = 0, max_ngs = 0, sort_bytes = 0, scan_bytes = 0;
  size_t s_cnt = 0, s_tmp = 0, s_P = 0, s_bk = 0, s_G = 0, s_Gh = 0, s_acc = 0, s_N = 0, s_NI = 0, slab_bytes = 0;
  std::vector<MsmbPart> parts;
  uint8_t *SL = nullptr, *Ks = nullptr;   // the slab's block; the split scalars
};
int msm_rows_dev_plan(nbls_ctx* ctx, size_t n_pts, size_t n_rows, MsmbPlan* pl);
int msm_rows_dev(nbls_ctx* ctx, const MsmbPlan& pl, const uint8_t* conv_pts, const uint8_t* d_scalars, uint8_t* d_out96, uint8_t* d_zero, hipStream_t s);
// the rows form with the group length, the point period and the scalars' period apart (pipelines_msm.cpp has the map): the passes of the FK20 cell proofs
int msm_map_dev_plan(nbls_ctx* ctx, size_t glen, size_t period, size_t pt_block, size_t k_mod, size_t n_groups, MsmbPlan* pl);
void msm_map_plans_settle(nbls_ctx* ctx, std::initializer_list<MsmbPlan*> plans);
int msm_map_dev(nbls_ctx* ctx, const MsmbPlan& pl, const uint8_t* conv_pts, const uint8_t* d_scalars, const uint8_t* split, uint8_t* d_out96, uint8_t* d_zero, uint8_t* conv, hipStream_t s);
int msm_split_scalars(nbls_ctx* ctx, size_t n, const uint8_t* d_scalars, uint8_t* split, hipStream_t s);
// ---- device handles (nbls_keyset, the KZG bases, nbls_kzg_fk20, nbls_groth16_vk): device memory of the device they were created on, usable from every context of that device.
// handle_free: a handle's device blocks freed on the handle's device, the caller's device restored.  handle_create: the frame of a create call behind its argument check -- the
// handle allocated, `device` set, build(h) run; where that fails the handle goes through its destroy function and *out stays NULL
static inline void handle_free(int device, std::initializer_list<void*> blocks) {
  int cur = 0;
  const bool restore = hipGetDevice(&cur) == hipSuccess;
  if (hipSetDevice(device) == hipSuccess) for (void* b : blocks) (void)hipFree(b);
  if (restore) (void)hipSetDevice(cur);
}
template <class H, class Build> static int handle_create(nbls_ctx* ctx, H** out, void (*destroy)(H*), Build build) {
  H* h = new (std::nothrow) H;
  if (!h) return NBLS_EHIP;
  h->device = ctx->device;
  const int r = build(h);
  if (r) { destroy(h); return r; }
  *out = h;
  return NBLS_OK;
}
// ---- KZG and the weighted verifiers (kzg_common.cpp): what pipelines_kzg.cpp, pipelines_kzg_prove.cpp, pipelines_kzg_cells.cpp and pipelines_kzg_verify_cells.cpp share, and
// the device helpers that pipelines_groth16.cpp and pipelines_multi_verify.cpp run as well
static const size_t KZG_MAX_ELEMS = (size_t)1 << 24;   // field elements per call of the Fr entry points and of the calls that take whole blobs
// -G2 in affine wire bytes (g2_wire_negate of the generator); the challenges of n blobs on host threads
const uint8_t* neg_g2_wire();
void blob_challenges(unsigned log2_n, size_t n, const uint8_t* blobs, const uint8_t* c48, uint8_t* z32);
// a context's device table, made on first use: the roots of 2^log2_n, the inverse roots (a permutation of the roots, made behind them on the same stream), or the inverse shifts
// of (log2_n, log2_cell); log2_cell is read for the last alone
enum KzgTable { KZG_ROOTS = 0, KZG_INV_ROOTS = 1, KZG_CELL_ISHIFTS = 2 };
int kzg_table(nbls_ctx* ctx, KzgTable kind, unsigned log2_n, unsigned log2_cell, hipStream_t s, const uint8_t** table);
// a basis of 2^log2_n points in the form the batched MSM reads (each point with its endomorphism image, raw projective).  The two public handles are types of their own, so
// that neither basis is taken for the other: nbls_kzg_setup holds a trusted setup's Lagrange basis, nbls_kzg_monomial the monomial basis [tau^i]G1
struct KzgBasis { int device = 0; unsigned log2_n = 0; uint8_t* pts = nullptr; };
struct nbls_kzg_setup : KzgBasis {};
struct nbls_kzg_monomial : KzgBasis {};
// the handle of the FK20 cell proofs (fr_exec.h has the identities): xhat = the c M fixed points X^[j][i] at index i c + j, in the converted form the batched MSM reads;
// bsplit = the M x M projection matrix B, row after row, split as msm_split_scalars leaves it (2 x 32 bytes an entry).  Both NULL where n' = N / c = 1: every proof is the zero point
struct nbls_kzg_fk20 { int device = 0; unsigned log2_n = 0, log2_cell = 0; uint8_t *xhat = nullptr, *bsplit = nullptr; };
// the prover's closing stage: pl.n_groups rows of scalars against the basis -> affine sums (aff96, zero) -> compressed to out48 -> closed by kzg_prove_tail_kernel with the
// statuses st_a, st_b (either may be NULL)
int kzg_proof_tail(nbls_ctx* ctx, const MsmbPlan& pl, const uint8_t* basis_pts, const uint8_t* rows, uint8_t* aff96, uint8_t* zero, const uint8_t* st_a, const uint8_t* st_b,
                   uint8_t* out48, uint8_t* status, hipStream_t s);
// what follows the sums in kzg_proof_tail, for a caller whose n affine sums and zero flags come from elsewhere (the second pass of the FK20 cell proofs)
int kzg_proof_close(nbls_ctx* ctx, size_t n, const uint8_t* aff96, const uint8_t* zero, const uint8_t* st_a, const uint8_t* st_b, uint8_t* out48, uint8_t* status, hipStream_t s);
// The device helpers of the weighted verifiers (verifier_frame.h has the header they write into).  Each is one fixed run of launches on `s`:
// sum3_affine: n sums of three affine parts (p3: 3 n points, part after part; st3: a status each, non-zero = the identity) -> raw projective (pj: 3 n points), the identity
//   where the status says so, two complete additions, affine again (out96) with a zero flag each; nn, ni: n norms and inverses
// combined_tail: the k combined points at pts96 with their zero flags (the generator for a zero point) against k line tables -> their Miller values behind the mm the caller has
//   left in ctx->F, product, final exponentiation (res576), *one = the result is one
// items_is_one: the cnt raw Fp12 values in ctx->F -> norms, one batched final exponentiation (e576: cnt x 576), v[i] = value i is one
// statuses_back: closes a per-item pass -- reads back the n final statuses at fs, disarms the pass's guard, copies them to the caller and sets *all_ok.  About that guard:
//   nothing is forked in a per-item pass, it is used for its wait alone.  fetch() has disarmed the staged block, and an error return between arming it and this call must not
//   leave the chain running on slots the next call regrows
int sum3_affine(nbls_ctx* ctx, size_t n, const uint8_t* p3, const uint8_t* st3, uint8_t* pj, uint8_t* nn, uint8_t* ni, uint8_t* out96, uint8_t* zero, hipStream_t s);
int combined_tail(nbls_ctx* ctx, size_t k, size_t mm, uint8_t* pts96, uint8_t* zero, const uint8_t* tables, uint8_t* res576, uint8_t* one, hipStream_t s);
int items_is_one(nbls_ctx* ctx, size_t cnt, uint8_t* e576, uint8_t* v, hipStream_t s);
int statuses_back(nbls_ctx* ctx, hipStream_t s, const uint8_t* fs, size_t n, ForkGuard& guard, int* all_ok, int8_t* status);
// The frame of a KZG verifier's call: the three staged parts [tau^c]G2 | -G2 | seed, the pairs block and the read-back block (verifier_frame.h has their formats), the opening
// launches, the combined check with its verdict and the per-item pass around the summands.  The caller keeps its staged inputs, its points and scalars blocks, its item
// kernels, the four sums that fill PT2 / A_ZERO, B3 and BST, and the three summands of every X_i (P3, ST3).  A call: rlc_seed (in front of DEV_ENTER) -> stage (among the caller's
// io.bytes) -> take (among its need() calls, in front of io.send) -> open (first launches; W: n weights) -> the caller's items and sums -> decide (*more: the statuses need the
// per-item pass) -> items_begin -> the caller's summands -> items_close
struct Staged;
struct KzgFrame {
  nbls_ctx* ctx; Staged& io; hipStream_t s; size_t n; Slot sb_pairs, sb_out, sb_items;
  size_t o_tau = 0, o_ng2 = 0, o_seed = 0; KzgPairs a; KzgItemTail t;
  uint8_t *PR = nullptr, *BK = nullptr, *TB = nullptr, *PT2 = nullptr, *A_ZERO = nullptr, *B3 = nullptr, *BST = nullptr, *PRE = nullptr, *TAIL = nullptr, *P3 = nullptr, *ST3 = nullptr;
  ForkGuard guard{false};   // armed by items_begin, disarmed by statuses_back
  KzgFrame(nbls_ctx* c, Staged& st, hipStream_t stream, size_t items, Slot pairs, Slot out, Slot per_item);
  void stage(const uint8_t* tau96, const uint8_t* seed);
  int take();
  int open(uint8_t* staged, uint8_t* W);
  int decide(int* all_ok, int8_t* status, bool* more);   // (*more is written on success alone)
  // front: the caller's own bytes in front of the tail's block (*FRONT); rows_plan (may be NULL): the plan of a batched MSM of n rows of row_pts points, taken behind the block
  int items_begin(size_t front, uint8_t** FRONT, MsmbPlan* rows_plan = nullptr, size_t row_pts = 0);
  int items_close(const uint8_t* proofs96, const uint8_t* proof_st, int* all_ok, int8_t* status);
};
// the verifying key of nbls_groth16_* (pipelines_groth16.cpp): one device block.  alpha96: alpha affine; g2neg: -beta, -gamma, -delta affine (3 x 192 wire bytes); tables: their
// three line tables; ic96: the m + 1 points IC_j affine; ic_conv: the same in the form the batched MSM reads (P_G1_MSM_PREP: 2 x 3 raw elements a point); ic0_proj: IC_0 raw projective
struct nbls_groth16_vk { int device = 0; size_t m = 0; uint8_t *mem = nullptr, *alpha96 = nullptr, *g2neg = nullptr, *tables = nullptr, *ic96 = nullptr, *ic_conv = nullptr, *ic0_proj = nullptr; };
int msm_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* pts, const uint8_t* scalars32, uint8_t* out, int8_t* status);
int dst_on_device(nbls_ctx* ctx, const uint8_t* dst, size_t* dst_len, hipStream_t s, uint8_t** dd);
std::vector<size_t> verify_plan(nbls_ctx* ctx, size_t n);
int pipe_event(nbls_ctx* ctx, size_t i, hipEvent_t* e);
int pipe_stream(nbls_ctx* ctx, size_t i, hipStream_t* st);
int verify_pipeline(nbls_ctx* ctx, size_t n, const VerifyIn& in, int final_exp, void* d_out, uint8_t* out, std::vector<int8_t>& st, int* bad_offsets, void* stream);
bool verify_pipe_enabled();
bool fp12_wire_is_one(const uint8_t* out);
int verify_statuses(const std::vector<int8_t>& st, size_t n, int* zero_flag, int8_t* pk_status);
int verify_decide(const std::vector<int8_t>& st, size_t n, const uint8_t* out, int* ok, int8_t* pk_status);
int verify_stage(nbls_ctx* ctx, size_t n, const void* d_sig96, const void* d_uniform, const void* d_pk48, std::vector<int8_t>& st, void* stream);
// a table of decoded keys (nbls_keyset_create): raw projective points, the identity stored for zero keys and keys that did not decode, and the decoder's status of every key
struct nbls_keyset { int device = 0; size_t n = 0; uint8_t* pts = nullptr; int8_t* st = nullptr; };
// the keys of nbls_verify_aggregates(_indexed): set j owns entries key_offsets[j] .. key_offsets[j + 1] of the call's compressed keys (MultiVerifyIn::pks48) or of key_index (into ks);
// nkeys and maxset are filled in by the argument check
struct AggKeys { const uint32_t* key_offsets = nullptr; const nbls_keyset* ks = nullptr; const uint32_t* key_index = nullptr; size_t nkeys = 0, maxset = 0; };
// the messages of the shared-message forms: msgs / offsets hold n_msgs messages, set i signs message msg_index[i]
struct MsgGroups { size_t n_msgs = 0; const uint32_t* msg_index = nullptr; };
// pipelines_multi_verify.cpp: what the six multi-verify entry points hand to their one pipeline.  agg == NULL: one key per set (pks48 = n keys); else the aggregate key of every
// set.  mg == NULL: one message per set
struct MultiVerifyIn {
  size_t n; const uint8_t *sigs96, *msgs; const uint32_t* offsets; const uint8_t* pks48; const AggKeys* agg; const MsgGroups* mg; const uint8_t* dst; size_t dst_len; const uint8_t* seed32;
};
int verify_multiple_pipeline(nbls_ctx* ctx, const MultiVerifyIn& in, int* all_ok, int8_t* status);
int os_seed(uint8_t* seed32);
int rlc_seed(const uint8_t* seed32, uint8_t* seed);   // the seed of a call's secret weights: the caller's, or one from the OS
int verify_batch_partial_core(nbls_ctx* ctx, size_t n, const uint8_t* sig96 /* or NULL */, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pk48,
                                     const uint8_t* dst, size_t dst_len, void* d_dst, void** d_partial, int* zero_flag, int8_t* pk_status);
#define NBLS_STAGING_CALL   // Staged / read_back use the context and the declarations above
#include "staging.h"
