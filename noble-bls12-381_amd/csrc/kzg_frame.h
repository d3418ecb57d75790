// kzg_frame.h -- what the two KZG verifiers (kzg_pipeline, verify_cells_pipeline) lay out the same way, as plain C++ with no HIP and no context (tests/c/kzg_frame_test.cpp
// runs it under the sanitizers): the carving of the "pairs" block and of the per-item tail's block, the header of what is read back, and the rule that turns that header into
// the combined check's verdict.  KzgFrame (nbls_internal.h, kzg_common.cpp) is the only user: no pipeline file names an offset or a byte position of these.
#pragma once
#include <cstddef>
#include <cstdint>
#include "programs.h"   // LINE_ELEMS; vm.h: RAW_FP_BYTES
namespace nbls {
// the next part of a device block that is carved into 64-byte aligned parts: its offset; *off moves past it
static size_t carve(size_t* off, size_t bytes) { const size_t o = *off; *off = o + ((bytes + 63) & ~(size_t)63); return o; }

// The pairs block: the G2 point and -G2 | their two line tables | the two combined points A, B | the product's final exponentiation | the three parts of B (affine) | their
// statuses | the same raw projective | B's norm and its inverse
struct KzgPairs { size_t g2, tb, pt2, res, b3, bst, bj, bn, bytes; };
static inline KzgPairs kzg_pairs_carve() {
  const size_t raw = RAW_FP_BYTES, line = (size_t)LINE_ELEMS * raw;
  KzgPairs a; size_t o = 0;
  a.g2 = carve(&o, 2 * 192); a.tb = carve(&o, 2 * line); a.pt2 = carve(&o, 2 * 96); a.res = carve(&o, 576); a.b3 = carve(&o, 3 * 96); a.bst = carve(&o, 3);
  a.bj = carve(&o, 3 * 3 * raw); a.bn = carve(&o, 2 * raw); a.bytes = o;
  return a;
}
// The per-item tail's buffers as offsets from the block's own start (*off: the caller's carving, moved past the block; returns where the block starts): the three summands of
// every X_i and their statuses | raw projective | norms, inverses | X_i | the final exponentiations | is one | X_i is zero | the final statuses
struct KzgItemTail { size_t p3, st3, proj, n, ni, x, e, v, xz, fs; };
static inline size_t kzg_item_tail_carve(size_t n, size_t* off, KzgItemTail* t) {
  const size_t raw = RAW_FP_BYTES, p = 3 * raw, start = *off;
  size_t o = 0;
  t->p3 = carve(&o, 3 * n * 96); t->st3 = carve(&o, 3 * n); t->proj = carve(&o, 3 * n * p); t->n = carve(&o, n * raw); t->ni = carve(&o, n * raw); t->x = carve(&o, n * 96);
  t->e = carve(&o, n * 576); t->v = carve(&o, n); t->xz = carve(&o, n); t->fs = carve(&o, n);
  *off = start + o;
  return start;
}
// What is read back: the product is one | A is the zero point | B is | the decoder status of the G2 point | (12 unused) | the n statuses before any pairing
static const size_t KZG_HDR_BYTES = 16;
static inline size_t kzg_back_bytes(size_t n) { return KZG_HDR_BYTES + n; }
static inline uint8_t* kzg_hdr_one(uint8_t* BK) { return BK; }
static inline uint8_t* kzg_hdr_a_zero(uint8_t* BK) { return BK + 1; }
static inline uint8_t* kzg_hdr_b_zero(uint8_t* BK) { return BK + 2; }
static inline uint8_t* kzg_hdr_g2_status(uint8_t* BK) { return BK + 3; }
static inline uint8_t* kzg_hdr_pre(uint8_t* BK) { return BK + KZG_HDR_BYTES; }
// The verdict of the combined check from the block as read back.  Zero points are valid: e(O, Q) = 1, so A = B = O accepts and exactly one of them zero rejects; otherwise the
// product decides.  Any status before the pairings rejects
enum KzgVerdict { KZG_REJECT = 0, KZG_ACCEPT = 1, KZG_BAD_G2 = 2 };
static inline KzgVerdict kzg_verdict(const uint8_t* got, size_t n) {
  if (got[3] != 0) return KZG_BAD_G2;   // the G2 point does not decode, or is the zero point
  const bool one = got[0] != 0, za = got[1] == 1, zb = got[2] == 1;
  bool clean = true;
  for (size_t i = 0; i < n && clean; i++) clean = got[KZG_HDR_BYTES + i] == 0;
  return clean && ((za && zb) || (!za && !zb && one)) ? KZG_ACCEPT : KZG_REJECT;
}
}  // namespace nbls
