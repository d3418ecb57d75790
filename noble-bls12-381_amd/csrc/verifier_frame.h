// verifier_frame.h -- what the weighted batch verifiers (kzg_pipeline, verify_cells_pipeline, groth16_pipeline) lay out the same way, as plain C++ with no HIP and no context
// (tests/c/verifier_frame_test.cpp runs it under the sanitizers): the carving of the KZG "pairs" block and of the per-item tail's block, the header of what is read back with
// each verifier's names for its bytes, the rules that turn that header into the combined check's verdict, and the negation of a G2 point in wire bytes.  The shared device
// helpers and KzgFrame (nbls_internal.h, kzg_common.cpp) and groth16_pipeline use these names: no pipeline file names an offset or a byte position of the header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
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
// What a verifier reads back behind its combined check: 16 header bytes, then the n statuses before any pairing.  Header: the product is one | three bytes of the verifier's own,
// the zero flags of its combined points first, in the order of the points (hdr_flags) | 12 unused.  A zero flag is the value 1 and nothing else (the to-affine program and the
// MSMs write 0 or 1)
static const size_t HDR_BYTES = 16;
static inline size_t back_bytes(size_t n) { return HDR_BYTES + n; }
static inline uint8_t* hdr_one(uint8_t* BK) { return BK; }
static inline uint8_t* hdr_flags(uint8_t* BK) { return BK + 1; }
static inline uint8_t* hdr_pre(uint8_t* BK) { return BK + HDR_BYTES; }
static inline bool hdr_clean(const uint8_t* got, size_t n) {
  bool clean = true;
  for (size_t i = 0; i < n && clean; i++) clean = got[HDR_BYTES + i] == 0;
  return clean;
}
// KZG: A is the zero point | B is | the decoder status of the G2 point
static inline uint8_t* kzg_hdr_a_zero(uint8_t* BK) { return hdr_flags(BK); }
static inline uint8_t* kzg_hdr_b_zero(uint8_t* BK) { return hdr_flags(BK) + 1; }
static inline uint8_t* kzg_hdr_g2_status(uint8_t* BK) { return BK + 3; }
// The verdict of the combined check from the block as read back.  Zero points are valid: e(O, Q) = 1, so A = B = O accepts and exactly one of them zero rejects; otherwise the
// product decides.  Any status before the pairings rejects
enum KzgVerdict { KZG_REJECT = 0, KZG_ACCEPT = 1, KZG_BAD_G2 = 2 };
static inline KzgVerdict kzg_verdict(const uint8_t* got, size_t n) {
  if (got[3] != 0) return KZG_BAD_G2;   // the G2 point does not decode, or is the zero point
  const bool one = got[0] != 0, za = got[1] == 1, zb = got[2] == 1;
  return hdr_clean(got, n) && ((za && zb) || (!za && !zb && one)) ? KZG_ACCEPT : KZG_REJECT;
}
// Groth16: [S_0]alpha is the zero point | sum [S_j]IC_j is | sum [r_i]C_i is -- the partners of -beta, -gamma, -delta.  The combined check accepts when every status is 0, the
// product is one and none of the three is the zero point (the generator stood in for it in the Miller loop)
static inline uint8_t* g16_hdr_alpha_zero(uint8_t* BK) { return hdr_flags(BK); }
static inline uint8_t* g16_hdr_ic_zero(uint8_t* BK) { return hdr_flags(BK) + 1; }
static inline uint8_t* g16_hdr_c_zero(uint8_t* BK) { return hdr_flags(BK) + 2; }
static inline bool g16_verdict(const uint8_t* got, size_t n) { return hdr_clean(got, n) && got[0] != 0 && got[1] != 1 && got[2] != 1 && got[3] != 1; }
// What a combined check's verdict means to the caller: *all_ok, zero statuses where it accepts; *more: it rejects and the caller asked for statuses, which the per-item pass
// fills (none asked for: the fast reject, no per-item work)
static inline void combined_result(bool accept, size_t n, int* all_ok, int8_t* status, bool* more) {
  *all_ok = accept;
  if (accept && status) memset(status, 0, n);
  *more = !accept && status;
}

// the field's modulus p, 48 bytes big-endian
static const uint8_t FP_MODULUS_BE[48] = {0x1a, 0x01, 0x11, 0xea, 0x39, 0x7f, 0xe6, 0x9a, 0x4b, 0x1b, 0xa7, 0xb6, 0x43, 0x4b, 0xac, 0xd7, 0x64, 0x77, 0x4b, 0x84, 0xf3, 0x85, 0x12, 0xbf,
                                          0x67, 0x30, 0xd2, 0xa0, 0xf6, 0xb0, 0xf6, 0x24, 0x1e, 0xab, 0xff, 0xfe, 0xb1, 0x53, 0xff, 0xff, 0xb9, 0xfe, 0xff, 0xff, 0xff, 0xff, 0xaa, 0xab};
// -Q for a G2 point in affine wire bytes (x.c0 || x.c1 || y.c0 || y.c1, 48 bytes big-endian each, every coordinate below p): y -> p - y, a zero coordinate stays zero
static inline void g2_wire_negate(const uint8_t* in192, uint8_t* out192) {
  memcpy(out192, in192, 96);
  for (int k = 2; k < 4; k++) {
    const uint8_t* y = in192 + 48 * k; uint8_t* o = out192 + 48 * k;
    bool zero = true;
    for (int i = 0; i < 48; i++) zero = zero && y[i] == 0;
    int bw = 0;
    for (int i = 47; i >= 0; i--) { const int d = (int)FP_MODULUS_BE[i] - (int)y[i] - bw; o[i] = zero ? 0 : (uint8_t)d; bw = d < 0; }
  }
}
}  // namespace nbls
