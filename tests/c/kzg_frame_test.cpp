// kzg_frame_test.cpp -- csrc/kzg_frame.h (the carvings of the KZG verifiers' pairs block and per-item tail, the read-back header and the verdict of the combined check) as a
// stand-alone program for AddressSanitizer / UBSan (csrc/Makefile: ../kzg_frame_test; run by tests/test_debug_build.py).  The totals are compared with the formulas the two
// pipelines carried before the frame was shared, written out here; the verdict is read from heap blocks of exactly kzg_back_bytes(n) bytes, so a read past the statuses is a
// sanitizer report and not a silent pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "kzg_frame.h"
using namespace nbls;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }
struct Part { size_t off, bytes; };
// every part 64-byte aligned, no two parts overlapping, the last one ending inside `total`
static void check_parts(const std::vector<Part>& parts, size_t total) {
  for (size_t i = 0; i < parts.size(); i++) {
    CHECK(parts[i].off % 64 == 0 && parts[i].off + parts[i].bytes <= total);
    for (size_t j = 0; j < i; j++) CHECK(parts[i].off >= parts[j].off + parts[j].bytes || parts[j].off >= parts[i].off + parts[i].bytes);
  }
}
// the rule as the pipelines stated it, from the four header fields and the statuses
static KzgVerdict expected(bool one, bool za, bool zb, bool g2_bad, bool clean) {
  if (g2_bad) return KZG_BAD_G2;
  return clean && ((za && zb) || (!za && !zb && one)) ? KZG_ACCEPT : KZG_REJECT;
}

int main() {
  const size_t raw = 64, p = 3 * raw, line = 6 * 68 * raw;   // one raw field element, one raw projective G1 point, one line table (68 lines of three Fp2)
  CHECK(raw == (size_t)RAW_FP_BYTES && line == (size_t)LINE_ELEMS * raw);
  size_t o = 0;
  CHECK(carve(&o, 0) == 0 && o == 0 && carve(&o, 1) == 0 && o == 64 && carve(&o, 64) == 64 && o == 128 && carve(&o, 65) == 128 && o == 256);
  // the pairs block does not depend on n
  const KzgPairs a = kzg_pairs_carve();
  check_parts({{a.g2, 2 * 192}, {a.tb, 2 * line}, {a.pt2, 2 * 96}, {a.res, 576}, {a.b3, 3 * 96}, {a.bst, 3}, {a.bj, 3 * p}, {a.bn, 2 * raw}}, a.bytes);
  CHECK(a.bytes == up64(2 * 192) + up64(2 * line) + up64(2 * 96) + up64(576) + up64(3 * 96) + up64(3) + up64(3 * p) + up64(2 * raw));
  CHECK(a.g2 == 0 && a.tb == 384 && a.pt2 == a.tb + 2 * line && a.bn + 2 * raw == a.bytes);
  printf("pairs %zu\n", a.bytes);
  for (size_t n : {(size_t)1, (size_t)3, (size_t)257}) {
    // the per-item tail behind a front of the caller's own (kzg_pipeline: two arrays of n scalars)
    size_t off = 0;
    const size_t b_zs = carve(&off, n * 32), b_ny = carve(&off, n * 32);
    KzgItemTail t;
    const size_t b_t = kzg_item_tail_carve(n, &off, &t);
    CHECK(b_zs == 0 && b_ny == up64(n * 32) && b_t == 2 * up64(n * 32) && t.p3 == 0);
    check_parts({{b_zs, n * 32}, {b_ny, n * 32}, {b_t + t.p3, 3 * n * 96}, {b_t + t.st3, 3 * n}, {b_t + t.proj, 3 * n * p}, {b_t + t.n, n * raw}, {b_t + t.ni, n * raw}, {b_t + t.x, n * 96},
                 {b_t + t.e, n * 576}, {b_t + t.v, n}, {b_t + t.xz, n}, {b_t + t.fs, n}}, off);
    CHECK(off == 2 * up64(n * 32) + up64(3 * n * 96) + up64(3 * n) + up64(3 * n * p) + 2 * up64(n * raw) + up64(n * 96) + up64(n * 576) + 3 * up64(n));
    // what is read back: 16 header bytes, then the n statuses before any pairing
    CHECK(kzg_back_bytes(n) == 16 + n);
    uint8_t* got = (uint8_t*)malloc(kzg_back_bytes(n));
    CHECK(kzg_hdr_one(got) == got && kzg_hdr_a_zero(got) == got + 1 && kzg_hdr_b_zero(got) == got + 2 && kzg_hdr_g2_status(got) == got + 3 && kzg_hdr_pre(got) == got + 16);
    // all sixteen settings of (one, za, zb, G2 status) x the statuses clean, unclean at the first index, unclean at the last index only
    int accepted = 0;
    for (int m = 0; m < 16; m++)
      for (int dirty = 0; dirty < 3; dirty++) {
        const bool one = m & 1, za = m & 2, zb = m & 4, g2_bad = m & 8;
        memset(got, 0, kzg_back_bytes(n));
        *kzg_hdr_one(got) = one; *kzg_hdr_a_zero(got) = za; *kzg_hdr_b_zero(got) = zb; *kzg_hdr_g2_status(got) = g2_bad ? 4 : 0;
        memset(got + 4, 0xee, 12);   // the unused bytes decide nothing
        if (dirty == 1) kzg_hdr_pre(got)[0] = 3;
        if (dirty == 2) kzg_hdr_pre(got)[n - 1] = 14;
        const KzgVerdict v = kzg_verdict(got, n);
        CHECK(v == expected(one, za, zb, g2_bad, dirty == 0));
        accepted += v == KZG_ACCEPT;
      }
    CHECK(accepted == 3);   // (one, not za, not zb), and za with zb whatever `one` says: each with clean statuses and a G2 point that decoded
    // a zero flag is the value 1 and nothing else (the to-affine program writes 0 or 1; a decoder status there would not count as zero)
    memset(got, 0, kzg_back_bytes(n));
    got[1] = got[2] = 2;
    CHECK(kzg_verdict(got, n) == KZG_REJECT);
    got[0] = 1;
    CHECK(kzg_verdict(got, n) == KZG_ACCEPT);
    free(got);
    printf("n %zu tail %zu back %zu\n", n, off, kzg_back_bytes(n));
  }
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
