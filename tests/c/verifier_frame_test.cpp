// verifier_frame_test.cpp -- csrc/verifier_frame.h (the carvings of the KZG verifiers' pairs block and per-item tail, the read-back header, the verdicts of the KZG and the
// Groth16 combined check, the negation of a G2 point in wire bytes) as a stand-alone program for AddressSanitizer / UBSan (csrc/Makefile: ../verifier_frame_test; run by
// tests/test_debug_build.py).  The totals are compared with the formulas the two KZG pipelines carried before the frame was shared, written out here; the verdicts are read from
// heap blocks of exactly back_bytes(n) bytes, so a read past the statuses is a sanitizer report and not a silent pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "verifier_frame.h"
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

// the Groth16 rule as groth16_pipeline stated it: every status 0, the product is one, none of the three flags equals 1
static bool g16_expected(uint8_t one, uint8_t f1, uint8_t f2, uint8_t f3, bool clean) { return clean && one != 0 && f1 != 1 && f2 != 1 && f3 != 1; }
static void unhex(const char* hex, uint8_t* out, size_t n) {
  auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
  for (size_t i = 0; i < n; i++) out[i] = (uint8_t)(nib(hex[2 * i]) << 4 | nib(hex[2 * i + 1]));
}
// g2_wire_negate on heap blocks of exactly 192 bytes
static void check_negation() {
  // the generator of G2, x.c0 || x.c1 || y.c0 || y.c1, and the 192 bytes of -G2 that the verifiers staged before the negation was shared (recorded from that code)
  static const char* gen = "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
                           "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                           "0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801"
                           "0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be";
  static const char* neg = "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"
                           "13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                           "0d1b3cc2c7027888be51d9ef691d77bcb679afda66c73f17f9ee3837a55024f78c71363275a75d75d86bab79f74782aa"
                           "13fa4d4a0ad8b1ce186ed5061789213d993923066dddaf1040bc3ff59f825c78df74f2d75467e25e0f55f8a00fa030ed";
  uint8_t *g = (uint8_t*)malloc(192), *want = (uint8_t*)malloc(192), *a = (uint8_t*)malloc(192), *b = (uint8_t*)malloc(192);
  unhex(gen, g, 192); unhex(neg, want, 192);
  g2_wire_negate(g, a);
  CHECK(memcmp(a, want, 192) == 0);
  g2_wire_negate(a, b);
  CHECK(memcmp(b, g, 192) == 0);   // twice: the identity
  // a coordinate that is all zero stays zero (p - 0 = p is no field element), the other one is still negated; x is copied
  for (int k = 2; k < 4; k++) {
    memcpy(b, g, 192); memset(b + 48 * k, 0, 48);
    g2_wire_negate(b, a);
    const int other = 5 - k;
    bool zero = true;
    for (int i = 0; i < 48; i++) zero = zero && a[48 * k + i] == 0;
    CHECK(zero && memcmp(a, g, 96) == 0 && memcmp(a + 48 * other, want + 48 * other, 48) == 0);
  }
  memset(b, 0, 192);
  g2_wire_negate(b, a);
  CHECK(memcmp(a, b, 192) == 0);
  CHECK(FP_MODULUS_BE[0] == 0x1a && FP_MODULUS_BE[47] == 0xab);
  free(g); free(want); free(a); free(b);
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
    CHECK(back_bytes(n) == 16 + n);
    uint8_t* got = (uint8_t*)malloc(back_bytes(n));
    CHECK(hdr_one(got) == got && kzg_hdr_a_zero(got) == got + 1 && kzg_hdr_b_zero(got) == got + 2 && kzg_hdr_g2_status(got) == got + 3 && hdr_pre(got) == got + 16);
    CHECK(hdr_flags(got) == got + 1 && g16_hdr_alpha_zero(got) == got + 1 && g16_hdr_ic_zero(got) == got + 2 && g16_hdr_c_zero(got) == got + 3 && HDR_BYTES == 16);
    // all sixteen settings of (one, za, zb, G2 status) x the statuses clean, unclean at the first index, unclean at the last index only
    int accepted = 0;
    for (int m = 0; m < 16; m++)
      for (int dirty = 0; dirty < 3; dirty++) {
        const bool one = m & 1, za = m & 2, zb = m & 4, g2_bad = m & 8;
        memset(got, 0, back_bytes(n));
        *hdr_one(got) = one; *kzg_hdr_a_zero(got) = za; *kzg_hdr_b_zero(got) = zb; *kzg_hdr_g2_status(got) = g2_bad ? 4 : 0;
        memset(got + 4, 0xee, 12);   // the unused bytes decide nothing
        if (dirty == 1) hdr_pre(got)[0] = 3;
        if (dirty == 2) hdr_pre(got)[n - 1] = 14;
        const KzgVerdict v = kzg_verdict(got, n);
        CHECK(v == expected(one, za, zb, g2_bad, dirty == 0));
        accepted += v == KZG_ACCEPT;
      }
    CHECK(accepted == 3);   // (one, not za, not zb), and za with zb whatever `one` says: each with clean statuses and a G2 point that decoded
    // a zero flag is the value 1 and nothing else (the to-affine program writes 0 or 1; a decoder status there would not count as zero)
    memset(got, 0, back_bytes(n));
    got[1] = got[2] = 2;
    CHECK(kzg_verdict(got, n) == KZG_REJECT);
    got[0] = 1;
    CHECK(kzg_verdict(got, n) == KZG_ACCEPT);
    // Groth16: all sixteen settings of (one, the three zero flags) x the statuses clean, unclean at the first index only, unclean at the last index only
    int g16_accepted = 0;
    for (int m = 0; m < 16; m++)
      for (int dirty = 0; dirty < 3; dirty++) {
        memset(got, 0, back_bytes(n));
        *hdr_one(got) = m & 1; *g16_hdr_alpha_zero(got) = (m >> 1) & 1; *g16_hdr_ic_zero(got) = (m >> 2) & 1; *g16_hdr_c_zero(got) = (m >> 3) & 1;
        memset(got + 4, 0xee, 12);   // the unused bytes decide nothing
        if (dirty == 1) hdr_pre(got)[0] = 3;
        if (dirty == 2) hdr_pre(got)[n - 1] = 14;
        const bool v = g16_verdict(got, n);
        CHECK(v == g16_expected(got[0], got[1], got[2], got[3], dirty == 0));
        CHECK(v == (m == 1 && dirty == 0));
        g16_accepted += v;
        // what the caller is told: the verdict, zero statuses on acceptance alone, the per-proof pass where it rejects and statuses were asked for
        int all_ok = 7; bool more = true; int8_t* st = (int8_t*)malloc(n);
        memset(st, 5, n);
        combined_result(v, n, &all_ok, st, &more);
        CHECK(all_ok == (int)v && more == !v && st[0] == (v ? 0 : 5) && st[n - 1] == (v ? 0 : 5));
        all_ok = 7; more = true;
        combined_result(v, n, &all_ok, nullptr, &more);
        CHECK(all_ok == (int)v && !more);
        free(st);
      }
    CHECK(g16_accepted == 1);   // the product is one, no flag set, clean statuses
    // a flag is the value 1 and nothing else: 2 does not count as a zero point
    memset(got, 0, back_bytes(n));
    got[0] = 1; got[1] = got[2] = got[3] = 2;
    CHECK(g16_verdict(got, n));
    got[2] = 1;
    CHECK(!g16_verdict(got, n));
    got[2] = 2; got[0] = 0;
    CHECK(!g16_verdict(got, n));
    free(got);
    printf("n %zu tail %zu back %zu\n", n, off, back_bytes(n));
  }
  check_negation();
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
