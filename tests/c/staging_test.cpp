// staging_test.cpp -- the pure part of csrc/staging.h (layout builder, packing, the oversize-tag rule) as a stand-alone program for AddressSanitizer / UBSan
// (csrc/Makefile: ../staging_test; run by tests/test_debug_build.py, which compares what is printed here).  Every block is a heap buffer of exactly the size the layout
// reports, so a write past a part is a sanitizer report and not a silent pass.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "staging.h"
using namespace nbls;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static void hex(const char* label, const uint8_t* p, size_t n) { printf("%s", label); for (size_t i = 0; i < n; i++) printf("%02x", p[i]); printf("\n"); }

int main() {
  // parts of 0, 1, 15, 16 and 17 bytes (and a trailing empty one): every part filled with its own byte, then read back
  const size_t sizes[] = {0, 1, 15, 16, 17, 0};
  const size_t np = sizeof(sizes) / sizeof(sizes[0]);
  StageLayout lay; size_t off[np];
  for (size_t i = 0; i < np; i++) off[i] = lay.part(sizes[i]);
  printf("layout");
  for (size_t i = 0; i < np; i++) printf(" %zu:%zu", sizes[i], off[i]);
  printf(" in_bytes %zu\n", lay.in_bytes);
  {
    uint8_t* block = (uint8_t*)malloc(lay.in_bytes);
    for (size_t i = 0; i < np; i++) { std::vector<uint8_t> src(sizes[i], (uint8_t)(0xa0 + i)); pack_bytes(block + off[i], src.data(), sizes[i]); }
    for (size_t i = 0; i < np; i++) for (size_t k = 0; k < sizes[i]; k++) CHECK(block[off[i] + k] == 0xa0 + i);
    free(block);
  }
  CHECK(StageLayout().in_bytes == 0);
  // relative offsets: count + 1 words behind a part of 5 bytes, the block again exactly in_bytes long
  const uint32_t offs[] = {5, 5, 9, 40}, one[] = {7, 12};
  for (int t = 0; t < 2; t++) {
    const uint32_t* o = t ? one : offs; const size_t count = t ? 1 : 3;
    StageLayout l2; l2.part(5); const size_t o_rel = l2.part((count + 1) * 4);
    uint8_t* block = (uint8_t*)malloc(l2.in_bytes);
    pack_rel(block + o_rel, o, count);
    printf("rel");
    for (size_t i = 0; i <= count; i++) { uint32_t w; memcpy(&w, block + o_rel + 4 * i, 4); printf(" %u", w); }
    printf("\n");
    free(block);
  }
  // tags of 0, 1, 255, 256 and 300 bytes (byte i = 7 i + 3): into a buffer of exactly the effective length, then into the 256-byte part of a block
  const size_t lens[] = {0, 1, 255, 256, 300};
  for (size_t len : lens) {
    std::vector<uint8_t> tag(len); for (size_t i = 0; i < len; i++) tag[i] = (uint8_t)(7 * i + 3);
    const size_t eff = len > 255 ? 32 : len;
    uint8_t* exact = (uint8_t*)malloc(eff ? eff : 1);
    CHECK(pack_dst(exact, tag.data(), len) == eff);
    StageLayout l3; l3.part(3); const size_t o_dst = l3.part(256);
    uint8_t* block = (uint8_t*)malloc(l3.in_bytes);
    CHECK(pack_dst(block + o_dst, tag.data(), len) == eff && (!eff || memcmp(block + o_dst, exact, eff) == 0));
    uint8_t scratch[32]; size_t l = len; const uint8_t* e = effective_dst(tag.data(), &l, scratch);
    CHECK(l == eff && (len > 255 ? e == scratch : e == tag.data()) && (!eff || memcmp(e, exact, eff) == 0));
    printf("dst %zu len %zu ", len, eff); hex("hex ", exact, eff);
    free(block); free(exact);
  }
  // strictly increasing offsets
  size_t n = 0, mx = 0;
  const uint32_t inc[] = {5, 6, 9, 40}, flat[] = {5, 5, 9, 40}, down[] = {5, 9, 8, 40};
  CHECK(strict_groups(3, inc, &n, &mx) && n == 35 && mx == 31);
  CHECK(!strict_groups(3, flat, &n, &mx) && !strict_groups(3, down, &n, &mx));
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
