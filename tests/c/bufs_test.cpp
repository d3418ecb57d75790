// bufs_test.cpp -- the buffer lists of the launch path (csrc/bufs.h: BufArg, BufList, ChainLink, bind_bufs) as a stand-alone program for AddressSanitizer / UBSan
// (csrc/Makefile: ../bufs_test; run by tests/test_debug_build.py).  The links are written with braces inside a helper and returned by value, so every list bound here is a copy
// whose braces are long gone: a list that only referred to them would be a use after scope.
#include <array>
#include <cstdio>
#include <vector>
#include "bufs.h"
using namespace nbls;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static uint8_t arena[8][4];   // distinct addresses to bind; never read through

static std::array<ChainLink, 3> make_links(int shift) {
  uint8_t *a = arena[shift], *b = arena[shift + 1], *c = arena[shift + 2];
  const ChainLink links[3] = {{P_EXPX, {B(3, a, 768), B(5, b, 768)}},
                              {P_FE_MID1, {B(3, a, 768), B(5, b, 768), B(6, c, 64)}},
                              {P_FE_FINAL, {B(0, a, 1), B(1, a, 2), B(2, a, 3), B(3, a, 4), B(4, b, 5), B(5, b, 6), B(6, c, 7), B(7, c, 0)}}};
  return {links[0], links[1], links[2]};
}
static void scribble() { volatile uint8_t junk[1024]; for (size_t i = 0; i < sizeof junk; i++) junk[i] = 0xa5; }   // over the stack the helper used

// what entry k of a bound list must hold
struct Want { const uint8_t* ptr; uint64_t stride; };
static void check_bound(const IOBuf* got, const Want* want) {
  for (int k = 0; k < MAX_BUFS; k++) CHECK(got[k].ptr == want[k].ptr && got[k].stride == want[k].stride);
}

int main() {
  for (int shift = 0; shift < 2; shift++) {
    const std::array<ChainLink, 3> links = make_links(shift);
    scribble();
    std::vector<ChainLink> copies(links.begin(), links.end());     // ... and copied once more, onto the heap
    uint8_t *a = arena[shift], *b = arena[shift + 1], *c = arena[shift + 2];
    const Want want[3][MAX_BUFS] = {{{nullptr, 0}, {nullptr, 0}, {nullptr, 0}, {a, 768}, {nullptr, 0}, {b, 768}, {nullptr, 0}, {nullptr, 0}},
                                    {{nullptr, 0}, {nullptr, 0}, {nullptr, 0}, {a, 768}, {nullptr, 0}, {b, 768}, {c, 64}, {nullptr, 0}},
                                    {{a, 1}, {a, 2}, {a, 3}, {a, 4}, {b, 5}, {b, 6}, {c, 7}, {c, 0}}};
    const ProgId ids[3] = {P_EXPX, P_FE_MID1, P_FE_FINAL};
    const int counts[3] = {2, 3, 8};
    for (int i = 0; i < 3; i++) {
      for (const ChainLink* l : {&links[i], (const ChainLink*)&copies[i]}) {
        IOBuf bufs[MAX_BUFS];
        for (IOBuf& x : bufs) x = IOBuf{arena[7], 99};              // bind_bufs clears what the list does not name
        CHECK(l->id == ids[i] && l->bufs.count == counts[i]);
        CHECK(bind_bufs(bufs, l->bufs));
        check_bound(bufs, want[i]);
      }
    }
  }
  // an index outside [0, MAX_BUFS) is refused, whatever stands beside it; nothing is bound through it
  for (int bad : {8, -1, 1 << 30, -(1 << 30)}) {
    IOBuf bufs[MAX_BUFS];
    for (IOBuf& x : bufs) x = IOBuf{arena[7], 99};
    CHECK(!bind_bufs(bufs, {B(2, arena[0], 4), B(bad, arena[1], 4), B(3, arena[2], 4)}));
    for (int k = 0; k < MAX_BUFS; k++) if (k != 2) CHECK(bufs[k].ptr == nullptr && bufs[k].stride == 0);
    CHECK(!bind_bufs(bufs, {B(bad, arena[1], 4)}));
    for (int k = 0; k < MAX_BUFS; k++) CHECK(bufs[k].ptr == nullptr && bufs[k].stride == 0);
  }
  // nine entries do not fit a list: refused, not truncated
  {
    IOBuf bufs[MAX_BUFS];
    const BufList nine = {B(0, arena[0], 1), B(1, arena[0], 1), B(2, arena[0], 1), B(3, arena[0], 1), B(4, arena[0], 1), B(5, arena[0], 1), B(6, arena[0], 1), B(7, arena[0], 1), B(0, arena[1], 1)};
    CHECK(nine.count < 0 && nine.begin() == nine.end() && !bind_bufs(bufs, nine));
    for (int k = 0; k < MAX_BUFS; k++) CHECK(bufs[k].ptr == nullptr && bufs[k].stride == 0);
  }
  // the empty list binds nothing; a later entry for the same index wins
  {
    IOBuf bufs[MAX_BUFS];
    CHECK(bind_bufs(bufs, BufList()) && bind_bufs(bufs, {}));
    for (int k = 0; k < MAX_BUFS; k++) CHECK(bufs[k].ptr == nullptr && bufs[k].stride == 0);
    CHECK(bind_bufs(bufs, {B(4, arena[0], 1), B(4, arena[1], 2)}) && bufs[4].ptr == arena[1] && bufs[4].stride == 2);
  }
  printf("links %d buffers %d\n", 3, MAX_BUFS);
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}
