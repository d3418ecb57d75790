// bufs.h -- the buffer list of a launch: which pointer and stride a program's buffer index is bound to.  Plain C++, no HIP, no context (tests/c/bufs_test.cpp runs it under the
// sanitizers).  A list owns its entries (at most MAX_BUFS, by value), so a ChainLink copies and outlives the braces it was written with.
#pragma once
#include <cstddef>
#include <initializer_list>
#include "programs.h"   // ProgId; vm.h: IOBuf, MAX_BUFS
namespace nbls {
struct BufArg { int idx; const void* ptr; size_t stride; };
static inline BufArg B(int idx, const void* p, size_t stride) { return {idx, p, stride}; }
struct BufList {
  BufArg a[MAX_BUFS] = {}; int count = 0;   // count < 0: written with more than MAX_BUFS entries (bind_bufs refuses it)
  BufList() {}
  BufList(std::initializer_list<BufArg> l) : count(l.size() > (size_t)MAX_BUFS ? -1 : (int)l.size()) { for (int i = 0; i < count; i++) a[i] = l.begin()[i]; }
  const BufArg* begin() const { return a; }
  const BufArg* end() const { return a + (count > 0 ? count : 0); }
};
// one program of a chain (run_chain) with its buffers
struct ChainLink { ProgId id; BufList bufs; };
// out[0 .. MAX_BUFS) <- the list; an index it does not name stays {nullptr, 0}.  false: an index outside [0, MAX_BUFS) or too long a list -- the launch is refused
static inline bool bind_bufs(IOBuf* out, const BufList& l) {
  for (int k = 0; k < MAX_BUFS; k++) out[k] = IOBuf{nullptr, 0};
  if (l.count < 0) return false;
  for (const BufArg& b : l) {
    if (b.idx < 0 || b.idx >= MAX_BUFS) return false;
    out[b.idx] = IOBuf{(uint8_t*)b.ptr, b.stride};
  }
  return true;
}
}  // namespace nbls
