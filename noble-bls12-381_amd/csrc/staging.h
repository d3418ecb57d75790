// staging.h -- the one staged block of a host-buffer pipeline: every input packed into the context's page-locked block, ONE asynchronous copy to the device, a chain of kernels,
// ONE block copied back, one synchronisation.  Two parts: the block's format (plain C++, no HIP, no context: tests/c/staging_test.cpp runs it under the sanitizers) and the
// call (Staged, compiled where nbls_internal.h includes this file), which owns the rule "no return while the block is in flight, no secret left behind".
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "sha256.h"
namespace nbls {
// ---- the format ------------------------------------------------------------------------------------------------
// part(bytes): the offset of the next part, 16-byte aligned; in_bytes: the end of the last part.  A part of zero bytes takes no space.
struct StageLayout {
  size_t in_bytes = 0;
  size_t part(size_t bytes) { const size_t o = (in_bytes + 15) & ~(size_t)15; in_bytes = o + bytes; return o; }
};
static inline void pack_bytes(uint8_t* at, const void* src, size_t bytes) { if (bytes) memcpy(at, src, bytes); }
// count + 1 words: the offsets relative to the first (the caller's arrays are read from offs[0] on)
static inline void pack_rel(void* at, const uint32_t* offs, size_t count) { uint32_t* rel = (uint32_t*)at; for (size_t i = 0; i <= count; i++) rel[i] = offs[i] - offs[0]; }
// a domain-separation tag into its 256-byte part: at most 255 bytes (sha256.h effective_dst); returns the length the hashing kernel is given
static inline size_t pack_dst(uint8_t* at, const uint8_t* dst, size_t dst_len) {
  uint8_t digest[32];
  dst = effective_dst(dst, &dst_len, digest);
  pack_bytes(at, dst, dst_len);
  return dst_len;
}
// strictly increasing offsets (no empty group) -> the number of entries and the largest group; the callers set their own limits on both
static inline bool strict_groups(size_t n_groups, const uint32_t* off, size_t* n, size_t* maxgroup) {
  size_t mx = 0;
  for (size_t g = 0; g < n_groups; g++) {
    if (off[g + 1] <= off[g]) return false;
    if ((size_t)(off[g + 1] - off[g]) > mx) mx = off[g + 1] - off[g];
  }
  *n = off[n_groups] - off[0]; *maxgroup = mx;
  return true;
}
}  // namespace nbls

#ifdef NBLS_STAGING_CALL
// ---- the call (one per pipeline call, on the stack, under the context's lock; takes no lock itself) ------------------
// the single device-to-host copy of a call into the context's read-back block and the call's synchronisation (also for the chains that stage nothing: verify_pipeline, the per-set pass)
static inline int read_back(nbls_ctx* ctx, hipStream_t s, const void* d_src, size_t back, const uint8_t** host) {
  const int r = ensure_pinned_out(ctx, back); if (r) return r;   // (already large enough when the call sent a Staged block)
  HIPCHK(hipMemcpyAsync(ctx->pinned_out, d_src, back, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *host = ctx->pinned_out;
  return NBLS_OK;
}
// A part is declared with its source -- bytes(), rel(), dst(), secret() return its offset, the same on the host and on the device -- and send() packs them all.  send() comes
// with the call's other ensure_* / need() calls, before anything is in flight (growing a page-locked block frees it), and arms the object BEFORE the copy is issued: from then on
// every exit from the scope waits for the whole device (as ForkGuard does: several pipelines fork onto side / side2), except the success path, which fetch() has synchronised (or
// done(), where the read-back is another function's).  The secret() part is zeroed in the host block on every exit, behind that wait: the copy may still be reading it.  The
// device copies of keys stay with HostIO::secret / wipe.
struct Staged : StageLayout {
  struct Part { int kind; size_t off; const void* src; size_t n; };   // kind 0: n bytes, 1: n + 1 offsets, 2: a tag of n bytes
  nbls_ctx* ctx; hipStream_t s; std::vector<Part> parts; size_t dst_len = 0, key_off = 0, key_bytes = 0; bool armed = false, packed = false;
  Staged(nbls_ctx* c, hipStream_t st) : ctx(c), s(st) {}
  ~Staged() {
    if (armed) (void)hipDeviceSynchronize();
    if (packed && key_bytes) memset(ctx->pinned + key_off, 0, key_bytes);
  }
  size_t add(int kind, size_t bytes, const void* src, size_t n) { parts.push_back({kind, part(bytes), src, n}); return parts.back().off; }
  size_t bytes(const void* src, size_t n) { return add(0, n, src, n); }
  size_t rel(const uint32_t* offs, size_t count) { return add(1, (count + 1) * 4, offs, count); }
  size_t dst(const uint8_t* tag, size_t len) { return add(2, 256, tag, len); }   // dst_len: the effective length, from send() on
  size_t secret(const void* src, size_t n) { key_bytes = n; return key_off = bytes(src, n); }
  int send(void* d_block, size_t back) {
    int r;
    if ((r = ensure_pinned(ctx, in_bytes)) || (r = ensure_pinned_out(ctx, back))) return r;
    packed = true;
    for (const Part& p : parts) {
      uint8_t* at = ctx->pinned + p.off;
      if (p.kind == 0) pack_bytes(at, p.src, p.n); else if (p.kind == 1) pack_rel(at, (const uint32_t*)p.src, p.n); else dst_len = pack_dst(at, (const uint8_t*)p.src, p.n);
    }
    armed = true;
    HIPCHK(hipMemcpyAsync(d_block, ctx->pinned, in_bytes, hipMemcpyHostToDevice, s));
    return NBLS_OK;
  }
  int fetch(const void* d_src, size_t back, const uint8_t** host) { const int r = read_back(ctx, s, d_src, back, host); if (!r) armed = false; return r; }
  // fetch, then the two halves of the block to the caller: results | statuses (optional)
  int fetch_to(const void* d_src, void* out, size_t out_bytes, void* status, size_t st_bytes) {
    const uint8_t* got; const int r = fetch(d_src, out_bytes + st_bytes, &got); if (r) return r;
    memcpy(out, got, out_bytes); if (status) memcpy(status, got + out_bytes, st_bytes);
    return NBLS_OK;
  }
  void done() { armed = false; }
};
#endif
