// pipelines_msm.cpp -- multi-scalar multiplication sum_i [k_i]P_i (the reference only has the unweighted sums aggregatePublicKeys / aggregateSignatures,
// index.ts:771-788): one sum per call (nbls_g*_msm, nbls_msm_dev: dev_msm) and many independent sums in one call (nbls_g*_msm_batch: groups of one point / scalar array;
// nbls_g*_msm_rows: many scalar vectors against one set of points: msmb_plan / msmb_run).  Both are the bucket method with c-bit windows, every group operation a complete
// addition run as a step program over whole arrays, and both run the SAME stage (bucket_slices) on points that the same step has prepared (msm_prepare):
//   0. points to raw projective form.  Scalars of more than 192 bits are split with the curve endomorphisms (GLV / GLS): k = sum_i a_i |z|^i, [|z|^i]P is one cheap map of P.
//      G1: 2 points with 129-bit scalars, G2: 4 points with 65-bit scalars -- the same number of bucket additions, half / a quarter of the bit positions in the tail.
//   1. keys (group, window, digit) for every (point, window) -- the key is at the same time the index of its bucket, (group * nwin + window) << c | digit, so two neighbouring
//      groups with equal digits never share a run; device radix sort of the keys (hipCUB); the points follow.
//   2. segmented sum over the sorted list as a balanced tree inside every run of equal keys: in the round with stride d the
//      elements whose rank in their run is a multiple of 2d absorb the element d further on.  The pairs of a round are
//      listed by a compaction kernel (their number stays on the device: the step program reads it there) and added in place,
//      the step program addressing its operands through the list: (entries) - (number of buckets hit) additions in total whatever the distribution of the digits;
//      ceil(log2(longest run)) rounds -- the longest run is the one value read back, unless the caller knows a bound.  The head of every run ends up as its bucket sum.
//   3. sum_b b * B_b per (group, window) = sum_t 2^t * T_t with T_t = sum of the buckets whose index has bit t: c * 2^(c-1) gathered
//      points per (group, window), a balanced tree of c - 1 rounds of pairwise additions (data independent).
// What follows the bit-slices T is the caller's:
//   dev_msm, built for ONE large sum: fixed 12-bit windows (12 * 2^11 gathered bucket points per window whatever n is), scratch in named slots (MsmSlots), a synchronisation per
//     call, then Horner over t inside every window (one item per window) and acc <- 2^12 * acc + S_w from the top window down.
//   msmb_run, where the sums share every launch and the window width fits their size.  One chain on the call's stream:
//     H2D copy -> step 0 for all points and scalars of the call ONCE
//              -> per slab of whole groups: the stage with run-time width c and the true number of key bits (a slab holds at most 2^(32 - c) / nwin groups)
//                 -> ONE doubling-and-add chain over the bit positions: slice t of window w weighs 2^(c w + t), so every group's sum is sum_j 2^j T_(g, j) whatever c is:
//                 acc <- 2 acc + T_j from the top bit down (programs.h XP_DBLADD_G*), all groups of the slab the items of each launch -> to_affine into the output block
//              -> a group above the cut-off (NBLS_TUNE_MSMB_BIG) runs through dev_msm between the slabs, and so does a call of one group: 12 bits and the wide tail are right there
//              -> D2H copy
//     Scratch: SB_MSMB_CALL and SB_MSMB_SLAB (nbls_internal.h), both sized before the first launch.  Three parts: the plan (msmb_plan: host arithmetic only), the device core
//     (msmb_run: on converted points and scalars that are on the device) and the staging of the host-buffer calls around them.  msm_rows_dev is the core for callers whose
//     scalars never were on the host (pipelines_kzg_prove.cpp).
// Result of every sum: affine wire bytes + status (1 = the sum is the zero point).
#include "nbls_internal.h"
#include <algorithm>

// Step 2 on its own, for every caller that has segments to sum (bucket_slices: runs of equal keys; segment_sums in pipelines_multi_verify.cpp: the keys of a set, the sets of a message):
// `count` points P whose segment is keys[j] and whose place inside it is rank[j]; ceil(log2(maxrun)) rounds leave every segment's sum at its first point.  counters: one word per
// round (the pairs of that round), list: count words.
int segmented_sum(nbls_ctx* ctx, bool g2, size_t count, const uint32_t* keys, const uint32_t* rank, uint32_t* list, uint32_t* counters, uint8_t* P, size_t maxrun, hipStream_t s) {
  const size_t p = g2 ? 6 * RAW : 3 * RAW; int r;
  for (size_t d = 1; d < maxrun; d *= 2, counters++) {
    const size_t bound = count / (d + 1) + 1;      // every pair owns d + 1 list positions of its own segment
    LAUNCHCHK(nbls_msm_pairs_launch(count, (unsigned)d, keys, rank, list, counters, s));
    // P[j] += P[j + d] for the listed j, in place: the step program addresses its buffers through the list (KernelArgs.item_index);
    // a listed element is never the partner of another one (ranks are multiples of 2d), so no pair touches another pair's points
    if ((r = run(ctx, g2 ? P_G2_ADD_AB : P_G1_ADD_AB, bound, {B(3, P, p), B(4, P + d * p, p), B(5, P, p)}, s, counters, list))) return r;
  }
  return NBLS_OK;
}
// Step 0.  d_pts: npoints affine points -> Pj, dims * p bytes each (NULL: the caller has them converted already); dims > 1 (the call splits): d_k, nscalars scalars of 32 bytes
// -> Ks, dims * 32 bytes each
static int msm_prepare(nbls_ctx* ctx, bool g2, unsigned dims, size_t npoints, const void* d_pts, uint8_t* Pj, size_t nscalars, const void* d_k, uint8_t* Ks, hipStream_t s) {
  const size_t a = g2 ? 192 : 96, p = g2 ? 6 * RAW : 3 * RAW; const bool split = dims > 1; int r;
  if (d_pts && (r = run(ctx, split ? (g2 ? P_G2_MSM_PREP : P_G1_MSM_PREP) : (g2 ? P_G2_TO_PROJ : P_G1_TO_PROJ), npoints, {B(g2 ? 1 : 0, d_pts, a), B(3, Pj, dims * p)}, s))) return r;
  if (split) LAUNCHCHK(nbls_msm_decompose_launch((unsigned)nscalars, dims, d_k, Ks, s));
  return NBLS_OK;
}
// Steps 1 to 3: from the bucket fill to the last halving round, for nbw = groups x windows of c bits and M = keys.m * keys.nwin entries.  The caller sizes every buffer.
struct MsmKeys { unsigned m, dims, nwin, i0, g0, ngroups, n_pts; const uint32_t* off; const void* scalars; unsigned glen = 0, pt_block = 0, k_mod = 0; };   // the arguments of the keys launch (msm_kernels.hip msm_keys_kernel) but c; glen > 0: the wider map of the rows form
struct BucketBufs {
  uint32_t *words, *counters;   // 6 M words: keys, values, both sorted, ranks, pair list; 64 counters: [0] longest run, [1 + round] pairs of that round
  uint8_t* tmp; size_t sort_bytes, scan_bytes;   // scratch of the sort and the scan, one after the other in the same bytes, and what each is told it has
  uint8_t *P, *Bk, *G, *Gh;     // M sorted points, nbw << c buckets, (nbw * c) << (c - 1) gathered bucket points, half as many
};
// Pj: the converted points the values index.  run_bound: what the caller knows the longest run cannot exceed, or 0: it is read back, which synchronises the stream.  With M = 0
// the buckets are filled all the same, and every slice is the identity.  -> *T: the nbw * c bit-slices, T[bw * c + t] (in G or Gh)
static int bucket_slices(nbls_ctx* ctx, bool g2, size_t M, size_t nbw, unsigned c, int key_bits, const MsmKeys& k, const uint8_t* Pj, const BucketBufs& b, size_t run_bound, uint8_t** T,
                         hipStream_t s) {
  const size_t p = g2 ? 6 * RAW : 3 * RAW, nb = nbw << c, ng = (nbw * c) << (c - 1); int r;
  LAUNCHCHK(nbls_msm_fill_launch(nb, (unsigned)p, g2 ? ctx->ident_g2 : ctx->ident_g1, b.Bk, s));
  if (M) {
    uint32_t *kin = b.words, *vin = kin + M, *kout = vin + M, *vout = kout + M, *pos = vout + M, *list = pos + M;
    if (k.glen) LAUNCHCHK(nbls_msm_keys_map_launch(k.m, k.dims, k.nwin, c, k.i0, k.g0, k.ngroups, k.n_pts, k.glen, k.pt_block, k.k_mod, k.scalars, kin, vin, s));
    else LAUNCHCHK(nbls_msm_keys_launch(k.m, k.dims, k.nwin, c, k.i0, k.g0, k.ngroups, k.n_pts, k.off, k.scalars, kin, vin, s));
    size_t sb = b.sort_bytes, cb = b.scan_bytes;
    LAUNCHCHK(nbls_msm_sort_launch(b.tmp, &sb, kin, kout, vin, vout, M, key_bits, s));
    LAUNCHCHK(nbls_msm_gather_launch(M, (unsigned)p, vout, Pj, b.P, s));
    LAUNCHCHK(nbls_msm_rank_launch(b.tmp, &cb, M, kout, pos, b.counters, s));
    uint32_t maxrun = (uint32_t)run_bound;
    if (!run_bound) { HIPCHK(hipMemcpyAsync(&maxrun, b.counters, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
    if ((r = segmented_sum(ctx, g2, M, kout, pos, list, b.counters + 1, b.P, maxrun, s))) return r;
    LAUNCHCHK(nbls_msm_heads_launch(M, (unsigned)p, kout, b.P, b.Bk, s));
  }
  LAUNCHCHK(nbls_msm_bitsel_launch(nbw, c, (unsigned)p, b.Bk, b.G, s));
  uint8_t *src = b.G, *dst = b.Gh;
  for (size_t cnt = ng; cnt > nbw * c; cnt /= 2) {
    if ((r = run(ctx, g2 ? P_G2_ADD2 : P_G1_ADD2, cnt / 2, {B(3, src, 2 * p), B(5, dst, p)}, s))) return r;
    std::swap(src, dst);
  }
  *T = src;
  return NBLS_OK;
}
// One sum.  nbits bounds the scalars (< 2^nbits), 0 = 256.  sl: the scratch slots of this instance.
int dev_msm(nbls_ctx* ctx, bool g2, size_t n, const void* d_pts, const void* d_scalars, unsigned nbits, void* d_out, void* d_status, hipStream_t s, const MsmSlots& sl) {
  const size_t p = g2 ? 6 * RAW : 3 * RAW;
  const unsigned C = MSM_WINDOW_BITS;
  if (nbits == 0 || nbits > 256) nbits = 256;
  if (n > ((size_t)1 << 22)) return NBLS_EINVAL;
  // the split shortens the tail: 10 / 5 instead of 21 rounds of "12 doublings + 1 addition" on a single point at the end (latency-bound: 0.11 ms each)
  const bool split = nbits > 192;
  const unsigned dims = split ? (g2 ? 4 : 2) : 1;
  const size_t n_in = n;
  if (split) { n *= dims; nbits = g2 ? 65 : 129; }
  const unsigned nwin = (nbits + C - 1) / C;
  const size_t m = n * nwin, nb = (size_t)nwin << C, ng = ((size_t)nwin * C) << (C - 1);
  uint8_t *Pj, *P, *A, *K, *tmp, *Bk, *G, *Gh, *N, *NI, *acc, *cnt, *Ks = nullptr, *T; int r;
  if (split && (r = need(ctx, sl[MsmSlots::SPLIT_SCALARS], (n + 1) * 32, &Ks))) return r;
  size_t tmp_bytes = 0;
  size_t scan_bytes = 0;
  if (m) { LAUNCHCHK(nbls_msm_sort_launch(nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, m, 17, s)); LAUNCHCHK(nbls_msm_rank_launch(nullptr, &scan_bytes, m, nullptr, nullptr, nullptr,
      s)); tmp_bytes = std::max(tmp_bytes, scan_bytes); }
  if ((r = need(ctx, sl[MsmSlots::POINTS], (n + 1) * p, &Pj)) || (r = need(ctx, sl[MsmSlots::SORTED], (m + 1) * p, &P)) || (r = need(ctx, sl[MsmSlots::WINDOW_SUMS], ((size_t)nwin + 1) * p, &A)) ||
      (r = need(ctx, sl[MsmSlots::KEYS], (m + 1) * 24, &K)) || (r = need(ctx, sl[MsmSlots::NORM], RAW, &N)) || (r = need(ctx, sl[MsmSlots::NORM_INV], RAW, &NI)) ||
      (r = need(ctx, sl[MsmSlots::TEMP], tmp_bytes + 16, &tmp)) || (r = need(ctx, sl[MsmSlots::BUCKETS], nb * p, &Bk)) || (r = need(ctx, sl[MsmSlots::SLICES], ng * p, &G)) ||
      (r = need(ctx, sl[MsmSlots::SLICES_HALF], (ng / 2 + 2) * p, &Gh)) || (r = need(ctx, sl[MsmSlots::COUNTERS], 64 * 4, &cnt))) return r;
  acc = Gh + ng / 2 * p;
  if (m && (r = msm_prepare(ctx, g2, dims, n_in, d_pts, Pj, n_in, d_scalars, Ks, s))) return r;
  // one group of 12-bit windows, in the rows form (group 0, point i: no offsets are read): key = window << 12 | digit, value = the index of the converted point.  The sort is
  // told 17 key bits whatever nwin is; the longest run is read back on every call
  const MsmKeys keys{(unsigned)n, dims, nwin, 0, 0, 1, (unsigned)n_in, nullptr, split ? Ks : (const uint8_t*)d_scalars};
  if ((r = bucket_slices(ctx, g2, m, nwin, C, 17, keys, Pj, {(uint32_t*)K, (uint32_t*)cnt, tmp, tmp_bytes, scan_bytes, P, Bk, G, Gh}, 0, &T, s))) return r;
  uint8_t* S = A;   // per-window sums
  static const bool wide_combine = env_long("NBLS_MSM_WIDE", 1) != 0;
  // Horner over the bit-slices t of every window (sum_t 2^t T_t, one sum per window), then over the windows (below).  G1 (round 6): both with one limb per lane, a wavefront per
  // sum, the four products of a doubling level on its four rows (g1_wide.h: 0.74 -> 0.25 ms of a 65,536-point call); G2 and NBLS_MSM_WIDE=0: the step programs
  if (!g2 && wide_combine) LAUNCHCHK(nbls_g1_wide_combine_launch(T, (int)C, 1, S, nwin, s));
  else if ((r = run(ctx, g2 ? P_G2_HORNER : P_G1_HORNER, nwin, {B(3, T, C * p), B(5, S, p)}, s))) return r;
  // acc <- 2^12 acc + S_w from the top window down: (nwin - 1) x (12 doublings + 1 addition) on ONE point
  if (!g2 && wide_combine) LAUNCHCHK(nbls_g1_wide_combine_launch(S, (int)nwin, (int)C, acc, 1, s));
  else {
    HIPCHK(hipMemcpyAsync(acc, S + (size_t)(nwin - 1) * p, p, hipMemcpyDeviceToDevice, s));
    for (int w = (int)nwin - 2; w >= 0; w--)
      if ((r = run(ctx, g2 ? P_G2_SHIFTADD : P_G1_SHIFTADD, 1, {B(3, acc, p), B(4, S + (size_t)w * p, p), B(5, acc, p)}, s))) return r;
  }
  return to_affine(ctx, g2, 1, acc, N, NI, d_out, d_status, s);
}
unsigned scalars_bit_length(size_t n, const uint8_t* k32) {   // max over the batch
  int lead = 32;   // leading zero bytes common to all scalars
  for (size_t i = 0; i < n && lead; i++) { int z = 0; while (z < lead && k32[32 * i + z] == 0) z++; lead = z; }
  if (lead == 32) return 1;
  uint8_t top = 0; for (size_t i = 0; i < n; i++) top |= k32[32 * i + lead];
  unsigned bits = 8 * (31 - lead); while (top) { bits++; top >>= 1; }
  return bits;
}
// The tail of the host-buffer calls: n affine sums are in `out`, zero[g] = 1 says that sum g is the zero point.  It has no affine form: P_G*_TO_AFFINE multiplies by the inverse
// of a Z that is 0 mod p, and which representative of 0 the chain before it left there (dev_msm's one-limb-per-lane combine leaves p) decides what the binary GCD returns for
// it.  The contract is all-zero bytes, as every other call reports the zero point
static void msm_zero_tail(bool g2, size_t n, const uint8_t* zero, uint8_t* out, int8_t* status) {
  const size_t a = g2 ? 192 : 96;
  for (size_t g = 0; g < n; g++) if (zero[g] == 1) memset(out + g * a, 0, a);
  if (status) memcpy(status, zero, n);
}
int msm_host(nbls_ctx* ctx, bool g2, size_t n, const uint8_t* pts, const uint8_t* scalars32, uint8_t* out, int8_t* status) {
  if (!ctx || !out || (n && (!pts || !scalars32))) return NBLS_EINVAL;
  const size_t a = g2 ? 192 : 96;
  LOCKED(ctx); HostIO io{ctx}; void *dp = io.alloc(n * a), *dk = io.alloc(n * 32), *o = io.alloc(a), *st = io.alloc(1); if (!dp || !dk || !o || !st) return NBLS_EHIP;
  if (n) { HIPCHK(hipMemcpyAsync(dp, pts, n * a, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dk, scalars32, n * 32, hipMemcpyHostToDevice, s)); }
  int r = dev_msm(ctx, g2, n, dp, dk, n ? scalars_bit_length(n, scalars32) : 1, o, st, s); if (r) return r;
  uint8_t z = 0; HIPCHK(hipMemcpyAsync(out, o, a, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(&z, st, 1, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
  msm_zero_tail(g2, 1, &z, out, status);
  return NBLS_OK;
}
EXPORT int nbls_g1_msm(nbls_ctx* ctx, size_t n, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out96, int8_t* status) { return msm_host(ctx, false, n, pts96, scalars32, out96, status); }
EXPORT int nbls_g2_msm(nbls_ctx* ctx, size_t n, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out192, int8_t* status) { return msm_host(ctx, true, n, pts192, scalars32, out192, status); }
// device-resident variant: points (affine wire bytes), scalars (32 B big-endian, all < 2^nbits; nbits = 0 means 256), one affine result + int8 status
// in device memory; enqueued on `stream` (NULL = the context's stream) except for one 4-byte read-back in the middle
EXPORT int nbls_msm_dev(nbls_ctx* ctx, int g2, size_t n, const void* d_pts, const void* d_scalars32, unsigned nbits, void* d_out, void* d_status, void* stream) {
  if (!ctx || !d_out || !d_status || (n && (!d_pts || !d_scalars32))) return NBLS_EINVAL;
  DEV_ENTER(ctx, stream);
  return dev_msm(ctx, g2 != 0, n, d_pts, d_scalars32, nbits, d_out, d_status, s);
}

// ---- many sums in one call ------------------------------------------------------------------------------------------------------------------------------------------------
static const size_t MSMB_BIG_DEFAULT = 16384;              // points of a group, as given, above which it runs alone through dev_msm
static const size_t MSMB_SLAB_DEFAULT = (size_t)1 << 23;   // sorted entries + gathered bucket points of a slab: 1.6 GB of raw G1 points, 3.2 GB in G2
static const unsigned MSMB_WIDTHS[] = {4, 6, 8, 10, 12};
static const size_t MSMB_NO_READBACK = 8;                  // points of the largest group after the split up to which the rounds of the segmented sum follow from that size alone

static inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
// additions per group of `pts` points (after the split): the sorted list and the gathered bit-slices
static inline size_t group_cost(size_t pts, unsigned nbits, unsigned c) { const size_t nwin = (nbits + c - 1) / c; return pts * nwin + ((nwin * c) << (c - 1)); }

// The plan of one call: the window width, the slabs of whole groups between the big ones (allow_big; a group above the cut-off runs alone through dev_msm) and the carving of
// the largest slab's block.  off: n_groups + 1 relative offsets; nbits: the bit length of the call's longest scalar
static int msmb_plan(nbls_ctx* ctx, bool g2, size_t n_groups, const uint32_t* off, size_t n_pts, unsigned nbits, bool allow_big, MsmbPlan* out) {
  MsmbPlan& pl = *out;
  const size_t p = g2 ? 6 * RAW : 3 * RAW;
  pl.g2 = g2; pl.n_groups = n_groups; pl.n_pts = n_pts; pl.nbits = nbits;
  const bool split = pl.split = nbits > 192;
  const unsigned dims = pl.dims = split ? (g2 ? 4 : 2) : 1, kbits = pl.kbits = split ? (g2 ? 65 : 129) : nbits;
  const size_t big = n_groups == 1 ? 0 : ctx->msmb_big ? ctx->msmb_big : MSMB_BIG_DEFAULT, budget = ctx->msmb_slab ? ctx->msmb_slab : MSMB_SLAB_DEFAULT;
  auto is_big = [&](size_t g) { return allow_big && (n_groups == 1 || (size_t)(off[g + 1] - off[g]) > big); };
  // the window width: by the mean size of the groups that take the batched path
  unsigned c = (unsigned)ctx->msmb_window;
  if (!c) {
    size_t small_groups = 0, small_pts = 0;
    for (size_t g = 0; g < n_groups; g++) if (!is_big(g)) { small_groups++; small_pts += off[g + 1] - off[g]; }
    const size_t mean = small_groups ? (small_pts * dims + small_groups - 1) / small_groups : 0;
    c = MSMB_WIDTHS[0];
    for (unsigned w : MSMB_WIDTHS) if (group_cost(mean, kbits, w) < group_cost(mean, kbits, c)) c = w;
  }
  pl.c = c;
  const size_t nwin = pl.nwin = (kbits + c - 1) / c;
  pl.J = nwin * c; pl.jtop = std::min<size_t>(pl.J, kbits);   // bit positions from jtop on hold no digit bit: their slices are the identity
  const size_t max_groups = std::min<size_t>(((size_t)1 << (32 - c)) / nwin, (size_t)1 << 20);
  // slabs of whole groups between the big ones, and the scratch of the largest slab
  size_t maxM = 0, max_ngs = 0, sort_bytes = 0, scan_bytes = 0;
  for (size_t g = 0; g < n_groups;) {
    if (is_big(g)) { pl.parts.push_back({g, g + 1, true, 0}); g++; continue; }
    size_t g1 = g, cost = 0;
    while (g1 < n_groups && !is_big(g1) && g1 - g < max_groups) {
      const size_t cg = group_cost((size_t)(off[g1 + 1] - off[g1]) * dims, kbits, c);
      if (g1 > g && cost + cg > budget) break;
      cost += cg; g1++;
    }
    const size_t M = (size_t)(off[g1] - off[g]) * dims * nwin, nb = ((g1 - g) * nwin) << c;
    if (M >= ((size_t)1 << 31)) return NBLS_EINVAL;   // (unreachable below the call's limits: 2^22 scalars x 4 parts x 17 windows)
    int key_bits = (int)c; while (key_bits < 32 && ((size_t)1 << key_bits) < nb) key_bits++;
    pl.parts.push_back({g, g1, false, key_bits});
    if (M) {   // the sort's and the scan's scratch, asked for the slab as it will run
      size_t sb = 0, cb = 0;
      LAUNCHCHK(nbls_msm_sort_launch(nullptr, &sb, nullptr, nullptr, nullptr, nullptr, M, key_bits, nullptr));
      LAUNCHCHK(nbls_msm_rank_launch(nullptr, &cb, M, nullptr, nullptr, nullptr, nullptr));
      sort_bytes = std::max(sort_bytes, sb); scan_bytes = std::max(scan_bytes, cb);
    }
    maxM = std::max(maxM, M); max_ngs = std::max(max_ngs, g1 - g);
    g = g1;
  }
  pl.maxM = maxM; pl.max_ngs = max_ngs; pl.sort_bytes = sort_bytes; pl.scan_bytes = scan_bytes;
  const size_t max_nbw = max_ngs * nwin, max_nb = max_nbw << c, max_ng = (max_nbw * c) << (c - 1);
  const size_t tmp_bytes = std::max(sort_bytes, scan_bytes) + 16;
  // a slab's block: keys, values, both sorted, ranks, pair list | counters | sort / scan scratch | sorted points | buckets | bit-slices | their halves | accumulators | norms | inverses
  pl.s_cnt = al((maxM + 1) * 24); pl.s_tmp = pl.s_cnt + al(64 * 4); pl.s_P = pl.s_tmp + al(tmp_bytes); pl.s_bk = pl.s_P + al((maxM + 1) * p); pl.s_G = pl.s_bk + al((max_nb + 1) * p);
  pl.s_Gh = pl.s_G + al((max_ng + 1) * p); pl.s_acc = pl.s_Gh + al((max_ng / 2 + 1) * p); pl.s_N = pl.s_acc + al((max_ngs + 1) * p); pl.s_NI = pl.s_N + al((max_ngs + 1) * RAW);
  pl.slab_bytes = pl.s_NI + al((max_ngs + 1) * RAW);
  return NBLS_OK;
}

// The device core: every part of the plan on stream s.  Pj: the converted points (dims * p bytes each); d_k: the scalars as given (read when the call is not split, and by
// dev_msm for a big group); pl.Ks: the split scalars; d_pts: the affine points as given (only a big group reads them); d_off: the offsets on the device (unused in the rows
// form) -> O: one affine sum per group, OST: its zero flag; or, conv != NULL (G1 only), every sum as it stands in projective coordinates with its endomorphism image
// (XP_ENDO_G1: 2 x 3 raw elements, the form the split path reads) and nothing to O / OST: the sums are the points of a second pass and the identity may be among them
static int msmb_run(nbls_ctx* ctx, const MsmbPlan& pl, const uint32_t* off, const uint8_t* Pj, const uint8_t* d_k, const uint8_t* d_pts, const uint32_t* d_off, uint8_t* O, uint8_t* OST,
                    hipStream_t s, uint8_t* conv = nullptr) {
  const bool g2 = pl.g2;
  const size_t a = g2 ? 192 : 96, p = g2 ? 6 * RAW : 3 * RAW, n_groups = pl.n_groups, n_pts = pl.n_pts, nwin = pl.nwin, J = pl.J, jtop = pl.jtop;
  const unsigned dims = pl.dims, c = pl.c;
  uint8_t *SL = pl.SL, *acc = SL + pl.s_acc, *Nm = SL + pl.s_N, *NI = SL + pl.s_NI, *T; int r;
  const BucketBufs bufs{(uint32_t*)SL, (uint32_t*)(SL + pl.s_cnt), SL + pl.s_tmp, pl.sort_bytes, pl.scan_bytes, SL + pl.s_P, SL + pl.s_bk, SL + pl.s_G, SL + pl.s_Gh};
  const DevProgram& step = ctx->extra[g2 ? XP_DBLADD_G2 : XP_DBLADD_G1];
  for (const MsmbPart& pt : pl.parts) {
    const size_t g0 = pt.g0, ngs = pt.g1 - pt.g0, i0 = off[pt.g0], cnt = off[pt.g1] - i0;
    if (pt.big) {
      // (dev_msm synchronises the stream for its own longest run; its scratch is the main slots, which hold nothing of this call)
      if ((r = dev_msm(ctx, g2, cnt, n_pts ? d_pts : d_pts + i0 * a, d_k + i0 * 32, pl.nbits, O + g0 * a, OST + g0, s))) return r;
      continue;
    }
    const size_t m = cnt * dims, M = m * nwin;
    LAUNCHCHK(nbls_msm_fill_launch(ngs, (unsigned)p, g2 ? ctx->ident_g2 : ctx->ident_g1, acc, s));
    if (M) {   // (a slab without entries: every sum is the identity the accumulators hold)
      size_t maxg = 0; for (size_t g = pt.g0; g < pt.g1; g++) maxg = std::max(maxg, (size_t)(off[g + 1] - off[g]) * dims);   // a run lies inside one window of one group
      const MsmKeys keys{(unsigned)m, dims, (unsigned)nwin, (unsigned)i0, (unsigned)g0, (unsigned)n_groups, (unsigned)n_pts, d_off, pl.split ? pl.Ks : d_k, (unsigned)pl.glen,
                         (unsigned)pl.pt_block, (unsigned)pl.k_mod};
      if ((r = bucket_slices(ctx, g2, M, ngs * nwin, c, pt.key_bits, keys, Pj, bufs, maxg > MSMB_NO_READBACK ? 0 : maxg, &T, s))) return r;
      // T[g * J + j], the slice of bit position j of group g
      for (size_t j = jtop; j-- > 0;)
        if ((r = run_dev(ctx, step, -1, ngs, {B(3, acc, p), B(4, T + j * p, J * p)}, s, nullptr, nullptr))) return r;
    }
    if (conv) { if ((r = run_dev(ctx, ctx->extra[XP_ENDO_G1], -1, ngs, {B(3, acc, p), B(5, conv + g0 * 2 * p, 2 * p)}, s, nullptr, nullptr))) return r; }
    else if ((r = to_affine(ctx, g2, ngs, acc, Nm, NI, O + g0 * a, OST + g0, s))) return r;
  }
  return NBLS_OK;
}

// off: n_groups + 1 relative offsets (off[0] = 0) into the N scalars; n_pts > 0: the rows form (scalar i meets point i % n_pts), else scalar i meets point i
static int msm_batch_pipeline(nbls_ctx* ctx, bool g2, size_t n_groups, const std::vector<uint32_t>& off, size_t n_pts, size_t npoints, const uint8_t* pts, const uint8_t* scalars,
                              uint8_t* out, int8_t* status) {
  const size_t a = g2 ? 192 : 96, p = g2 ? 6 * RAW : 3 * RAW, N = off[n_groups];
  MsmbPlan pl; int r;
  if ((r = msmb_plan(ctx, g2, n_groups, off.data(), n_pts, N ? scalars_bit_length(N, scalars) : 1, true, &pl))) return r;
  const bool split = pl.split; const unsigned dims = pl.dims;
  // the call's block: points | scalars | offsets (what is staged) | converted points | split scalars | affine sums | statuses (what is read back)
  hipStream_t s = ctx->stream;
  Staged io(ctx, s);
  const size_t o_pts = io.bytes(pts, npoints * a), o_k = io.bytes(scalars, N * 32), o_off = io.rel(off.data(), n_groups), o_pj = al(io.in_bytes), o_ks = o_pj + al((npoints * dims + 1) * p),
               o_out = o_ks + al(split ? (N + 1) * 32 * dims : 0), back = n_groups * a + n_groups, call_bytes = o_out + al(back);
  uint8_t* CB; const uint8_t* res;
  // (from the copy on a failed call returns, and a later call touches the scratch, only after the device has drained)
  if ((r = need(ctx, SB_MSMB_CALL, call_bytes, &CB)) || (r = need(ctx, SB_MSMB_SLAB, pl.slab_bytes, &pl.SL)) || (r = upload_extra(ctx, g2 ? XP_DBLADD_G2 : XP_DBLADD_G1)) ||
      (r = io.send(CB, back)))
    return r;
  const uint8_t *d_pts = CB + o_pts, *d_k = CB + o_k; const uint32_t* d_off = (const uint32_t*)(CB + o_off);
  uint8_t *Pj = CB + o_pj, *O = CB + o_out, *OST = O + n_groups * a;
  pl.Ks = CB + o_ks;
  if (pl.maxM && (r = msm_prepare(ctx, g2, dims, npoints, d_pts, Pj, N, d_k, pl.Ks, s))) return r;
  if ((r = msmb_run(ctx, pl, off.data(), Pj, d_k, d_pts, d_off, O, OST, s))) return r;
  if ((r = io.fetch(O, back, &res))) return r;
  memcpy(out, res, n_groups * a);
  msm_zero_tail(g2, n_groups, res + n_groups * a, out, status);
  return NBLS_OK;
}

// The rows form in G1 from device memory (nbls_internal.h): the plan and its two slots first, then the chain.  The scalars are split as 256-bit values whatever they hold
int msm_rows_dev_plan(nbls_ctx* ctx, size_t n_pts, size_t n_rows, MsmbPlan* pl) {
  if (!n_pts || !n_rows || n_rows > MSMB_MAX_GROUPS || n_pts > MSMB_MAX_ITEMS || n_rows * n_pts > MSMB_MAX_ITEMS) return NBLS_EINVAL;
  std::vector<uint32_t> off(n_rows + 1);
  for (size_t g = 0; g <= n_rows; g++) off[g] = (uint32_t)(g * n_pts);
  int r;
  if ((r = msmb_plan(ctx, false, n_rows, off.data(), n_pts, 256, false, pl)) || (r = need(ctx, SB_MSMB_CALL, al((n_rows * n_pts + 1) * 32 * pl->dims), &pl->Ks)) ||
      (r = need(ctx, SB_MSMB_SLAB, pl->slab_bytes, &pl->SL)) || (r = upload_extra(ctx, XP_DBLADD_G1)))
    return r;
  return NBLS_OK;
}
int msm_rows_dev(nbls_ctx* ctx, const MsmbPlan& pl, const uint8_t* conv_pts, const uint8_t* d_scalars, uint8_t* d_out96, uint8_t* d_zero, hipStream_t s) {
  std::vector<uint32_t> off(pl.n_groups + 1); int r;
  for (size_t g = 0; g <= pl.n_groups; g++) off[g] = (uint32_t)(g * pl.n_pts);
  if ((r = msm_prepare(ctx, false, pl.dims, 0, nullptr, nullptr, pl.n_groups * pl.n_pts, d_scalars, pl.Ks, s))) return r;   // (the points came converted)
  return msmb_run(ctx, pl, off.data(), conv_pts, d_scalars, nullptr, nullptr, d_out96, d_zero, s);
}

// The wider map of the rows form in G1 (msm_keys_kernel; the two passes of the FK20 cell proofs and the one MSM of their handle): n_groups sums of glen scalars each, scalar i
// against point i % period + (i / pt_block) * period (pt_block = 0: i % period), read at i % k_mod of an array the caller has split already (k_mod > 0: no split here, and
// SB_MSMB_CALL is not taken), else at i of d_scalars.  Several plans of one call share the two slots: msm_map_plans_settle gives every plan the slots' final pointers
int msm_map_dev_plan(nbls_ctx* ctx, size_t glen, size_t period, size_t pt_block, size_t k_mod, size_t n_groups, MsmbPlan* pl) {
  if (!glen || !period || !n_groups || n_groups > MSMB_MAX_GROUPS || n_groups * glen > MSMB_MAX_ITEMS) return NBLS_EINVAL;
  std::vector<uint32_t> off(n_groups + 1);
  for (size_t g = 0; g <= n_groups; g++) off[g] = (uint32_t)(g * glen);
  int r;
  if ((r = msmb_plan(ctx, false, n_groups, off.data(), period, 256, false, pl))) return r;
  pl->glen = glen; pl->pt_block = pt_block; pl->k_mod = k_mod;
  if ((!k_mod && (r = need(ctx, SB_MSMB_CALL, al((n_groups * glen + 1) * 32 * pl->dims), &pl->Ks))) || (r = need(ctx, SB_MSMB_SLAB, pl->slab_bytes, &pl->SL)) ||
      (r = upload_extra(ctx, XP_DBLADD_G1)) || (r = upload_extra(ctx, XP_ENDO_G1)))
    return r;
  return NBLS_OK;
}
void msm_map_plans_settle(nbls_ctx* ctx, std::initializer_list<MsmbPlan*> plans) {
  for (MsmbPlan* pl : plans) if (pl->n_groups) { pl->SL = ctx->sb[SB_MSMB_SLAB]; if (!pl->k_mod) pl->Ks = ctx->sb[SB_MSMB_CALL]; }
}
// split (k_mod > 0): the caller's split scalars.  conv != NULL: the sums in the converted projective form (msmb_run), else affine sums and zero flags
int msm_map_dev(nbls_ctx* ctx, const MsmbPlan& pl, const uint8_t* conv_pts, const uint8_t* d_scalars, const uint8_t* split, uint8_t* d_out96, uint8_t* d_zero, uint8_t* conv, hipStream_t s) {
  std::vector<uint32_t> off(pl.n_groups + 1); int r;
  for (size_t g = 0; g <= pl.n_groups; g++) off[g] = (uint32_t)(g * pl.glen);
  MsmbPlan run_pl = pl;
  if (pl.k_mod) run_pl.Ks = const_cast<uint8_t*>(split);
  else if ((r = msm_prepare(ctx, false, pl.dims, 0, nullptr, nullptr, pl.n_groups * pl.glen, d_scalars, pl.Ks, s))) return r;
  return msmb_run(ctx, run_pl, off.data(), conv_pts, d_scalars, nullptr, nullptr, d_out96, d_zero, s, conv);
}
// a caller's scalars into the split form the wider map reads with k_mod (the handle's matrix, split once)
int msm_split_scalars(nbls_ctx* ctx, size_t n, const uint8_t* d_scalars, uint8_t* split, hipStream_t s) { return msm_prepare(ctx, false, 2, 0, nullptr, nullptr, n, d_scalars, split, s); }

static int msm_batch_host(nbls_ctx* ctx, bool g2, size_t n_groups, const uint32_t* group_offsets, size_t n_pts, const uint8_t* pts, const uint8_t* scalars, uint8_t* out, int8_t* status) {
  WHOLE_CALL(ctx);
  if (!ctx || !out || !n_groups || n_groups > MSMB_MAX_GROUPS) return NBLS_EINVAL;
  const size_t a = g2 ? 192 : 96;
  std::vector<uint32_t> off(n_groups + 1);
  size_t npoints, first = 0;
  if (group_offsets) {
    for (size_t g = 0; g < n_groups; g++) if (group_offsets[g + 1] < group_offsets[g]) return NBLS_EINVAL;
    first = group_offsets[0];
    if ((size_t)group_offsets[n_groups] - first > MSMB_MAX_ITEMS) return NBLS_EINVAL;
    pack_rel(off.data(), group_offsets, n_groups);
    npoints = off[n_groups];
  } else {
    if (!n_pts || n_pts > MSMB_MAX_ITEMS || n_groups * n_pts > MSMB_MAX_ITEMS) return NBLS_EINVAL;
    for (size_t g = 0; g <= n_groups; g++) off[g] = (uint32_t)(g * n_pts);
    npoints = n_pts;
  }
  if (off[n_groups] && (!pts || !scalars)) return NBLS_EINVAL;
  // one group IS nbls_g*_msm: the same call, without the staging copy of this pipeline (0.1 ms of a 65,536-point call)
  if (n_groups == 1) return msm_host(ctx, g2, off[1], pts ? pts + first * a : nullptr, scalars ? scalars + first * 32 : nullptr, out, status);
  LOCKED(ctx);
  return msm_batch_pipeline(ctx, g2, n_groups, off, group_offsets ? 0 : n_pts, npoints, pts ? pts + first * a : nullptr, scalars ? scalars + first * 32 : nullptr, out, status);
}
EXPORT int nbls_g1_msm_batch(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* pts96, const uint8_t* scalars32, uint8_t* out96, int8_t* status) {
  if (!group_offsets) return NBLS_EINVAL;
  return msm_batch_host(ctx, false, n_groups, group_offsets, 0, pts96, scalars32, out96, status);
}
EXPORT int nbls_g2_msm_batch(nbls_ctx* ctx, size_t n_groups, const uint32_t* group_offsets, const uint8_t* pts192, const uint8_t* scalars32, uint8_t* out192, int8_t* status) {
  if (!group_offsets) return NBLS_EINVAL;
  return msm_batch_host(ctx, true, n_groups, group_offsets, 0, pts192, scalars32, out192, status);
}
EXPORT int nbls_g1_msm_rows(nbls_ctx* ctx, size_t n_pts, const uint8_t* pts96, size_t n_rows, const uint8_t* scalars32, uint8_t* out96, int8_t* status) {
  return msm_batch_host(ctx, false, n_rows, nullptr, n_pts, pts96, scalars32, out96, status);
}
EXPORT int nbls_g2_msm_rows(nbls_ctx* ctx, size_t n_pts, const uint8_t* pts192, size_t n_rows, const uint8_t* scalars32, uint8_t* out192, int8_t* status) {
  return msm_batch_host(ctx, true, n_rows, nullptr, n_pts, pts192, scalars32, out192, status);
}
