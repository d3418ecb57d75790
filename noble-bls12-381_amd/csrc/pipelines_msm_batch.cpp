// pipelines_msm_batch.cpp -- many independent multi-scalar multiplications in one call (nbls_g*_msm_batch: groups of one point / scalar array; nbls_g*_msm_rows: many scalar
// vectors against one set of points).  dev_msm (pipelines_codec.cpp) is built for ONE large sum: fixed 12-bit windows, 12 * 2^11 gathered bucket points per window whatever n
// is, a single-point tail and a synchronisation per call.  Here the sums share every launch, and the window width fits their size.  One chain on the call's stream:
//   H2D copy -> all points to raw projective form and all scalars split along the endomorphisms ONCE (P_G*_MSM_PREP + msm_decompose, or P_G*_TO_PROJ when every scalar of the
//               call is below 2^192)
//            -> per slab of whole groups: keys (group, window, digit) with run-time width c (msmb_kernels.hip) -> radix sort over the true number of key bits -> gather -> ranks
//               -> segmented sum (P_G*_ADD_AB through the pair lists) -> heads into the buckets -> bit-slices T_t of every (group, window) -> c - 1 rounds of P_G*_ADD2
//               -> ONE doubling-and-add chain over the bit positions: slice t of window w weighs 2^(c w + t), so every group's sum is sum_j 2^j T_(g, j) whatever c is:
//               acc <- 2 acc + T_j from the top bit down (programs.h XP_DBLADD_G*), all groups of the slab the items of each launch -> to_affine into the output block
//            -> a group above the cut-off (NBLS_TUNE_MSMB_BIG) runs through dev_msm between the slabs, and so does a call of one group: 12 bits and the wide tail are right there
//            -> D2H copy
// The key is at the same time the index of its bucket: (group * nwin + window) << c | digit, in 32 bits -- a slab holds at most 2^(32 - c) / nwin groups.  Two neighbouring
// groups with equal digits therefore never share a run.  Scratch: SB_MSMB_CALL and SB_MSMB_SLAB (nbls_internal.h), both sized before the first launch.
// Three parts: the plan (msmb_plan: host arithmetic only), the device core (msmb_run: every launch from the keys to to-affine, on converted points and scalars that are on the
// device) and the staging of the host-buffer calls around them.  msm_rows_dev is the core for callers whose scalars never were on the host (pipelines_kzg_prove.cpp).
#include "nbls_internal.h"
#include <algorithm>

static const size_t MSMB_MAX_ITEMS = (size_t)1 << 22, MSMB_MAX_GROUPS = (size_t)1 << 20;
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
// form) -> O: one affine sum per group, OST: its zero flag
static int msmb_run(nbls_ctx* ctx, const MsmbPlan& pl, const uint32_t* off, const uint8_t* Pj, const uint8_t* d_k, const uint8_t* d_pts, const uint32_t* d_off, uint8_t* O, uint8_t* OST,
                    hipStream_t s) {
  const bool g2 = pl.g2, split = pl.split;
  const size_t a = g2 ? 192 : 96, p = g2 ? 6 * RAW : 3 * RAW, n_groups = pl.n_groups, n_pts = pl.n_pts, nwin = pl.nwin, J = pl.J, jtop = pl.jtop;
  const unsigned dims = pl.dims, c = pl.c;
  const ExtraProg xp = g2 ? XP_DBLADD_G2 : XP_DBLADD_G1;
  const uint8_t* ident = g2 ? ctx->ident_g2 : ctx->ident_g1;
  uint8_t *SL = pl.SL, *Ks = pl.Ks; int r;
  uint32_t *counters = (uint32_t*)(SL + pl.s_cnt);   // [0] longest run, [1 + round] pairs of that round
  uint8_t *tmp = SL + pl.s_tmp, *P = SL + pl.s_P, *Bk = SL + pl.s_bk, *G = SL + pl.s_G, *Gh = SL + pl.s_Gh, *acc = SL + pl.s_acc, *Nm = SL + pl.s_N, *NI = SL + pl.s_NI;
  const DevProgram& step = ctx->extra[xp];
  for (const MsmbPart& pt : pl.parts) {
    const size_t g0 = pt.g0, ngs = pt.g1 - pt.g0, i0 = off[pt.g0], cnt = off[pt.g1] - i0;
    if (pt.big) {
      // (dev_msm synchronises the stream for its own longest run; its scratch is the main slots, which hold nothing of this call)
      if ((r = dev_msm(ctx, g2, cnt, n_pts ? d_pts : d_pts + i0 * a, d_k + i0 * 32, pl.nbits, O + g0 * a, OST + g0, s))) return r;
      continue;
    }
    const size_t m = cnt * dims, M = m * nwin, nbw = ngs * nwin, nb = nbw << c, ng = (nbw * c) << (c - 1);
    LAUNCHCHK(nbls_msm_fill_launch(ngs, (unsigned)p, ident, acc, s));
    if (M) {
      uint32_t *kin = (uint32_t*)SL, *vin = kin + M, *kout = vin + M, *vout = kout + M, *pos = vout + M, *list = pos + M;
      LAUNCHCHK(nbls_msm_fill_launch(nb, (unsigned)p, ident, Bk, s));
      LAUNCHCHK(nbls_msmb_keys_launch((unsigned)m, dims, (unsigned)nwin, c, (unsigned)i0, (unsigned)g0, (unsigned)n_groups, (unsigned)n_pts, d_off, split ? Ks : d_k, kin, vin, s));
      size_t sb = pl.sort_bytes, cb = pl.scan_bytes;
      LAUNCHCHK(nbls_msm_sort_launch(tmp, &sb, kin, kout, vin, vout, M, pt.key_bits, s));
      LAUNCHCHK(nbls_msm_gather_launch(M, (unsigned)p, vout, Pj, P, s));
      LAUNCHCHK(nbls_msm_rank_launch(tmp, &cb, M, kout, pos, counters, s));
      size_t maxg = 0; for (size_t g = pt.g0; g < pt.g1; g++) maxg = std::max(maxg, (size_t)(off[g + 1] - off[g]) * dims);
      uint32_t maxrun = (uint32_t)maxg;      // a run lies inside one window of one group
      if (maxg > MSMB_NO_READBACK) { HIPCHK(hipMemcpyAsync(&maxrun, counters, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
      if ((r = segmented_sum(ctx, g2, M, kout, pos, list, counters + 1, P, maxrun, s))) return r;
      LAUNCHCHK(nbls_msm_heads_launch(M, (unsigned)p, kout, P, Bk, s));
      LAUNCHCHK(nbls_msmb_bitsel_launch(nbw, c, (unsigned)p, Bk, G, s));
      uint8_t *src = G, *dst = Gh;
      for (size_t k = ng; k > nbw * c; k /= 2) {
        if ((r = run(ctx, g2 ? P_G2_ADD2 : P_G1_ADD2, k / 2, {B(3, src, 2 * p), B(5, dst, p)}, s))) return r;
        std::swap(src, dst);
      }
      // src: T[g * J + j], the slice of bit position j of group g
      for (size_t j = jtop; j-- > 0;)
        if ((r = run_dev(ctx, step, -1, ngs, {B(3, acc, p), B(4, src + j * p, J * p)}, s, nullptr, nullptr))) return r;
    }
    if ((r = to_affine(ctx, g2, ngs, acc, Nm, NI, O + g0 * a, OST + g0, s))) return r;
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
  if (pl.maxM) {
    if (split) {
      if ((r = run(ctx, g2 ? P_G2_MSM_PREP : P_G1_MSM_PREP, npoints, {B(g2 ? 1 : 0, d_pts, a), B(3, Pj, dims * p)}, s))) return r;
      LAUNCHCHK(nbls_msm_decompose_launch((unsigned)N, dims, d_k, pl.Ks, s));
    } else if ((r = run(ctx, g2 ? P_G2_TO_PROJ : P_G1_TO_PROJ, npoints, {B(g2 ? 1 : 0, d_pts, a), B(3, Pj, p)}, s))) return r;
  }
  if ((r = msmb_run(ctx, pl, off.data(), Pj, d_k, d_pts, d_off, O, OST, s))) return r;
  if ((r = io.fetch(O, back, &res))) return r;
  memcpy(out, res, n_groups * a);
  // the zero point has no affine form: P_G*_TO_AFFINE multiplies by the inverse of a Z that is 0 mod p, and which representative of 0 the chain before it left there (dev_msm's
  // one-limb-per-lane combine leaves p) decides what the binary GCD returns for it.  The contract is all-zero bytes
  const uint8_t* zero = res + n_groups * a;
  for (size_t g = 0; g < n_groups; g++) if (zero[g]) memset(out + g * a, 0, a);
  if (status) memcpy(status, zero, n_groups);
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
  std::vector<uint32_t> off(pl.n_groups + 1);
  for (size_t g = 0; g <= pl.n_groups; g++) off[g] = (uint32_t)(g * pl.n_pts);
  LAUNCHCHK(nbls_msm_decompose_launch((unsigned)(pl.n_groups * pl.n_pts), pl.dims, d_scalars, pl.Ks, s));
  return msmb_run(ctx, pl, off.data(), conv_pts, d_scalars, nullptr, nullptr, d_out96, d_zero, s);
}

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
