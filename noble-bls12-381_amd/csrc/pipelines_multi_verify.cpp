// pipelines_multi_verify.cpp -- verify(sig_i, m_i, pk_i) (reference index.ts:756-767) for n INDEPENDENT sets, checked together by a random linear combination
// (the MSM's follow-on).  With secret 64-bit weights r_i (rlc_weights.h) every set is valid when
//   prod_i e([r_i]pk_i, H(m_i)) * e(-G1, sum_i [r_i]sig_i) = 1:
// n + 1 Miller loops and ONE final exponentiation where n verify calls spend 2n and n.  An invalid set passes with probability at most 2^-63 over the weights; the weights
// stop the cancellation that beats a plain sum (sig_a + D, sig_b - D).  Where the combined answer does not count -- some set failed to decode, the product is not one, or the
// weighted sum of the signatures is the zero point -- and the caller asked for statuses, a per-set pass judges every set on its own: millerLoop(pk_i, H_i) x millerLoop(-G1, sig_i)
// with the UNWEIGHTED key (P_MILLER_RAW2), n final exponentiations, one byte per set compared with one on the device.
//
// One chain as verify_pipeline builds it: the inputs travel as one copy from the page-locked block, nothing is decided on the host before the combined result is read back
// (with the decoder statuses, in one copy), and the per-set pass is a second chain with a second read-back.
//   s (the call's stream):  H2D copy -> weights -> fork | expand_message_xmd -> hash-to-G2 (H_i)            | join -> Miller loops of n + 1 pairs -> product -> final exp -> read-back
//   side2:                  keys: decompress -> [r_i]pk_i (P_G1_MUL64) -> inversion -> affine  (aggregates: decompress every key or gather it from a key table -> one sum per set
//                           -> affine, then the same)
//   side:                   signatures: decompress -> S = sum_i [r_i]sig_i (G2 MSM with 64-bit scalars; dev_msm synchronises its stream once, after the decoding)
// Scratch slots: chains that run side by side never share one --
//   s: 9 staged inputs, 8 expand_message_xmd output, 0 .. 6 / 11 / 13 / 18 / 19 hash-to-G2 (dev_hash_to_g2), 20 weights, 21 the decoded points, the pairs and what is read back;
//   side2: 14 .. 16 / 17 key decompression, 23 / 24 / 25 the ladder's projective points (+ the affine program's unused statuses), norms and their inverses;
//          nbls_verify_aggregates: 44 .. 47 the per-set key sums before the ladder (dev_aggregate_keys);
//   side: 26 .. 28 / 29 signature decompression, 30 .. 39 / 41 / 43 the MSM (dev_msm slot0 = 30);
//   per-set pass (s, after the read-back): 22 the interleaved pairs, the n final exponentiations and the verdict bytes.
// Shared messages (nbls_verify_multiple_shared and its twins: n sets over m <= n messages, msg_index[i] = the message of set i).  The factors of one message are multiplied together
// by bilinearity, prod_g e(sum_{i in g} [r_i]pk_i, H(m_g)) * e(-G1, S) = 1: m hashes and m + 1 Miller loops.  The hash chain runs over the m messages; side2 goes on from the
// ladder's PROJECTIVE outputs (dev_group_keys): gathered into group order, summed per group by the MSM's list-driven rounds, and only the m sums are inverted and made affine.
//   side2, after the ladder: 48 the gathered points, 49 group ids, ranks, pair lists, counters and statuses in group order, 50 the sums, their norms, inverses and zero flags
//   (slots of their own: the hash chain, the signature chain and -- on side2 itself, earlier -- dev_aggregate_keys keep theirs, and no buffer is regrown under a kernel in flight).
#include "nbls_internal.h"
#include <algorithm>
#include <cerrno>
#include <new>
#include <sys/random.h>

#define LAUNCHCHK(call) do { int e_ = (call); if (e_) { ctx->last_hip = e_; return NBLS_EHIP; } } while (0)

static int os_seed(uint8_t* seed) {
  size_t got = 0;
  while (got < 32) {
    const ssize_t k = getrandom(seed + got, 32 - got, 0);
    if (k < 0) { if (errno == EINTR) continue; return NBLS_ENOSUP; }   // never a fixed seed instead
    got += (size_t)k;
  }
  return NBLS_OK;
}

// The aggregate key of every set (aggregatePublicKeys, index.ts:771-778) on `s` -> PK (affine wire bytes, n x 96) and one status byte per set (STK): the decoder's status of the
// set's first key that does not decode, else 1 when the keys sum to the zero point, else 0.  d_keys: the call's keys (48 B compressed) or indices into agg.ks; d_koff: n + 1 relative
// key offsets.  The sums are the MSM's segmented balanced tree (dev_msm step 2): the keys of a set are contiguous already, so set id and rank stand in for the sorted (window, digit)
// keys, and ceil(log2(largest set)) rounds of pairs + P_G1_ADD_AB leave every set's sum at its first key -- a launch count independent of n.
// Scratch slots 44 (decoded keys), 45 (projective keys), 46 (set ids, ranks, pair lists, counters, statuses), 47 (the aggregates, their norms and inverses), and 14 .. 16 / 17
// for the decompression (side2 of verify_multiple_pipeline).
static int dev_aggregate_keys(nbls_ctx* ctx, size_t n, const AggKeys& agg, const uint8_t* d_keys, const uint32_t* d_koff, uint8_t* PK, int8_t* STK, hipStream_t s) {
  const size_t K = agg.nkeys, p = 3 * RAW;
  uint8_t *KA = nullptr, *KP, *U, *A; int r;
  if ((!agg.ks && (r = need(ctx, 44, K * 97, &KA))) || (r = need(ctx, 45, (K + 1) * p, &KP)) || (r = need(ctx, 46, K * 13 + n * 5 + 32 * 4, &U)) ||
      (r = need(ctx, 47, n * (p + 2 * RAW), &A)))
    return r;
  uint32_t *set_id = (uint32_t*)U, *rank = set_id + K, *list = rank + K, *first = list + K, *counters = first + n;
  int8_t *GST = (int8_t*)(counters + 32), *Z = GST + K;
  uint8_t *N = A + n * p, *NI = N + n * RAW;
  const uint8_t* src;
  const int8_t* st_src;
  if (agg.ks) { src = agg.ks->pts; st_src = agg.ks->st; }
  else {
    // PointG1.fromHex (index.ts:301-326) of every key, then raw projective points (Z = 1; zero keys and keys that did not decode become the identity below)
    int8_t* KST = (int8_t*)(KA + K * 96);
    if ((r = dev_decompress(ctx, false, K, d_keys, KA, KST, s, 14, 17)) || (r = run(ctx, P_G1_TO_PROJ, K, {B(0, KA, 96), B(3, KP, p)}, s))) return r;
    src = KP; st_src = KST;
  }
  LAUNCHCHK(nbls_agg_keys_launch((unsigned)K, (unsigned)n, d_koff, agg.ks ? d_keys : nullptr, st_src, set_id, rank, GST, first, s));
  LAUNCHCHK(nbls_agg_points_launch(K, (unsigned)p, agg.ks ? d_keys : nullptr, GST, ctx->ident_g1, src, KP, s));
  int round = 0;
  for (size_t d = 1; d < agg.maxset; d *= 2, round++) {
    const size_t bound = K / (d + 1) + 1;      // every pair owns d + 1 keys of its own set
    uint32_t* c = counters + round;
    LAUNCHCHK(nbls_msm_pairs_launch(K, (unsigned)d, set_id, rank, list, c, s));
    if ((r = run(ctx, P_G1_ADD_AB, bound, {B(3, KP, p), B(4, KP + d * p, p), B(5, KP, p)}, s, c, list))) return r;
  }
  LAUNCHCHK(nbls_msm_heads_launch(K, (unsigned)p, set_id, KP, A, s));   // A[j] = the sum of set j, left at its first key
  if ((r = run(ctx, P_G1_NORM, n, {B(3, A, p), B(4, N, RAW)}, s)) || (r = run_inv_buf(ctx, n, N, NI, s)) ||
      (r = run(ctx, P_G1_TO_AFFINE, n, {B(3, A, p), B(4, NI, RAW), B(2, PK, 96), B(7, Z, 1)}, s)))
    return r;
  LAUNCHCHK(nbls_agg_status_launch((unsigned)n, first, GST, Z, STK, s));
  return NBLS_OK;
}

// Shared messages: the weighted key of every message group, sum_{i : msg_index[i] = g} [r_i]pk_i, from the ladder's projective outputs Pj (n x 3 RAW, set order) -> RPK (affine
// wire bytes, m x 96).  d_order: the sets sorted by group, d_goff: m + 1 group offsets into it (every group non-empty: checked on the host), STK: the key status of every set.
// agg_keys_kernel gives every position of the sorted list its group, its rank and the status of the set that stands there; agg_points_kernel gathers Pj[order[k]] with the identity
// in place of every set whose key status is not 0 (the sum stays defined; such a call never counts the combined check); then ceil(log2(largest group)) rounds of pairs + P_G1_ADD_AB
// as in dev_aggregate_keys, heads, and norm / inversion / affine over the m sums.  A group that sums to the zero point cannot go into a Miller loop: *d_gzero = 1 and -G1 stands
// in for it (grp_zero_kernel); the caller reads the word back with the statuses and does not count the combined check.
static int dev_group_keys(nbls_ctx* ctx, size_t n, const MsgGroups& mg, const uint32_t* d_order, const uint32_t* d_goff, const int8_t* STK, const uint8_t* Pj, uint8_t* RPK,
                          uint32_t* d_gzero, hipStream_t s) {
  const size_t m = mg.n_msgs, p = 3 * RAW;
  uint8_t *GP, *U, *A; int r;
  if ((r = need(ctx, 48, (n + 1) * p, &GP)) || (r = need(ctx, 49, n * 13 + m * 4 + 32 * 4, &U)) || (r = need(ctx, 50, m * (p + 2 * RAW) + m, &A))) return r;
  uint32_t *grp = (uint32_t*)U, *rank = grp + n, *list = rank + n, *first = list + n, *counters = first + m;
  int8_t* GST = (int8_t*)(counters + 32);
  uint8_t *N = A + m * p, *NI = N + m * RAW, *Z = NI + m * RAW;
  LAUNCHCHK(nbls_agg_keys_launch((unsigned)n, (unsigned)m, d_goff, d_order, STK, grp, rank, GST, first, s));
  LAUNCHCHK(nbls_agg_points_launch(n, (unsigned)p, d_order, GST, ctx->ident_g1, Pj, GP, s));
  int round = 0;
  for (size_t d = 1; d < mg.maxgroup; d *= 2, round++) {
    const size_t bound = n / (d + 1) + 1;      // every pair owns d + 1 positions of its own group
    uint32_t* c = counters + round;
    LAUNCHCHK(nbls_msm_pairs_launch(n, (unsigned)d, grp, rank, list, c, s));
    if ((r = run(ctx, P_G1_ADD_AB, bound, {B(3, GP, p), B(4, GP + d * p, p), B(5, GP, p)}, s, c, list))) return r;
  }
  LAUNCHCHK(nbls_msm_heads_launch(n, (unsigned)p, grp, GP, A, s));   // A[g] = the sum of group g, left at its first position
  if ((r = run(ctx, P_G1_NORM, m, {B(3, A, p), B(4, N, RAW)}, s)) || (r = run_inv_buf(ctx, m, N, NI, s)) ||
      (r = run(ctx, P_G1_TO_AFFINE, m, {B(3, A, p), B(4, NI, RAW), B(2, RPK, 96), B(7, Z, 1)}, s)))
    return r;
  LAUNCHCHK(nbls_grp_zero_launch((unsigned)m, Z, ctx->neg_g1, RPK, d_gzero, s));
  return NBLS_OK;
}

// agg == NULL: nbls_verify_multiple (pks48 = n keys); else nbls_verify_aggregates(_indexed), whose key stage (dev_aggregate_keys) yields one affine key and one status per set: what
// follows the key stage is the same for both.  mg == NULL: one message per set; else msgs / offsets hold mg->n_msgs messages and set i signs message mg->msg_index[i] (nh = the
// number of messages hashed, and of Miller loops beside the signatures')
int verify_multiple_pipeline(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pks48, const AggKeys* agg,
                             const MsgGroups* mg, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  uint8_t seed[32];
  if (seed32) memcpy(seed, seed32, 32);
  else { const int e = os_seed(seed); if (e) return e; }
  const size_t nh = mg ? mg->n_msgs : n;
  for (size_t i = 0; i < nh; i++) if (offsets[i + 1] < offsets[i]) return NBLS_EINVAL;
  // shared messages: one pass over the index validates it and counts every group, a second one sorts the sets by group (counting sort, stable): goff[nh + 1] | order[n]
  std::vector<uint32_t> groups;
  size_t maxgroup = 0;
  if (mg) {
    groups.assign(nh + 1 + n, 0);
    uint32_t *goff = groups.data(), *order = goff + nh + 1;
    for (size_t i = 0; i < n; i++) { if (mg->msg_index[i] >= nh) return NBLS_EINVAL; goff[mg->msg_index[i] + 1]++; }
    for (size_t g = 0; g < nh; g++) {
      if (!goff[g + 1]) return NBLS_EINVAL;   // a message that no set names
      maxgroup = std::max(maxgroup, (size_t)goff[g + 1]);
      goff[g + 1] += goff[g];
    }
    std::vector<uint32_t> at(goff, goff + nh);
    for (size_t i = 0; i < n; i++) order[at[mg->msg_index[i]]++] = (uint32_t)i;
  }
  const size_t total = offsets[nh] - offsets[0];
  uint8_t dst_hash[32];
  if (dst_len > 255) { Sha256 c; c.update((const uint8_t*)"H2C-OVERSIZE-DST-", 17); c.update(dst, dst_len); c.final(dst_hash); dst = dst_hash; dst_len = 32; }
  // the staged block: messages | offsets (relative) | DST | keys | signatures | seed.  Keys: n compressed keys, or (aggregates) the call's compressed keys / table indices followed by
  // the n + 1 key offsets (relative) at o_pk + o_koff
  const size_t o_koff = agg ? ((agg->nkeys * (agg->ks ? 4 : 48) + 15) & ~(size_t)15) : 0, key_bytes = agg ? o_koff + (n + 1) * 4 : n * 48;
  // shared messages: the message index, then the group offsets and the sorted sets, behind the seed
  const size_t o_off = (total + 15) & ~(size_t)15, o_dst = o_off + (((nh + 1) * 4 + 15) & ~(size_t)15), o_pk = o_dst + 256, o_sig = o_pk + ((key_bytes + 15) & ~(size_t)15),
               o_seed = o_sig + n * 96, o_idx = o_seed + 32, o_grp = o_idx + n * 4, in_bytes = mg ? o_grp + (nh + 1 + n) * 4 : o_idx;
  // slot 21: [r_i]pk_i (shared messages: the weighted key of every group) and -G1 | H_i and S | pk_i | sig_i | result (576) | key statuses | signature statuses | MSM status |
  // bad-offsets word | (shared messages) zero-group word
  const size_t o_h = (nh + 1) * 96, o_pkd = o_h + (nh + 1) * 192, o_sgd = o_pkd + n * 96, o_res = o_sgd + n * 192, o_bad = 576 + ((2 * n + 1 + 3) & ~(size_t)3),
               st_bytes = o_bad - 576 + (mg ? 8 : 4), back = 576 + st_bytes;
  LOCKED(ctx);
  StreamOrder order_(ctx, s);
  uint8_t *c, *du, *W, *P, *Pj, *N, *NI = nullptr; int r;
  if ((r = need(ctx, 9, in_bytes, &c)) || (r = need(ctx, 8, nh * 256, &du)) || (r = need(ctx, 20, n * 32, &W)) || (r = need(ctx, 21, o_res + back, &P)) ||
      (r = need(ctx, 23, n * 3 * RAW + n, &Pj)) || (r = need(ctx, 24, n * RAW, &N)) || (!mg && (r = need(ctx, 25, n * RAW, &NI))) || (r = ensure_pinned(ctx, in_bytes)) ||
      (r = ensure_pinned_out(ctx, back)) || (r = ensure_scratch(ctx, n + 1)) || (r = ensure_side(ctx)) || (r = ensure_side2(ctx)))
    return r;
  if (!ctx->ev_fork && hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); return NBLS_EHIP; }
  uint8_t *RPK = P, *H = P + o_h, *PK = P + o_pkd, *SG = P + o_sgd, *O = P + o_res, *STK = O + 576, *STS = STK + n, *MS = STS + n;
  uint32_t* d_bad = (uint32_t*)(O + o_bad);
  uint8_t* pin = ctx->pinned;
  if (total) memcpy(pin, msgs + offsets[0], total);
  { uint32_t* rel = (uint32_t*)(pin + o_off); for (size_t i = 0; i <= nh; i++) rel[i] = offsets[i] - offsets[0]; }
  if (mg) { memcpy(pin + o_idx, mg->msg_index, n * 4); memcpy(pin + o_grp, groups.data(), groups.size() * 4); }
  memcpy(pin + o_dst, dst, dst_len); memcpy(pin + o_sig, sigs96, n * 96); memcpy(pin + o_seed, seed, 32);
  if (!agg) memcpy(pin + o_pk, pks48, n * 48);
  else {
    const uint32_t k0 = agg->key_offsets[0];
    if (agg->ks) memcpy(pin + o_pk, agg->key_index + k0, agg->nkeys * 4);
    else memcpy(pin + o_pk, agg->pks48 + (size_t)k0 * 48, agg->nkeys * 48);
    uint32_t* rel = (uint32_t*)(pin + o_pk + o_koff);
    for (size_t j = 0; j <= n; j++) rel[j] = agg->key_offsets[j] - k0;
  }
  ForkGuard fork_guard;   // from the first asynchronous copy on: an error return waits for every stream of the call
  HIPCHK(hipMemcpyAsync(c, pin, in_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_bad, 0, mg ? 8 : 4, s));
  if (nbls_rlc_weights_launch((unsigned)n, c + o_seed, W, s)) { ctx->last_hip = (int)hipGetLastError(); return NBLS_EHIP; }
  HIPCHK(hipEventRecord(ctx->ev_fork, s));
  // signatures (side): PointG2.fromSignature, index.ts:500-530
  HIPCHK(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  if ((r = dev_decompress(ctx, true, n, c + o_sig, SG, STS, ctx->side, 26, 29))) return r;
  // keys (side2): PointG1.fromHex, index.ts:301-326 (aggregates: of every key, then one sum per set), then [r_i]pk_i
  HIPCHK(hipStreamWaitEvent(ctx->side2, ctx->ev_fork, 0));
  if (!agg) { if ((r = dev_decompress(ctx, false, n, c + o_pk, PK, STK, ctx->side2, 14, 17))) return r; }
  else if ((r = dev_aggregate_keys(ctx, n, *agg, c + o_pk, (const uint32_t*)(c + o_pk + o_koff), PK, (int8_t*)STK, ctx->side2))) return r;
  if ((r = run(ctx, P_G1_MUL64, n, {B(0, PK, 96), B(2, W, 32), B(3, Pj, 3 * RAW), B(4, N, RAW)}, ctx->side2))) return r;
  if (mg) {
    const uint32_t* d_goff = (const uint32_t*)(c + o_grp);
    if ((r = dev_group_keys(ctx, n, MsgGroups{nh, mg->msg_index, maxgroup}, d_goff + nh + 1, d_goff, (const int8_t*)STK, Pj, RPK, d_bad + 1, ctx->side2))) return r;
  } else {
    if ((r = run_inv_buf(ctx, n, N, NI, ctx->side2))) return r;
    if ((r = run(ctx, P_G1_TO_AFFINE, n, {B(3, Pj, 3 * RAW), B(4, NI, RAW), B(2, RPK, 96), B(7, Pj + n * 3 * RAW, 1)}, ctx->side2))) return r;
  }
  HIPCHK(hipEventRecord(ctx->ev_join2, ctx->side2));
  // messages (s): expand_message_xmd, PointG2.hashToCurve (index.ts:481-490)
  { const int e = nbls_xmd_launch((unsigned)nh, c, c + o_off, c + o_dst, (unsigned)dst_len, du, 256, d_bad, s); if (e) { ctx->last_hip = e; return NBLS_EHIP; } }
  if ((r = dev_hash_to_g2(ctx, nh, du, H, s))) return r;
  // S = sum_i [r_i]sig_i behind the signatures on the side stream (enqueued last: dev_msm waits on the host for its stream once, with the hash chain and the keys in flight)
  if ((r = dev_msm(ctx, true, n, SG, W, 64, H + nh * 192, MS, ctx->side, 30))) return r;
  HIPCHK(hipEventRecord(ctx->ev_join, ctx->side));
  HIPCHK(hipStreamWaitEvent(s, ctx->ev_join2, 0));
  HIPCHK(hipStreamWaitEvent(s, ctx->ev_join, 0));
  HIPCHK(hipMemcpyAsync(RPK + nh * 96, ctx->neg_g1, 96, hipMemcpyDeviceToDevice, s));   // PointG1.BASE.negate()
  size_t m = 0;
  uint8_t* res = ctx->F;
  if ((r = miller_values(ctx, nh + 1, RPK, H, &m, s)) || (r = reduce_product(ctx, m, &res, s)) || (r = finish_single(ctx, res, 1, O, s))) return r;
  HIPCHK(hipMemcpyAsync(ctx->pinned_out, O, back, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  fork_guard.armed = false;      // synchronised: both side streams were joined into s
  std::vector<uint8_t> rb(ctx->pinned_out, ctx->pinned_out + back);
  uint32_t bad = 0, gzero = 0; memcpy(&bad, rb.data() + o_bad, 4);
  if (bad) return NBLS_EINVAL;
  if (mg) memcpy(&gzero, rb.data() + o_bad + 4, 4);
  const int8_t *stk = (const int8_t*)rb.data() + 576, *sts = stk + n;
  bool decoded = sts[n] == 0 && !gzero;   // (the MSM's status: 1 = the weighted sum is the zero point; gzero: some message group's weighted keys sum to it)
  for (size_t i = 0; i < n && decoded; i++) if (stk[i] || sts[i]) decoded = false;
  if (decoded && fp12_wire_is_one(rb.data())) {
    *all_ok = 1;
    if (status) memset(status, 0, n);
    return NBLS_OK;
  }
  *all_ok = 0;
  if (!status) return NBLS_OK;     // fast reject: no per-set work
  // the per-set pass, on the unweighted keys: millerLoop(pk_i, H_i) x millerLoop(-G1, sig_i), final exponentiation, compared with one on the device
  uint8_t *X;
  if ((r = need(ctx, 22, n * (192 + 384 + 576) + n, &X))) return r;
  uint8_t *G1x = X, *G2x = G1x + n * 192, *E = G2x + n * 384, *V = E + n * 576;
  if (mg ? nbls_grp_interleave_launch((unsigned)n, c + o_idx, PK, ctx->neg_g1, H, SG, G1x, G2x, s) : nbls_rlc_interleave_launch((unsigned)n, PK, ctx->neg_g1, H, SG, G1x, G2x, s)) {
    ctx->last_hip = (int)hipGetLastError(); return NBLS_EHIP;
  }
  if ((r = run(ctx, P_MILLER_RAW2, n, {B(0, G1x, 192), B(1, G2x, 384), B(3, ctx->F, F12)}, s)) || (r = run(ctx, P_NORM_RAW, n, {B(3, ctx->F, F12), B(4, ctx->N, RAW)}, s)) ||
      (r = final_exp_pipeline(ctx, n, ctx->F, E, s)))
    return r;
  if (nbls_rlc_is_one_launch((unsigned)n, E, V, s)) { ctx->last_hip = (int)hipGetLastError(); return NBLS_EHIP; }
  if ((r = ensure_pinned_out(ctx, n))) return r;
  HIPCHK(hipMemcpyAsync(ctx->pinned_out, V, n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int all = 1;
  for (size_t i = 0; i < n; i++) {
    // the reference's order (oracle_verify): the key decodes, the message hashes, the signature decodes, the pairing throws on a zero point ("No pairings at point of Infinity")
    const int8_t k = stk[i], g = sts[i];
    const int8_t v = k >= 2 ? k : g >= 2 ? (int8_t)(10 + g) : k == 1 ? 1 : g == 1 ? 11 : ctx->pinned_out[i] ? 0 : NBLS_ST_NOT_VERIFIED;
    status[i] = v;
    if (v) all = 0;
  }
  *all_ok = all;
  return NBLS_OK;
}

EXPORT int nbls_verify_multiple(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pks48, const uint8_t* dst, size_t dst_len,
                                const uint8_t* seed32, int* all_ok, int8_t* status) {
  std::lock_guard<std::recursive_mutex> whole_call_(ctx ? ctx->mu : g_null_mu);   // scratch and I/O staging buffers belong to this call until it returns
  if (!ctx || !all_ok || !n || !sigs96 || !offsets || !pks48 || !dst || (!msgs && offsets[n] != offsets[0])) return NBLS_EINVAL;
  if (n > ((size_t)1 << 22)) return NBLS_EINVAL;   // dev_msm's bound
  return verify_multiple_pipeline(ctx, n, sigs96, msgs, offsets, pks48, nullptr, nullptr, dst, dst_len, seed32, all_ok, status);
}

// ---- aggregates: verify(sig_j, m_j, aggregatePublicKeys(keys_j)) (index.ts:756-778) for n sets, one random linear combination over the sets
static const size_t AGG_MAX_KEYS = (size_t)1 << 24;   // keys per call (u32 set ids and ranks, at most 24 rounds of the segmented sum)
// the key offsets: non-decreasing, no empty set (the reference's aggregatePublicKeys throws "Expected non-empty array"), at most AGG_MAX_KEYS keys; every index inside the table
static int agg_check(size_t n, const uint32_t* key_offsets, const uint32_t* key_index, const nbls_keyset* ks, AggKeys* agg) {
  size_t maxset = 0;
  for (size_t j = 0; j < n; j++) {
    if (key_offsets[j + 1] <= key_offsets[j]) return NBLS_EINVAL;
    maxset = std::max(maxset, (size_t)(key_offsets[j + 1] - key_offsets[j]));
  }
  const size_t K = key_offsets[n] - key_offsets[0];
  if (K > AGG_MAX_KEYS) return NBLS_EINVAL;
  if (ks) for (size_t k = key_offsets[0]; k < key_offsets[n]; k++) if (key_index[k] >= ks->n) return NBLS_EINVAL;
  agg->nkeys = K; agg->maxset = maxset; agg->key_offsets = key_offsets; agg->ks = ks; agg->key_index = key_index;
  return NBLS_OK;
}
EXPORT int nbls_verify_aggregates(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pks48, const uint32_t* key_offsets,
                                  const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  std::lock_guard<std::recursive_mutex> whole_call_(ctx ? ctx->mu : g_null_mu);
  if (!ctx || !all_ok || !n || !sigs96 || !offsets || !pks48 || !key_offsets || !dst || (!msgs && offsets[n] != offsets[0])) return NBLS_EINVAL;
  if (n > ((size_t)1 << 22)) return NBLS_EINVAL;   // dev_msm's bound
  AggKeys agg;
  int r = agg_check(n, key_offsets, nullptr, nullptr, &agg); if (r) return r;
  agg.pks48 = pks48;
  return verify_multiple_pipeline(ctx, n, sigs96, msgs, offsets, nullptr, &agg, nullptr, dst, dst_len, seed32, all_ok, status);
}
EXPORT int nbls_verify_aggregates_indexed(nbls_ctx* ctx, const nbls_keyset* ks, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* key_index,
                                          const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  std::lock_guard<std::recursive_mutex> whole_call_(ctx ? ctx->mu : g_null_mu);
  if (!ctx || !ks || !all_ok || !n || !sigs96 || !offsets || !key_index || !key_offsets || !dst || (!msgs && offsets[n] != offsets[0])) return NBLS_EINVAL;
  if (n > ((size_t)1 << 22) || ks->device != ctx->device) return NBLS_EINVAL;   // the table lives in the memory of the device it was created on
  AggKeys agg;
  int r = agg_check(n, key_offsets, key_index, ks, &agg); if (r) return r;
  return verify_multiple_pipeline(ctx, n, sigs96, msgs, offsets, nullptr, &agg, nullptr, dst, dst_len, seed32, all_ok, status);
}

// ---- shared messages: the three calls above for n sets over n_msgs <= n messages, msg_index[i] = the message of set i; the index itself is validated in the pipeline's one pass
#define SHARED_ARGS_BAD (!ctx || !all_ok || !n || !sigs96 || !offsets || !msg_index || !dst || !n_msgs || n_msgs > n || n > ((size_t)1 << 22) || (!msgs && offsets[n_msgs] != offsets[0]))
EXPORT int nbls_verify_multiple_shared(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* msg_index,
                                       const uint8_t* pks48, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  std::lock_guard<std::recursive_mutex> whole_call_(ctx ? ctx->mu : g_null_mu);
  if (SHARED_ARGS_BAD || !pks48) return NBLS_EINVAL;
  const MsgGroups mg{n_msgs, msg_index, 0};
  return verify_multiple_pipeline(ctx, n, sigs96, msgs, offsets, pks48, nullptr, &mg, dst, dst_len, seed32, all_ok, status);
}
EXPORT int nbls_verify_aggregates_shared(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* msg_index,
                                         const uint8_t* pks48, const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  std::lock_guard<std::recursive_mutex> whole_call_(ctx ? ctx->mu : g_null_mu);
  if (SHARED_ARGS_BAD || !pks48 || !key_offsets) return NBLS_EINVAL;
  AggKeys agg;
  int r = agg_check(n, key_offsets, nullptr, nullptr, &agg); if (r) return r;
  agg.pks48 = pks48;
  const MsgGroups mg{n_msgs, msg_index, 0};
  return verify_multiple_pipeline(ctx, n, sigs96, msgs, offsets, nullptr, &agg, &mg, dst, dst_len, seed32, all_ok, status);
}
EXPORT int nbls_verify_aggregates_indexed_shared(nbls_ctx* ctx, const nbls_keyset* ks, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets,
                                                 const uint32_t* msg_index, const uint32_t* key_index, const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len,
                                                 const uint8_t* seed32, int* all_ok, int8_t* status) {
  std::lock_guard<std::recursive_mutex> whole_call_(ctx ? ctx->mu : g_null_mu);
  if (SHARED_ARGS_BAD || !ks || !key_index || !key_offsets || ks->device != ctx->device) return NBLS_EINVAL;
  AggKeys agg;
  int r = agg_check(n, key_offsets, key_index, ks, &agg); if (r) return r;
  const MsgGroups mg{n_msgs, msg_index, 0};
  return verify_multiple_pipeline(ctx, n, sigs96, msgs, offsets, nullptr, &agg, &mg, dst, dst_len, seed32, all_ok, status);
}

// The key table: PointG1.fromHex (index.ts:298-327) of every key once, kept as raw projective points with the identity in place of zero keys and keys that did not decode, and the
// decoder's status of every key (which nbls_verify_aggregates_indexed reports for a set that names the key).  Owns its device memory: usable from any context on the same device,
// and after the creating context is destroyed.
EXPORT int nbls_keyset_create(nbls_ctx* ctx, size_t n, const uint8_t* pks48, int8_t* status, nbls_keyset** out) {
  std::lock_guard<std::recursive_mutex> whole_call_(ctx ? ctx->mu : g_null_mu);
  if (!ctx || !n || !pks48 || !out || n > AGG_MAX_KEYS) return NBLS_EINVAL;
  *out = nullptr;
  LOCKED(ctx);
  HostIO io{ctx};
  void *d = io.alloc(n * 48), *a = io.alloc(n * 96);
  if (!d || !a) return NBLS_EHIP;
  nbls_keyset* ks = new (std::nothrow) nbls_keyset;
  if (!ks) return NBLS_EHIP;
  ks->device = ctx->device; ks->n = n;
  uint8_t* mem = nullptr;
  if (hipMalloc(&mem, n * 3 * RAW + n) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); delete ks; return NBLS_EHIP; }
  ks->pts = mem; ks->st = (int8_t*)(mem + n * 3 * RAW);
  int r = NBLS_OK;
  hipError_t e = hipMemcpyAsync(d, pks48, n * 48, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && !(r = dev_decompress(ctx, false, n, d, a, ks->st, s)) && !(r = run(ctx, P_G1_TO_PROJ, n, {B(0, a, 96), B(3, ks->pts, 3 * RAW)}, s))) {
    const int k = nbls_agg_points_launch(n, (unsigned)(3 * RAW), nullptr, ks->st, ctx->ident_g1, ks->pts, ks->pts, s);
    if (k) { ctx->last_hip = k; r = NBLS_EHIP; }
    else if (status) e = hipMemcpyAsync(status, ks->st, n, hipMemcpyDeviceToHost, s);
    if (!r && e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) { ctx->last_hip = (int)e; r = NBLS_EHIP; }
  if (r) { (void)hipStreamSynchronize(s); hipFree(mem); delete ks; return r; }
  *out = ks;
  return NBLS_OK;
}
EXPORT void nbls_keyset_destroy(nbls_keyset* ks) {
  if (!ks) return;
  int cur = 0;
  const bool restore = hipGetDevice(&cur) == hipSuccess;
  if (hipSetDevice(ks->device) == hipSuccess) (void)hipFree(ks->pts);
  if (restore) (void)hipSetDevice(cur);
  delete ks;
}
EXPORT int nbls_keyset_size(const nbls_keyset* ks, size_t* n) {
  if (!ks || !n) return NBLS_EINVAL;
  *n = ks->n;
  return NBLS_OK;
}
