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
// Scratch slots: chains that run side by side never share one (nbls_internal.h, enum Slot and the static_asserts behind it).
// Shared messages (nbls_verify_multiple_shared and its twins: n sets over m <= n messages, msg_index[i] = the message of set i).  The factors of one message are multiplied together
// by bilinearity, prod_g e(sum_{i in g} [r_i]pk_i, H(m_g)) * e(-G1, S) = 1: m hashes and m + 1 Miller loops.  The hash chain runs over the m messages; side2 goes on from the
// ladder's PROJECTIVE outputs (group_keys): gathered into group order, summed per group by the MSM's list-driven rounds, and only the m sums are inverted and made affine.
#include "nbls_internal.h"
#include <algorithm>
#include <cerrno>
#include <new>
#include <sys/random.h>

int os_seed(uint8_t* seed) {   // 32 bytes from getrandom(2): the seed of the secret weights when the caller passes none
  size_t got = 0;
  while (got < 32) {
    const ssize_t k = getrandom(seed + got, 32 - got, 0);
    if (k < 0) { if (errno == EINTR) continue; return NBLS_ENOSUP; }   // never a fixed seed instead
    got += (size_t)k;
  }
  return NBLS_OK;
}
int rlc_seed(const uint8_t* seed32, uint8_t* seed) {   // every weighted verifier's first step (this file, pipelines_kzg*.cpp, pipelines_groth16.cpp)
  if (!seed32) return os_seed(seed);
  memcpy(seed, seed32, 32);
  return NBLS_OK;
}

// One sum per segment, as affine wire bytes (G1: 96 B, G2: 192 B): `count` positions in `nseg` contiguous segments (d_off: nseg + 1 offsets), position k holding the point
// src[index ? index[k] : k] (raw projective) with status st_src[the same].  agg_keys_kernel gives every position its segment, its rank and its status, and every segment its first
// position whose status is >= 2; agg_points_kernel gathers the points with the identity in place of those whose status is not 0 (the sum stays defined); the segments are
// contiguous, so segment id and rank stand in for the MSM's sorted (window, digit) keys, and ceil(log2(maxseg)) rounds of segmented_sum leave every sum at its segment's first
// position -- a launch count independent of the sizes; then heads, norm / inversion / affine over the nseg sums -> out.  What the caller's closing status kernel reads comes back
// in `o` (SegSums, nbls_internal.h).  Callers: the key sums of the multi-verify calls below (G1) and the recombination of threshold shares (pipelines_threshold.cpp, G1 and G2).
int segment_sums(nbls_ctx* ctx, bool g2, const SegSlots& sl, size_t count, size_t nseg, const uint32_t* d_off, const uint32_t* d_index, const uint8_t* src, const int8_t* st_src,
                 size_t maxseg, uint8_t* out, SegSums* o, hipStream_t s) {
  const size_t p = (g2 ? 6 : 3) * RAW;
  uint8_t *GP, *U, *A; int r;
  if ((r = need(ctx, sl.points, (count + 1) * p, &GP)) || (r = need(ctx, sl.labels, count * 13 + nseg * 4 + 32 * 4 + (sl.zero_with_sums ? 0 : nseg), &U)) ||
      (r = need(ctx, sl.sums, nseg * (p + 2 * RAW) + (sl.zero_with_sums ? nseg : 0), &A)))
    return r;
  uint32_t *id = (uint32_t*)U, *rank = id + count, *list = rank + count, *first = list + count, *counters = first + nseg;
  int8_t* GST = (int8_t*)(counters + 32);
  uint8_t *N = A + nseg * p, *NI = N + nseg * RAW, *Z = sl.zero_with_sums ? NI + nseg * RAW : (uint8_t*)GST + count;
  LAUNCHCHK(nbls_agg_keys_launch((unsigned)count, (unsigned)nseg, d_off, d_index, st_src, id, rank, GST, first, s));
  LAUNCHCHK(nbls_agg_points_launch(count, (unsigned)p, d_index, GST, g2 ? ctx->ident_g2 : ctx->ident_g1, src, GP, s));
  if ((r = segmented_sum(ctx, g2, count, id, rank, list, counters, GP, maxseg, s))) return r;
  LAUNCHCHK(nbls_msm_heads_launch(count, (unsigned)p, id, GP, A, s));   // A[j] = the sum of segment j, left at its first position
  *o = {first, GST, Z};
  return to_affine(ctx, g2, nseg, A, N, NI, out, Z, s);
}

// The aggregate key of every set (aggregatePublicKeys, index.ts:771-778) on `s` -> PK (affine wire bytes, n x 96) and one status byte per set (STK): the decoder's status of the
// set's first key that does not decode, else 1 when the keys sum to the zero point, else 0.  d_keys: the call's keys (48 B compressed) or indices into agg.ks; d_koff: n + 1 relative
// key offsets.
static int aggregate_keys(nbls_ctx* ctx, size_t n, const AggKeys& agg, const uint8_t* d_keys, const uint32_t* d_koff, uint8_t* PK, int8_t* STK, hipStream_t s) {
  const size_t K = agg.nkeys, p = 3 * RAW;
  const uint8_t* src = agg.ks ? agg.ks->pts : nullptr;
  const int8_t* st_src = agg.ks ? agg.ks->st : nullptr;
  int r;
  if (!agg.ks) {
    // PointG1.fromHex (index.ts:301-326) of every key, then raw projective points (Z = 1; zero keys and keys that did not decode become the identity in segment_sums, which
    // gathers in place)
    uint8_t *KA, *KP;
    if ((r = need(ctx, SB_AGG_DECODED, K * 97, &KA)) || (r = need(ctx, SEG_AGG.points, (K + 1) * p, &KP))) return r;
    int8_t* KST = (int8_t*)(KA + K * 96);
    if ((r = dev_decompress(ctx, false, K, d_keys, KA, KST, s, DEC_KEYS)) || (r = run(ctx, P_G1_TO_PROJ, K, {B(0, KA, 96), B(3, KP, p)}, s))) return r;
    src = KP; st_src = KST;
  }
  SegSums o;
  if ((r = segment_sums(ctx, false, SEG_AGG, K, n, d_koff, agg.ks ? (const uint32_t*)d_keys : nullptr, src, st_src, agg.maxset, PK, &o, s))) return r;
  LAUNCHCHK(nbls_agg_status_launch((unsigned)n, o.first, o.st, o.zero, STK, s));
  return NBLS_OK;
}

// Shared messages: the weighted key of every message group, sum_{i : msg_index[i] = g} [r_i]pk_i, from the ladder's projective outputs Pj (n x 3 RAW, set order) -> RPK (affine
// wire bytes, m x 96).  d_order: the sets sorted by group, d_goff: m + 1 group offsets into it (every group non-empty: checked on the host), STK: the key status of every set (a
// set whose status is not 0 adds the identity; such a call never counts the combined check).  A group that sums to the zero point cannot go into a Miller loop: *d_gzero = 1 and
// -G1 stands in for it (agg_fix_zero_kernel); the caller reads the word back with the statuses and does not count the combined check.
static int group_keys(nbls_ctx* ctx, size_t n, size_t m, size_t maxgroup, const uint32_t* d_order, const uint32_t* d_goff, const int8_t* STK, const uint8_t* Pj, uint8_t* RPK,
                      uint32_t* d_gzero, hipStream_t s) {
  SegSums o;
  const int r = segment_sums(ctx, false, SEG_GRP, n, m, d_goff, d_order, Pj, STK, maxgroup, RPK, &o, s); if (r) return r;
  LAUNCHCHK(nbls_agg_fix_zero_launch((unsigned)m, o.zero, ctx->neg_g1, RPK, d_gzero, s));
  return NBLS_OK;
}

// in.agg == NULL: nbls_verify_multiple (pks48 = n keys); else nbls_verify_aggregates(_indexed), whose key stage (aggregate_keys) yields one affine key and one status per set: what
// follows the key stage is the same for both.  in.mg == NULL: one message per set; else msgs / offsets hold mg->n_msgs messages and set i signs message mg->msg_index[i] (nh = the
// number of messages hashed, and of Miller loops beside the signatures')
int verify_multiple_pipeline(nbls_ctx* ctx, const MultiVerifyIn& in, int* all_ok, int8_t* status) {
  const size_t n = in.n; const uint32_t* offsets = in.offsets; const AggKeys* agg = in.agg; const MsgGroups* mg = in.mg;
  uint8_t seed[32];
  const int e = rlc_seed(in.seed32, seed); if (e) return e;
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
  // the staged block: messages | offsets (relative) | DST | keys | key offsets | signatures | seed | message index | groups.  Keys: n compressed keys, or (aggregates) the call's
  // compressed keys / table indices and the n + 1 key offsets (relative); shared messages: the message index, then the group offsets and the sorted sets
  // SB_RLC_PAIRS: [r_i]pk_i (shared messages: the weighted key of every group) and -G1 | H_i and S | pk_i | sig_i | result (576) | key statuses | signature statuses | MSM status |
  // bad-offsets word | (shared messages) zero-group word
  const size_t o_h = (nh + 1) * 96, o_pkd = o_h + (nh + 1) * 192, o_sgd = o_pkd + n * 96, o_res = o_sgd + n * 192, o_bad = 576 + ((2 * n + 1 + 3) & ~(size_t)3),
               st_bytes = o_bad - 576 + (mg ? 8 : 4), back = 576 + st_bytes;
  DEV_ENTER(ctx, nullptr);
  Staged io(ctx, s);
  const uint32_t k0 = agg ? agg->key_offsets[0] : 0;
  const size_t o_msg = io.bytes(total ? in.msgs + offsets[0] : nullptr, total), o_off = io.rel(offsets, nh), o_dst = io.dst(in.dst, in.dst_len),
               o_pk = !agg ? io.bytes(in.pks48, n * 48) : agg->ks ? io.bytes(agg->key_index + k0, agg->nkeys * 4) : io.bytes(in.pks48 + (size_t)k0 * 48, agg->nkeys * 48),
               o_koff = agg ? io.rel(agg->key_offsets, n) : 0, o_sig = io.bytes(in.sigs96, n * 96), o_seed = io.bytes(seed, 32),
               o_idx = io.bytes(mg ? mg->msg_index : nullptr, mg ? n * 4 : 0), o_grp = io.bytes(groups.data(), groups.size() * 4);
  uint8_t *c, *du, *W, *P, *Pj, *N, *NI = nullptr; const uint8_t* got; int r;
  if ((r = need(ctx, SB_STAGED, io.in_bytes, &c)) || (r = need(ctx, SB_UNIFORM, nh * 256, &du)) || (r = need(ctx, SB_RLC_WEIGHTS, n * 32, &W)) || (r = need(ctx, SB_RLC_PAIRS, o_res + back, &P)) ||
      (r = need(ctx, SB_RLC_KEYS_PROJ, n * 3 * RAW + n, &Pj)) || (r = need(ctx, SB_RLC_KEYS_NORM, n * RAW, &N)) || (!mg && (r = need(ctx, SB_RLC_KEYS_INV, n * RAW, &NI))) ||
      (r = ensure_scratch(ctx, n + 1)) || (r = ensure_side(ctx)) || (r = ensure_side2(ctx)))
    return r;
  if (!ctx->ev_fork && hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); return NBLS_EHIP; }
  uint8_t *RPK = P, *H = P + o_h, *PK = P + o_pkd, *SG = P + o_sgd, *O = P + o_res, *STK = O + 576, *STS = STK + n, *MS = STS + n;
  uint32_t* d_bad = (uint32_t*)(O + o_bad);
  if ((r = io.send(c, back))) return r;   // from here on an error return waits for every stream of the call
  HIPCHK(hipMemsetAsync(d_bad, 0, mg ? 8 : 4, s));
  LAUNCHCHK(nbls_rlc_weights_launch((unsigned)n, c + o_seed, W, s));
  HIPCHK(hipEventRecord(ctx->ev_fork, s));
  // signatures (side): PointG2.fromSignature, index.ts:500-530
  HIPCHK(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
  if ((r = dev_decompress(ctx, true, n, c + o_sig, SG, STS, ctx->side, DEC_SIGS))) return r;
  // keys (side2): PointG1.fromHex, index.ts:301-326 (aggregates: of every key, then one sum per set), then [r_i]pk_i
  HIPCHK(hipStreamWaitEvent(ctx->side2, ctx->ev_fork, 0));
  if (!agg) { if ((r = dev_decompress(ctx, false, n, c + o_pk, PK, STK, ctx->side2, DEC_KEYS))) return r; }
  else if ((r = aggregate_keys(ctx, n, *agg, c + o_pk, (const uint32_t*)(c + o_koff), PK, (int8_t*)STK, ctx->side2))) return r;
  if ((r = run(ctx, P_G1_MUL64, n, {B(0, PK, 96), B(2, W, 32), B(3, Pj, 3 * RAW), B(4, N, RAW)}, ctx->side2))) return r;
  if (mg) {
    const uint32_t* d_goff = (const uint32_t*)(c + o_grp);
    if ((r = group_keys(ctx, n, nh, maxgroup, d_goff + nh + 1, d_goff, (const int8_t*)STK, Pj, RPK, d_bad + 1, ctx->side2))) return r;
  } else if ((r = to_affine(ctx, false, n, Pj, N, NI, RPK, Pj + n * 3 * RAW, ctx->side2, false))) return r;
  HIPCHK(hipEventRecord(ctx->ev_join2, ctx->side2));
  // messages (s): expand_message_xmd, PointG2.hashToCurve (index.ts:481-490)
  LAUNCHCHK(nbls_xmd_launch((unsigned)nh, c + o_msg, c + o_off, c + o_dst, (unsigned)io.dst_len, du, 256, d_bad, s));
  if ((r = dev_hash_to_g2(ctx, nh, du, H, s))) return r;
  // S = sum_i [r_i]sig_i behind the signatures on the side stream (enqueued last: dev_msm waits on the host for its stream once, with the hash chain and the keys in flight)
  if ((r = dev_msm(ctx, true, n, SG, W, 64, H + nh * 192, MS, ctx->side, MSM_RLC))) return r;
  HIPCHK(hipEventRecord(ctx->ev_join, ctx->side));
  HIPCHK(hipStreamWaitEvent(s, ctx->ev_join2, 0));
  HIPCHK(hipStreamWaitEvent(s, ctx->ev_join, 0));
  HIPCHK(hipMemcpyAsync(RPK + nh * 96, ctx->neg_g1, 96, hipMemcpyDeviceToDevice, s));   // PointG1.BASE.negate()
  size_t m = 0;
  uint8_t* res = ctx->F;
  if ((r = miller_values(ctx, nh + 1, RPK, H, &m, s)) || (r = reduce_product(ctx, m, &res, s)) || (r = finish_single(ctx, Window(), res, 1, O, s))) return r;
  if ((r = io.fetch(O, back, &got))) return r;   // synchronised: both side streams were joined into s
  std::vector<uint8_t> rb(got, got + back);      // (the per-set pass reads back through the same block)
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
  if ((r = need(ctx, SB_RLC_PER_SET, n * (192 + 384 + 576) + n, &X))) return r;
  uint8_t *G1x = X, *G2x = G1x + n * 192, *E = G2x + n * 384, *V = E + n * 576;
  LAUNCHCHK(nbls_rlc_interleave_launch((unsigned)n, mg ? (const uint32_t*)(c + o_idx) : nullptr, PK, ctx->neg_g1, H, SG, G1x, G2x, s));
  if ((r = run(ctx, P_MILLER_RAW2, n, {B(0, G1x, 192), B(1, G2x, 384), B(3, ctx->F, F12)}, s)) || (r = items_is_one(ctx, n, E, V, s)) || (r = read_back(ctx, s, V, n, &got))) return r;
  int all = 1;
  for (size_t i = 0; i < n; i++) {
    // the reference's order (oracle_verify): the key decodes, the message hashes, the signature decodes, the pairing throws on a zero point ("No pairings at point of Infinity")
    const int8_t k = stk[i], g = sts[i];
    const int8_t v = k >= 2 ? k : g >= 2 ? (int8_t)(10 + g) : k == 1 ? 1 : g == 1 ? 11 : got[i] ? 0 : NBLS_ST_NOT_VERIFIED;
    status[i] = v;
    if (v) all = 0;
  }
  *all_ok = all;
  return NBLS_OK;
}

// ---- the six entry points: verify(sig_i, m_i, pk_i) for n sets; aggregates: pk_i = aggregatePublicKeys(keys_i) (index.ts:756-778), the keys given compressed or as indices into
// a key table; shared: the sets sign n_msgs <= n messages, msg_index[i] = the message of set i (the index itself is validated in the pipeline's one pass)
static const size_t AGG_MAX_KEYS = (size_t)1 << 24;   // keys per call (u32 set ids and ranks, at most 24 rounds of the segmented sum)
// What all six refuse before any device work.  Every call: context, result, sets (at most dev_msm's bound), signatures, offsets, tag, and message bytes when the offsets say there
// are some; shared forms: the index, 1 .. n messages; keys: compressed ones, or a table on this context's device (it lives in the memory of the device it was created on) and the
// indices; aggregates: key offsets that are increasing -- no empty set, the reference's aggregatePublicKeys throws "Expected non-empty array" -- over at most AGG_MAX_KEYS keys,
// every index inside the table.  Fills in agg->nkeys / maxset.
static int multi_verify(nbls_ctx* ctx, MultiVerifyIn in, AggKeys* agg, bool indexed, const MsgGroups* mg, int* all_ok, int8_t* status) {
  WHOLE_CALL(ctx);   // scratch and I/O staging buffers belong to this call until it returns
  const size_t n = in.n, nh = mg ? mg->n_msgs : n;
  if (!ctx || !all_ok || !n || n > ((size_t)1 << 22) || !in.sigs96 || !in.offsets || !in.dst || (mg && (!mg->msg_index || !nh || nh > n))) return NBLS_EINVAL;
  if (!in.msgs && in.offsets[nh] != in.offsets[0]) return NBLS_EINVAL;
  if (indexed ? (!agg->ks || !agg->key_index || agg->ks->device != ctx->device) : !in.pks48) return NBLS_EINVAL;
  if (agg) {
    const uint32_t* ko = agg->key_offsets;
    if (!ko) return NBLS_EINVAL;
    if (!strict_groups(n, ko, &agg->nkeys, &agg->maxset) || agg->nkeys > AGG_MAX_KEYS) return NBLS_EINVAL;
    if (indexed) for (size_t k = ko[0]; k < ko[n]; k++) if (agg->key_index[k] >= agg->ks->n) return NBLS_EINVAL;
  }
  in.agg = agg; in.mg = mg;
  return verify_multiple_pipeline(ctx, in, all_ok, status);
}
EXPORT int nbls_verify_multiple(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pks48, const uint8_t* dst, size_t dst_len,
                                const uint8_t* seed32, int* all_ok, int8_t* status) {
  return multi_verify(ctx, {n, sigs96, msgs, offsets, pks48, nullptr, nullptr, dst, dst_len, seed32}, nullptr, false, nullptr, all_ok, status);
}
EXPORT int nbls_verify_aggregates(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint8_t* pks48, const uint32_t* key_offsets,
                                  const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  AggKeys agg{key_offsets};
  return multi_verify(ctx, {n, sigs96, msgs, offsets, pks48, nullptr, nullptr, dst, dst_len, seed32}, &agg, false, nullptr, all_ok, status);
}
EXPORT int nbls_verify_aggregates_indexed(nbls_ctx* ctx, const nbls_keyset* ks, size_t n, const uint8_t* sigs96, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* key_index,
                                          const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  AggKeys agg{key_offsets, ks, key_index};
  return multi_verify(ctx, {n, sigs96, msgs, offsets, nullptr, nullptr, nullptr, dst, dst_len, seed32}, &agg, true, nullptr, all_ok, status);
}
EXPORT int nbls_verify_multiple_shared(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* msg_index,
                                       const uint8_t* pks48, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  const MsgGroups mg{n_msgs, msg_index};
  return multi_verify(ctx, {n, sigs96, msgs, offsets, pks48, nullptr, nullptr, dst, dst_len, seed32}, nullptr, false, &mg, all_ok, status);
}
EXPORT int nbls_verify_aggregates_shared(nbls_ctx* ctx, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets, const uint32_t* msg_index,
                                         const uint8_t* pks48, const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len, const uint8_t* seed32, int* all_ok, int8_t* status) {
  AggKeys agg{key_offsets};
  const MsgGroups mg{n_msgs, msg_index};
  return multi_verify(ctx, {n, sigs96, msgs, offsets, pks48, nullptr, nullptr, dst, dst_len, seed32}, &agg, false, &mg, all_ok, status);
}
EXPORT int nbls_verify_aggregates_indexed_shared(nbls_ctx* ctx, const nbls_keyset* ks, size_t n, const uint8_t* sigs96, size_t n_msgs, const uint8_t* msgs, const uint32_t* offsets,
                                                 const uint32_t* msg_index, const uint32_t* key_index, const uint32_t* key_offsets, const uint8_t* dst, size_t dst_len,
                                                 const uint8_t* seed32, int* all_ok, int8_t* status) {
  AggKeys agg{key_offsets, ks, key_index};
  const MsgGroups mg{n_msgs, msg_index};
  return multi_verify(ctx, {n, sigs96, msgs, offsets, nullptr, nullptr, nullptr, dst, dst_len, seed32}, &agg, true, &mg, all_ok, status);
}

// The key table: PointG1.fromHex (index.ts:298-327) of every key once, kept as raw projective points with the identity in place of zero keys and keys that did not decode, and the
// decoder's status of every key (which nbls_verify_aggregates_indexed reports for a set that names the key).  Owns its device memory: usable from any context on the same device,
// and after the creating context is destroyed.
static int keyset_build(nbls_ctx* ctx, nbls_keyset* ks, const uint8_t* pks48, int8_t* status) {
  const size_t n = ks->n;
  LOCKED(ctx);
  HostIO io{ctx};
  void *d = io.alloc(n * 48), *a = io.alloc(n * 96);
  if (!d || !a) return NBLS_EHIP;
  uint8_t* mem = nullptr;
  if (hipMalloc(&mem, n * 3 * RAW + n) != hipSuccess) { ctx->last_hip = (int)hipGetLastError(); return NBLS_EHIP; }
  ks->pts = mem; ks->st = (int8_t*)(mem + n * 3 * RAW);   // (freed by the caller's nbls_keyset_destroy on every error return)
  int r = NBLS_OK;
  hipError_t e = hipMemcpyAsync(d, pks48, n * 48, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && !(r = dev_decompress(ctx, false, n, d, a, ks->st, s)) && !(r = run(ctx, P_G1_TO_PROJ, n, {B(0, a, 96), B(3, ks->pts, 3 * RAW)}, s))) {
    const int k = nbls_agg_points_launch(n, (unsigned)(3 * RAW), nullptr, ks->st, ctx->ident_g1, ks->pts, ks->pts, s);
    if (k) { ctx->last_hip = k; r = NBLS_EHIP; }
    else if (status) e = hipMemcpyAsync(status, ks->st, n, hipMemcpyDeviceToHost, s);
    if (!r && e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) { ctx->last_hip = (int)e; r = NBLS_EHIP; }
  if (r) (void)hipStreamSynchronize(s);
  return r;
}
EXPORT int nbls_keyset_create(nbls_ctx* ctx, size_t n, const uint8_t* pks48, int8_t* status, nbls_keyset** out) {
  WHOLE_CALL(ctx);
  if (!ctx || !n || !pks48 || !out || n > AGG_MAX_KEYS) return NBLS_EINVAL;
  *out = nullptr;
  return handle_create(ctx, out, nbls_keyset_destroy, [&](nbls_keyset* ks) { ks->n = n; return keyset_build(ctx, ks, pks48, status); });
}
EXPORT void nbls_keyset_destroy(nbls_keyset* ks) {
  if (!ks) return;
  handle_free(ks->device, {ks->pts});
  delete ks;
}
EXPORT int nbls_keyset_size(const nbls_keyset* ks, size_t* n) {
  if (!ks || !n) return NBLS_EINVAL;
  *n = ks->n;
  return NBLS_OK;
}
