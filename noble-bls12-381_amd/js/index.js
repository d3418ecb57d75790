/*
 * index.js -- drop-in facade with the exported names of paulmillr/noble-bls12-381 v1.4.0 (reference index.ts:715-821)
 * over the MI355X engine (libnbls.so via the N-API addon).  Argument handling, error messages and result encodings follow
 * the reference; the arithmetic runs on the GPU.  Additive batched entry points: pairingBatch, millerProduct.
 *
 * getPublicKey / sign run the double-and-add-always ladders of the engine (SURVEY 8(f).1); additive: getPublicKeys, signBatch.
 * The reference's re-exported field classes Fp, Fr, Fp2 (index.ts:22) are single-element bigint helpers outside the batched hot
 * path: fields.js provides them on the host, together with Fp6 and Fp12 (finalExponentiate goes to the GPU).
 */
'use strict';
const path = require('path');
const native = require(path.join(__dirname, 'nbls_napi.node'));
const { Fp, Fr, Fp2, Fp6, Fp12 } = require('./fields.js');

// curve parameters under the reference's key names (math.ts:13-63).  h = (z - 1)^2 / 3 and h2 = (z^8 - 4z^7 + 5z^6 - 4z^4 + 6z^3 - 4z^2 - 4z + 13) / 9
// with z = -x; h2Eff is the effective G2 cofactor of RFC 9380 section 8.8.2; P2 is p^2 - 1 as in the reference.
const P_ = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaabn;
const CURVE = {
  P: P_,
  r: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001n,
  h: 0x396c8c005555e1568c00aaab0000aaabn,
  Gx: 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bbn,
  Gy: 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1n,
  b: 4n,
  P2: P_ ** 2n - 1n,
  h2: 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5n,
  G2x: [0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8n, 0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7en],
  G2y: [0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801n, 0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79ben],
  b2: [4n, 4n],
  x: 0xd201000000010000n,
  h2Eff: 0xbc69f08f2ee75b3584c6a0ea91b352888e2a8e9145ad7689986ff031508ffe1329c2f178731db956d82bf015d1212b02ec0ec69d7477c1ae954cbc06689f6a359894c0adebbf6b4e8020005aaa95551n,
};
const htfDefaults = { DST: 'BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_' };      // reference index.ts:60-81
let inited = false;
// NBLS_DEVICES = "0,1,2,3" (or "all") opens every listed GPU behind one handle: pairing batches, Miller products and verifyBatch then shard
// over them inside the library (nbls_multi_*, include/nbls.h); NBLS_DEVICE = n selects a single GPU (default 0).
function ensureInit() {
  if (inited) return;
  const list = process.env.NBLS_DEVICES;
  if (list) native.initMulti(list === 'all' ? null : Int32Array.from(list.split(',').map(Number)));
  else native.init(Number(process.env.NBLS_DEVICE || 0));
  inited = true;
}

// ---- byte helpers (reference math.ts:158-212)
function hexToBytes(hex) {
  if (typeof hex !== 'string') throw new TypeError('hexToBytes: expected string, got ' + typeof hex);
  if (hex.length % 2) throw new Error('hexToBytes: received invalid unpadded hex');
  const a = new Uint8Array(hex.length / 2);
  for (let i = 0; i < a.length; i++) { const b = Number.parseInt(hex.slice(2 * i, 2 * i + 2), 16); if (Number.isNaN(b)) throw new Error('Invalid byte sequence'); a[i] = b; }
  return a;
}
const hexes = Array.from({ length: 256 }, (v, i) => i.toString(16).padStart(2, '0'));
function bytesToHex(u8) { let s = ''; for (let i = 0; i < u8.length; i++) s += hexes[u8[i]]; return s; }
function ensureBytes(hex) { return hex instanceof Uint8Array ? Uint8Array.from(hex) : hexToBytes(hex); }
function concat(...arrs) { const n = arrs.reduce((a, b) => a + b.length, 0); const r = new Uint8Array(n); let o = 0; for (const a of arrs) { r.set(a, o); o += a.length; } return r; }
function toBig(u8) { return BigInt('0x' + (bytesToHex(u8) || '0')); }
function stringToBytes(str) { const b = new Uint8Array(str.length); for (let i = 0; i < str.length; i++) b[i] = str.charCodeAt(i); return b; }
function isZeroBytes(u8) { for (let i = 0; i < u8.length; i++) if (u8[i]) return false; return true; }
const G1_STATUS = { 2: 'Invalid G1 point: not on curve Fp', 3: 'Invalid G1 point: must be of prime-order subgroup', 4: 'Invalid compressed G1 point' };
const G2_STATUS = { 2: 'Invalid G2 point: not on curve Fp2', 3: 'Invalid G2 point: must be of prime-order subgroup', 4: 'Failed to find a square root' };

// ---- Fp12: the host class of fields.js (coordinates, math.ts:705-885 method names); the final exponentiation runs on the GPU
Fp12.prototype.finalExponentiate = function () { ensureInit(); return Fp12.fromBytes(native.finalExpBatch(this.toBytes())); };

// ---- points: affine wire bytes, or the zero point
// reference math.ts:1035-1043
function validateScalar(n) {
  if (typeof n === 'number') n = BigInt(n);
  if (typeof n !== 'bigint' || n <= 0 || n > CURVE.r) throw new Error(`Point#multiply: invalid scalar, expected positive integer < CURVE.r. Got: ${n}`);
  return n;
}
const scalarBytes = (n) => hexToBytes(validateScalar(n).toString(16).padStart(64, '0'));

// ---- threshold recombination (nbls_g2_combine_shares / nbls_g1_combine_shares; not in the reference, whose README names the use): sum_k [lambda_k]share_k with the Lagrange
// coefficients at zero of the identifiers, one call for all groups, on a worker thread.  Identifiers: bigint | number | hex | 32 bytes, any value below 2^256 (reduced mod r).
function shareIdBytes(x) {
  if (x instanceof Uint8Array) { if (x.length !== 32) throw new Error('Invalid share identifier: expected 32 bytes'); return x; }
  if (typeof x === 'number' && !Number.isSafeInteger(x)) throw new Error('Invalid share identifier: expected an integer');
  const v = typeof x === 'string' ? BigInt('0x' + x.replace(/^0x/, '')) : BigInt(x);
  if (v < 0n || v >> 256n) throw new Error('Invalid share identifier: expected 0 <= id < 2^256');
  return hexToBytes(v.toString(16).padStart(64, '0'));
}
// groups: [{ shares, ids }] (or [shares, ids] pairs).  A group of points yields a point; of bytes or hex (compressed shares), bytes; a group that mixes the
// two is refused.  Throws Error on identifiers that are zero or
// repeated mod r and on a share that does not decode, as the decoders do
async function combineSharesBatch(Point, groups) {
  const g2 = Point === PointG2, e = g2 ? 96 : 48, STATUS = g2 ? G2_STATUS : G1_STATUS;
  if (!groups.length) throw new Error('Expected non-empty array');
  const offs = new Uint32Array(groups.length + 1), ids = [], shares = [], asPoint = [];
  groups.forEach((grp, g) => {
    const sh = Array.isArray(grp) ? grp[0] : grp.shares, id = Array.isArray(grp) ? grp[1] : grp.ids;
    if (!sh || !id || !sh.length || sh.length !== id.length) throw new Error('Expected as many share identifiers as shares, at least one');
    const points = sh.filter((p) => p instanceof Point).length;
    if (points && points !== sh.length) throw new Error('Expected the shares of a group to be all points or all compressed bytes');
    asPoint.push(points > 0);
    for (const p of sh) {
      const b = p instanceof Point ? (g2 ? p.toSignature() : p.toRawBytes(true)) : ensureBytes(p);
      if (b.length !== e) throw new Error('Invalid share: expected ' + e + ' compressed bytes');
      shares.push(b);
    }
    for (const x of id) ids.push(shareIdBytes(x));
    offs[g + 1] = offs[g] + sh.length;
  });
  ensureInit();
  const { out, status } = await native.combineSharesAsync(g2 ? 1 : 0, offs, concat(...ids), concat(...shares));
  return groups.map((_, g) => {
    const st = status[g];
    if (st === 20) throw new Error('Invalid share identifiers: zero or repeated modulo CURVE.r');
    if (st > 1) throw new Error(STATUS[st] || 'Invalid share (status ' + st + ')');
    const bytes = out.slice(g * e, g * e + e);
    if (!asPoint[g]) return bytes;
    return st === 1 ? Point.ZERO : (g2 ? PointG2.fromSignature(bytes) : PointG1.fromHex(bytes));
  });
}

// ---- share public keys (nbls_g1_poly_eval / nbls_g2_poly_eval; not in the reference): the commitment polynomial of a DKG / Feldman VSS, F(x) = sum_j [x^j]A_j with the committed
// coefficients A_j lowest degree first (A_0 = the group key), evaluated at the share identifiers -- any value below 2^256, zero included: F(0) = A_0 --, one call for all groups,
// on a worker thread.  groups: [{ coefs, ids }] (or [coefs, ids] pairs).  A group of points yields points; of bytes or hex (compressed coefficients), bytes; a group that mixes
// the two is refused.  Throws Error on a coefficient that does not decode, as the decoders do
async function evalCommitmentBatch(Point, groups) {
  const g2 = Point === PointG2, e = g2 ? 96 : 48, STATUS = g2 ? G2_STATUS : G1_STATUS;
  if (!groups.length) throw new Error('Expected non-empty array');
  const coffs = new Uint32Array(groups.length + 1), offs = new Uint32Array(groups.length + 1), ids = [], coefs = [], asPoint = [];
  groups.forEach((grp, g) => {
    const cf = Array.isArray(grp) ? grp[0] : grp.coefs, id = Array.isArray(grp) ? grp[1] : grp.ids;
    if (!cf || !id || !cf.length || !id.length) throw new Error('Expected at least one coefficient and one identifier');
    const points = cf.filter((p) => p instanceof Point).length;
    if (points && points !== cf.length) throw new Error('Expected the coefficients of a group to be all points or all compressed bytes');
    asPoint.push(points > 0);
    for (const p of cf) {
      const b = p instanceof Point ? (g2 ? p.toSignature() : p.toRawBytes(true)) : ensureBytes(p);
      if (b.length !== e) throw new Error('Invalid coefficient: expected ' + e + ' compressed bytes');
      coefs.push(b);
    }
    for (const x of id) ids.push(shareIdBytes(x));
    coffs[g + 1] = coffs[g] + cf.length; offs[g + 1] = offs[g] + id.length;
  });
  ensureInit();
  const { out, status } = await native.polyEvalAsync(g2 ? 1 : 0, coffs, concat(...coefs), offs, concat(...ids));
  return groups.map((_, g) => {
    const res = [];
    for (let k = offs[g]; k < offs[g + 1]; k++) {
      const st = status[k];
      if (st > 1) throw new Error(STATUS[st] || 'Invalid coefficient (status ' + st + ')');
      const bytes = out.slice(k * e, k * e + e);
      res.push(!asPoint[g] ? bytes : st === 1 ? Point.ZERO : (g2 ? PointG2.fromSignature(bytes) : PointG1.fromHex(bytes)));
    }
    return res;
  });
}

// ---- KZG (nbls_kzg_verify_proofs / nbls_kzg_verify_blobs; EIP-4844, not in the reference): verify_kzg_proof_batch and verify_blob_kzg_proof_batch against the setup's [tau]G2
// (96 compressed bytes, hex, or a PointG2).  Commitments and proofs: 48 compressed bytes, hex, or PointG1 (the zero point is valid for both); z, y: bigint | number | hex | 32
// bytes, canonical (a value >= CURVE.r is refused with status 21).  -> { ok, status }: ok = every item verified; status = one byte per item (0 ok, 9 not verified, 3 / 4 the
// commitment does not decode, 13 / 14 the proof, 21 a non-canonical field element), or null with opts.perItem === false (the combined check alone).  opts.seed: 32 bytes for a
// reproducible test; by default the weights come from the OS.  The arrays are filled by loops: a mainnet call carries blobs of 131,072 bytes each
function kzgPack(items, width, what, toBytes) {
  const out = new Uint8Array(items.length * width);
  for (let i = 0; i < items.length; i++) {
    const b = toBytes(items[i]);
    if (b.length !== width) throw new Error('Invalid ' + what + ': expected ' + width + ' bytes');
    out.set(b, i * width);
  }
  return out;
}
const kzgG1 = (p) => (p instanceof PointG1 ? p.toRawBytes(true) : ensureBytes(p));
const kzgTau = (t) => { const b = t instanceof PointG2 ? t.toSignature() : ensureBytes(t); if (b.length !== 96) throw new Error('Invalid [tau]G2: expected 96 compressed bytes'); return b; };
function kzgSeed(opts) {
  const seed = opts && opts.seed ? ensureBytes(opts.seed) : null;
  if (seed && seed.length !== 32) throw new Error('Invalid seed: expected 32 bytes');
  return seed;
}
function kzgResult(res, perItem) {
  const ok = (res.out[0] | res.out[1] | res.out[2] | res.out[3]) !== 0;
  return { ok, status: perItem ? res.status : null };
}
function kzgProofArgs(commitments, zs, ys, proofs, tauG2, opts) {
  const n = commitments.length;
  if (!n) throw new Error('Expected non-empty array');
  if (zs.length !== n || ys.length !== n || proofs.length !== n) throw new Error('Expected as many points, values and proofs as commitments');
  const perItem = !(opts && opts.perItem === false);
  return [kzgPack(commitments, 48, 'commitment', kzgG1), kzgPack(zs, 32, 'field element', shareIdBytes), kzgPack(ys, 32, 'field element', shareIdBytes), kzgPack(proofs, 48, 'proof', kzgG1),
    kzgTau(tauG2), kzgSeed(opts), perItem ? 1 : 0];
}
function kzgBlobArgs(blobs, commitments, proofs, tauG2, opts) {
  const n = blobs.length;
  if (!n) throw new Error('Expected non-empty array');
  if (commitments.length !== n || proofs.length !== n) throw new Error('Expected as many commitments and proofs as blobs');
  const first = ensureBytes(blobs[0]), log2n = Math.round(Math.log2(first.length / 32));
  if (log2n < 1 || log2n > 12 || first.length !== 32 << log2n) throw new Error('Invalid blob: expected 32 * 2^k bytes, 1 <= k <= 12');
  const perItem = !(opts && opts.perItem === false);
  return [log2n, kzgPack(blobs, first.length, 'blob', ensureBytes), kzgPack(commitments, 48, 'commitment', kzgG1), kzgPack(proofs, 48, 'proof', kzgG1), kzgTau(tauG2), kzgSeed(opts), perItem ? 1 : 0];
}
function kzgFail(e) {
  if (e && e.nblsCode === -5) throw new Error('Invalid [tau]G2: does not decode or is the zero point');
  throw e;
}
function verifyKzgProofBatch(commitments, zs, ys, proofs, tauG2, opts) {
  const a = kzgProofArgs(commitments, zs, ys, proofs, tauG2, opts);
  ensureInit();
  try { return kzgResult(native.kzgVerifyProofs(a[0], a[1], a[2], a[3], a[4], a[5], a[6]), a[6]); } catch (e) { return kzgFail(e); }
}
async function verifyKzgProofBatchAsync(commitments, zs, ys, proofs, tauG2, opts) {
  const a = kzgProofArgs(commitments, zs, ys, proofs, tauG2, opts);
  ensureInit();
  try { return kzgResult(await native.kzgVerifyProofsAsync(a[0], a[1], a[2], a[3], a[4], a[5], a[6]), a[6]); } catch (e) { return kzgFail(e); }
}
function verifyBlobKzgProofBatch(blobs, commitments, proofs, tauG2, opts) {
  const a = kzgBlobArgs(blobs, commitments, proofs, tauG2, opts);
  ensureInit();
  try { return kzgResult(native.kzgVerifyBlobs(a[0], a[1], a[2], a[3], a[4], a[5], a[6]), a[6]); } catch (e) { return kzgFail(e); }
}
async function verifyBlobKzgProofBatchAsync(blobs, commitments, proofs, tauG2, opts) {
  const a = kzgBlobArgs(blobs, commitments, proofs, tauG2, opts);
  ensureInit();
  try { return kzgResult(await native.kzgVerifyBlobsAsync(a[0], a[1], a[2], a[3], a[4], a[5], a[6]), a[6]); } catch (e) { return kzgFail(e); }
}

// ---- KZG, the prover's side (nbls_kzg_setup_*, nbls_kzg_commit_blobs / _compute_proofs / _compute_blob_proofs): blob_to_kzg_commitment, compute_kzg_proof and
// compute_blob_kzg_proof for many blobs against a setup kept on the device.  new PointG1.KzgSetup(points) (a static of PointG1, like the calls: the top-level exports stay as they are): the setup's g1_lagrange in bit-reversed order (2^k points, 1 <= k <= 12; 48
// compressed bytes, hex, or PointG1 each), decoded once; close() frees it.  Blobs: bytes or hex of 32 * 2^k; z: bigint | number | hex | 32 bytes.  Results are arrays of
// Uint8Array (48-byte compressed points, 32-byte values) and status = one byte per blob (0, or 21: a blob element or z is >= CURVE.r, that blob's outputs are then all-zero bytes)
class KzgSetup {
  constructor(points) {
    const log2n = Math.round(Math.log2(points.length));
    if (log2n < 1 || log2n > 12 || points.length !== 1 << log2n) throw new Error('Invalid setup: expected 2^k points, 1 <= k <= 12');
    ensureInit();
    this.log2n = log2n;
    try { this.handle = native.kzgSetupCreate(log2n, kzgPack(points, 48, 'setup point', kzgG1)); } catch (e) {
      if (e && e.nblsCode === -5) { const err = new Error('Invalid setup: a point does not decode, is outside the subgroup or is the zero point'); err.status = e.status; throw err; }
      throw e;
    }
  }
  close() { if (this.handle) native.kzgSetupDestroy(this.handle); this.handle = null; }
}
function kzgProveArgs(setup, blobs, aux, auxWidth, what, toBytes) {
  if (!(setup instanceof KzgSetup) || !setup.handle) throw new Error('Expected an open KzgSetup');
  if (!blobs.length) throw new Error('Expected non-empty array');
  if (aux && aux.length !== blobs.length) throw new Error('Expected as many ' + what + 's as blobs');
  return [setup.handle, kzgPack(blobs, 32 << setup.log2n, 'blob', ensureBytes), aux ? kzgPack(aux, auxWidth, what, toBytes) : null];
}
function kzgSplit(res, n, widths) {
  const parts = []; let at = 0;
  for (const w of widths) { const one = []; for (let i = 0; i < n; i++) one.push(res.out.slice(at + i * w, at + (i + 1) * w)); parts.push(one); at += n * w; }
  return parts;
}
const kzgCommitResult = (res, n) => ({ commitments: kzgSplit(res, n, [48])[0], status: res.status });
const kzgProofResult = (res, n) => { const p = kzgSplit(res, n, [48, 32]); return { proofs: p[0], ys: p[1], status: res.status }; };
const kzgBlobProofResult = (res, n) => { const p = kzgSplit(res, n, [48, 48]); return { commitments: p[0], proofs: p[1], status: res.status }; };
function blobToKzgCommitments(setup, blobs) { const a = kzgProveArgs(setup, blobs, null); return kzgCommitResult(native.kzgProve(0, a[0], a[1], null), blobs.length); }
async function blobToKzgCommitmentsAsync(setup, blobs) { const a = kzgProveArgs(setup, blobs, null); return kzgCommitResult(await native.kzgProveAsync(0, a[0], a[1], null), blobs.length); }
function computeKzgProofs(setup, blobs, zs) { const a = kzgProveArgs(setup, blobs, zs, 32, 'field element', shareIdBytes); return kzgProofResult(native.kzgProve(1, a[0], a[1], a[2]), blobs.length); }
async function computeKzgProofsAsync(setup, blobs, zs) { const a = kzgProveArgs(setup, blobs, zs, 32, 'field element', shareIdBytes); return kzgProofResult(await native.kzgProveAsync(1, a[0], a[1], a[2]), blobs.length); }
function computeBlobKzgProofs(setup, blobs, commitments) { const a = kzgProveArgs(setup, blobs, commitments || null, 48, 'commitment', kzgG1); return kzgBlobProofResult(native.kzgProve(2, a[0], a[1], a[2]), blobs.length); }
async function computeBlobKzgProofsAsync(setup, blobs, commitments) { const a = kzgProveArgs(setup, blobs, commitments || null, 48, 'commitment', kzgG1); return kzgBlobProofResult(await native.kzgProveAsync(2, a[0], a[1], a[2]), blobs.length); }

// ---- PeerDAS (nbls_fr_ntt, nbls_kzg_compute_cells, nbls_kzg_monomial_*, nbls_kzg_compute_cells_and_proofs; EIP-7594): the transform between the coefficients of a polynomial
// and its values on the roots of unity, compute_cells and compute_cells_and_kzg_proofs for many blobs.  Statics of PointG1 like the prover's calls.  new PointG1.KzgMonomialSetup(points):
// the setup's g1_monomial in natural order (2^k points, 1 <= k <= 12), decoded once; close() frees it.  Rows and blobs: bytes or hex of 32 * 2^k.  Results are arrays of Uint8Array
// and status = one byte per polynomial or blob (0; 21: an element or the shift is >= CURVE.r; 5: the shift is 0 -- the outputs of that item are then all-zero bytes)
class KzgMonomialSetup {
  constructor(points) {
    const log2n = Math.round(Math.log2(points.length));
    if (log2n < 1 || log2n > 12 || points.length !== 1 << log2n) throw new Error('Invalid setup: expected 2^k points, 1 <= k <= 12');
    ensureInit();
    this.log2n = log2n;
    try { this.handle = native.kzgMonomialCreate(log2n, kzgPack(points, 48, 'setup point', kzgG1)); } catch (e) {
      if (e && e.nblsCode === -5) { const err = new Error('Invalid setup: a point does not decode, is outside the subgroup or is the zero point'); err.status = e.status; throw err; }
      throw e;
    }
  }
  close() { if (this.handle) native.kzgMonomialDestroy(this.handle); this.handle = null; }
}
function frNttArgs(log2n, rows, toEvals, shifts) {
  if (!Number.isInteger(log2n) || log2n < 1 || log2n > 12) throw new Error('Expected log2n in 1 .. 12');
  if (!rows.length) throw new Error('Expected non-empty array');
  if (shifts && shifts.length !== rows.length) throw new Error('Expected as many shifts as polynomials');
  ensureInit();
  return [log2n, toEvals ? 1 : 0, kzgPack(rows, 32 << log2n, 'polynomial', ensureBytes), shifts ? kzgPack(shifts, 32, 'field element', shareIdBytes) : null];
}
const frNttResult = (res, n, log2n) => ({ rows: kzgSplit(res, n, [32 << log2n])[0], status: res.status });
function frNtt(log2n, rows, toEvals, shifts) { const a = frNttArgs(log2n, rows, toEvals, shifts); return frNttResult(native.frNtt(a[0], a[1], a[2], a[3]), rows.length, log2n); }
async function frNttAsync(log2n, rows, toEvals, shifts) { const a = frNttArgs(log2n, rows, toEvals, shifts); return frNttResult(await native.frNttAsync(a[0], a[1], a[2], a[3]), rows.length, log2n); }
function kzgCellArgs(log2n, log2cell, blobs) {
  if (!Number.isInteger(log2cell) || log2cell < 0 || log2cell > log2n) throw new Error('Expected log2cell in 0 .. log2n');
  if (!blobs.length) throw new Error('Expected non-empty array');
  return kzgPack(blobs, 32 << log2n, 'blob', ensureBytes);
}
// res.out = per blob its 2 N elements in cell order (, then the proofs) -> cells[blob][k], proofs[blob][k]
function kzgCellsResult(res, n, log2n, log2cell, withProofs) {
  const per = 2 << (log2n - log2cell), cell = 32 << log2cell, cells = [], proofs = [], at = n * per * cell;
  for (let i = 0; i < n; i++) {
    const cs = [], ps = [];
    for (let k = 0; k < per; k++) {
      cs.push(res.out.slice((i * per + k) * cell, (i * per + k + 1) * cell));
      if (withProofs) ps.push(res.out.slice(at + (i * per + k) * 48, at + (i * per + k + 1) * 48));
    }
    cells.push(cs); proofs.push(ps);
  }
  return withProofs ? { cells, proofs, status: res.status } : { cells, status: res.status };
}
function computeCells(log2n, log2cell, blobs) {
  if (!Number.isInteger(log2n) || log2n < 1 || log2n > 12) throw new Error('Expected log2n in 1 .. 12');
  const b = kzgCellArgs(log2n, log2cell, blobs); ensureInit();
  return kzgCellsResult(native.kzgComputeCells(log2n, log2cell, b), blobs.length, log2n, log2cell, false);
}
async function computeCellsAsync(log2n, log2cell, blobs) {
  if (!Number.isInteger(log2n) || log2n < 1 || log2n > 12) throw new Error('Expected log2n in 1 .. 12');
  const b = kzgCellArgs(log2n, log2cell, blobs); ensureInit();
  return kzgCellsResult(await native.kzgComputeCellsAsync(log2n, log2cell, b), blobs.length, log2n, log2cell, false);
}
function kzgMonomialOpen(setup) { if (!(setup instanceof KzgMonomialSetup) || !setup.handle) throw new Error('Expected an open KzgMonomialSetup'); }
function computeCellsAndKzgProofs(setup, log2cell, blobs) {
  kzgMonomialOpen(setup); const b = kzgCellArgs(setup.log2n, log2cell, blobs);
  return kzgCellsResult(native.kzgCellsAndProofs(setup.handle, log2cell, b), blobs.length, setup.log2n, log2cell, true);
}
async function computeCellsAndKzgProofsAsync(setup, log2cell, blobs) {
  kzgMonomialOpen(setup); const b = kzgCellArgs(setup.log2n, log2cell, blobs);
  return kzgCellsResult(await native.kzgCellsAndProofsAsync(setup.handle, log2cell, b), blobs.length, setup.log2n, log2cell, true);
}
// recover_cells_and_kzg_proofs (nbls_kzg_recover_cells / _and_proofs): cellIndices[i] lists the numbers of the cells given for blob i, in any order, cells[i] those cells (bytes
// or hex of 32 << log2cell each, as computeCells returns them); at least half of a blob's cells.  -> { cells, status } / { cells, proofs, status } as computeCells /
// computeCellsAndKzgProofs return them for the recovered blobs; status per blob: 22 = fewer than half of the cells, an index out of range or twice; 21 = an element is >= CURVE.r;
// 23 = the given cells contradict one another -- the blob's cells are then all-zero bytes and its proofs 48 zero bytes each
function kzgRecoverArgs(log2n, log2cell, cellIndices, cells) {
  if (!Number.isInteger(log2n) || log2n < 1 || log2n > 12) throw new Error('Expected log2n in 1 .. 12');
  if (!Number.isInteger(log2cell) || log2cell < 0 || log2cell > log2n) throw new Error('Expected log2cell in 0 .. log2n');
  if (!Array.isArray(cellIndices) || !Array.isArray(cells) || !cells.length) throw new Error('Expected non-empty array');
  if (cellIndices.length !== cells.length) throw new Error('Expected as many lists of cell indices as lists of cells');
  const offs = new Uint32Array(cells.length + 1), flat = [], all = [];
  cells.forEach((cs, i) => {
    if (!Array.isArray(cs) || !Array.isArray(cellIndices[i]) || cs.length !== cellIndices[i].length) throw new Error('Expected as many cell indices as cells for every blob');
    for (const v of cellIndices[i]) { if (!Number.isInteger(v) || v < 0 || v > 0xffffffff) throw new Error('Invalid cell index: expected a 32-bit unsigned integer'); flat.push(v); }
    for (const c of cs) all.push(c);
    offs[i + 1] = flat.length;
  });
  return [offs, Uint32Array.from(flat), all.length ? kzgPack(all, 32 << log2cell, 'cell', ensureBytes) : new Uint8Array(0)];
}
function recoverCells(log2n, log2cell, cellIndices, cells) {
  const a = kzgRecoverArgs(log2n, log2cell, cellIndices, cells); ensureInit();
  return kzgCellsResult(native.kzgRecoverCells(log2n, log2cell, a[0], a[1], a[2]), cells.length, log2n, log2cell, false);
}
async function recoverCellsAsync(log2n, log2cell, cellIndices, cells) {
  const a = kzgRecoverArgs(log2n, log2cell, cellIndices, cells); ensureInit();
  return kzgCellsResult(await native.kzgRecoverCellsAsync(log2n, log2cell, a[0], a[1], a[2]), cells.length, log2n, log2cell, false);
}
function recoverCellsAndKzgProofs(setup, log2cell, cellIndices, cells) {
  kzgMonomialOpen(setup); const a = kzgRecoverArgs(setup.log2n, log2cell, cellIndices, cells);
  return kzgCellsResult(native.kzgRecoverCellsAndProofs(setup.handle, log2cell, a[0], a[1], a[2]), cells.length, setup.log2n, log2cell, true);
}
async function recoverCellsAndKzgProofsAsync(setup, log2cell, cellIndices, cells) {
  kzgMonomialOpen(setup); const a = kzgRecoverArgs(setup.log2n, log2cell, cellIndices, cells);
  return kzgCellsResult(await native.kzgRecoverCellsAndProofsAsync(setup.handle, log2cell, a[0], a[1], a[2]), cells.length, setup.log2n, log2cell, true);
}
// verify_cell_kzg_proof_batch (nbls_kzg_verify_cells): cell k of the call is cell number cellIndices[k] of the blob committed to by commitments[commitmentIndices[k]] -- every
// commitment once, cells may repeat --, with its proof; tauCG2: the setup's [tau^c]G2 (g2_monomial[c]; 96 compressed bytes, hex, or a PointG2), c = 2^log2cell <= 64 elements per
// cell.  -> { ok, status } as verifyKzgProofBatch (status per cell: 21 = an element of the cell is >= CURVE.r); opts.seed, opts.perItem likewise
function kzgVerifyCellsArgs(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts) {
  kzgMonomialOpen(setup);
  if (!Number.isInteger(log2cell) || log2cell < 0 || log2cell > 6 || log2cell > setup.log2n) throw new Error('Expected log2cell in 0 .. min(6, log2n)');
  const n = cells.length;
  if (!n || !commitments.length) throw new Error('Expected non-empty array');
  if (commitmentIndices.length !== n || cellIndices.length !== n || proofs.length !== n) throw new Error('Expected as many commitment indices, cell indices and proofs as cells');
  const index = (v, bound, what) => { if (!Number.isInteger(v) || v < 0 || v >= bound) throw new Error('Invalid ' + what + ': expected an integer in 0 .. ' + (bound - 1)); return v; };
  const ci = Uint32Array.from(commitmentIndices, (v) => index(v, commitments.length, 'commitment index'));
  const ki = Uint32Array.from(cellIndices, (v) => index(v, 2 << (setup.log2n - log2cell), 'cell index'));
  const perItem = !(opts && opts.perItem === false);
  return [setup.handle, log2cell, kzgPack(commitments, 48, 'commitment', kzgG1), ci, ki, kzgPack(cells, 32 << log2cell, 'cell', ensureBytes), kzgPack(proofs, 48, 'proof', kzgG1),
    kzgTau(tauCG2), kzgSeed(opts), perItem ? 1 : 0];
}
function verifyCellKzgProofBatch(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts) {
  const a = kzgVerifyCellsArgs(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts);
  try { return kzgResult(native.kzgVerifyCells(...a), a[9]); } catch (e) { return kzgFail(e); }
}
async function verifyCellKzgProofBatchAsync(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts) {
  const a = kzgVerifyCellsArgs(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts);
  try { return kzgResult(await native.kzgVerifyCellsAsync(...a), a[9]); } catch (e) { return kzgFail(e); }
}

// ---- Groth16 (nbls_groth16_vk_*, nbls_groth16_verify; not in the reference): n proofs against one verifying key, checked together by a random linear combination.
// new PointG1.Groth16Vk({alpha, beta, gamma, delta, ic}): alpha and the m + 1 points ic: 48 compressed bytes, hex or PointG1; beta, gamma, delta: 96 compressed bytes, hex or
// PointG2; decoded once, close() frees it.  Parsing bellman's uncompressed key file stays with the caller.  verifyGroth16Batch(vk, proofs, inputs, {seed, perItem}): proofs =
// an array of 192-byte proofs (A || B || C compressed: bytes or hex) or ONE packed Uint8Array of n * 192 bytes; inputs = an array of rows of m field elements (bigint | number |
// hex | 32 bytes, canonical) or ONE packed Uint8Array of n * m * 32 bytes.  -> { ok, status } as verifyKzgProofBatch: status per proof 0 ok, 9 not verified, 1 / 3 / 4 A is the
// zero point / does not decode, 11 / 13 / 14 B, 31 / 33 / 34 C, 21 a non-canonical input
const g16G2 = (p, what) => { const b = p instanceof PointG2 ? p.toSignature() : ensureBytes(p); if (b.length !== 96) throw new Error('Invalid ' + what + ': expected 96 compressed bytes'); return b; };
class Groth16Vk {
  constructor(key) {
    if (!key || !key.ic || key.ic.length < 2 || key.ic.length > 65537) throw new Error('Invalid key: expected alpha, beta, gamma, delta and 2 .. 65537 points ic');
    ensureInit();
    this.inputs = key.ic.length - 1;
    const alpha = kzgG1(key.alpha);
    if (alpha.length !== 48) throw new Error('Invalid alpha: expected 48 compressed bytes');
    try { this.handle = native.groth16VkCreate(alpha, g16G2(key.beta, 'beta'), g16G2(key.gamma, 'gamma'), g16G2(key.delta, 'delta'), kzgPack(key.ic, 48, 'key point', kzgG1)); } catch (e) {
      if (e && e.nblsCode === -5) { const err = new Error('Invalid key: a point does not decode, is outside the subgroup or is the zero point'); err.status = e.status; throw err; }
      throw e;
    }
  }
  close() { if (this.handle) native.groth16VkDestroy(this.handle); this.handle = null; }
}
function groth16Args(vk, proofs, inputs, opts) {
  if (!(vk instanceof Groth16Vk) || !vk.handle) throw new Error('Expected an open Groth16Vk');
  const packed = (v) => v instanceof Uint8Array;
  const ps = packed(proofs) ? proofs : kzgPack(proofs, 192, 'proof', ensureBytes);
  const n = ps.length / 192;
  if (!n || !Number.isInteger(n)) throw new Error('Expected one proof or more of 192 bytes each');
  let xs = inputs;
  if (!packed(inputs)) {
    if (inputs.length !== n) throw new Error('Expected as many rows of inputs as proofs');
    xs = new Uint8Array(n * vk.inputs * 32);
    for (let i = 0; i < n; i++) {
      if (inputs[i].length !== vk.inputs) throw new Error('Invalid inputs: expected ' + vk.inputs + ' per proof');
      xs.set(kzgPack(inputs[i], 32, 'field element', shareIdBytes), i * vk.inputs * 32);
    }
  }
  if (xs.length !== n * vk.inputs * 32) throw new Error('Invalid inputs: expected ' + vk.inputs + ' per proof, 32 bytes each');
  const perItem = !(opts && opts.perItem === false);
  return [vk.handle, ps, xs, kzgSeed(opts), perItem ? 1 : 0];
}
function verifyGroth16Batch(vk, proofs, inputs, opts) { const a = groth16Args(vk, proofs, inputs, opts); return kzgResult(native.groth16Verify(...a), a[4]); }
async function verifyGroth16BatchAsync(vk, proofs, inputs, opts) { const a = groth16Args(vk, proofs, inputs, opts); return kzgResult(await native.groth16VerifyAsync(...a), a[4]); }

// ---- The Groth16 prover (nbls_groth16_pk_*, nbls_groth16_prove; not in the reference).  groth16ProvingKey({log2n, nVars, nPublic, matrices: [A, B, C], alphaG1, betaG1,
// betaG2, deltaG1, deltaG2, aQuery, bG1Query, bG2Query, lQuery, hQuery}): a matrix is an array of rows (the same number in all three, at most 2^log2n), a row an array of
// [column, coefficient] with the coefficient a field element (bigint | number | hex | 32 bytes, canonical); G1 points 48 compressed bytes, hex or PointG1, G2 points 96
// compressed bytes, hex or PointG2; a zero point (c0 00..) is valid in the four per-variable queries.  Decoded once, close() frees it; a refused key throws with the decoder's statuses as `status`.
// groth16Prove(pk, witnesses, rs): witnesses = an array of assignments z = [1, x_1 .. x_m, aux ..] of nVars field elements each, or ONE packed Uint8Array; rs = an array of
// [r, s] per witness, or null / undefined: drawn from the OS.  -> { proofs: n x 192 bytes (A || B || C compressed), status } -- status per proof 0 ok, 21 an element >= CURVE.r,
// 24 the witness does not satisfy the constraints, 1 A or B is the zero point; a proof whose status is not 0 is 192 zero bytes.  The library wipes its own copies of the
// witness and of (r, s); the arrays passed in are the caller's
class Groth16Pk {
  constructor(key) {
    if (!key || !Array.isArray(key.matrices) || key.matrices.length !== 3) throw new Error('Invalid key: expected log2n, nVars, nPublic, three matrices and the key points');
    const { log2n, nVars, nPublic } = key, rows = key.matrices[0].length;
    if (!Number.isInteger(log2n) || log2n < 1 || log2n > 21 || !Number.isInteger(nVars) || !Number.isInteger(nPublic) || nPublic < 1 || nVars <= nPublic)
      throw new Error('Invalid key: expected log2n in 1 .. 21 and 0 < nPublic < nVars');
    if (key.matrices.some((m) => m.length !== rows) || rows > 2 ** log2n) throw new Error('Invalid key: expected three matrices of the same number of rows, at most 2^log2n');
    ensureInit();
    const args = [Uint32Array.of(log2n, nVars, nPublic, rows)];
    for (const m of key.matrices) {
      const offs = new Uint32Array(rows + 1), cols = [], vals = [];
      m.forEach((row, j) => { for (const [c, v] of row) { cols.push(c); vals.push(v); } offs[j + 1] = cols.length; });
      args.push(offs, Uint32Array.from(cols), kzgPack(vals, 32, 'coefficient', shareIdBytes));
    }
    const g1 = (p, what) => { const b = kzgG1(p); if (b.length !== 48) throw new Error('Invalid ' + what + ': expected 48 compressed bytes'); return b; };
    args.push(g1(key.alphaG1, 'alphaG1'), g1(key.betaG1, 'betaG1'), g16G2(key.betaG2, 'betaG2'), g1(key.deltaG1, 'deltaG1'), g16G2(key.deltaG2, 'deltaG2'));
    const query = (q, count, width, what, toBytes) => { if (!q || q.length !== count) throw new Error('Invalid ' + what + ': expected ' + count + ' points'); return kzgPack(q, width, what, toBytes); };
    args.push(query(key.aQuery, nVars, 48, 'aQuery', kzgG1), query(key.bG1Query, nVars, 48, 'bG1Query', kzgG1), query(key.bG2Query, nVars, 96, 'bG2Query', (p) => g16G2(p, 'bG2Query')),
      query(key.lQuery, nVars - nPublic - 1, 48, 'lQuery', kzgG1), query(key.hQuery, 2 ** log2n - 1, 48, 'hQuery', kzgG1));
    this.log2n = log2n; this.nVars = nVars; this.nPublic = nPublic;
    try { this.handle = native.groth16PkCreate(...args); } catch (e) {
      if (e && e.nblsCode === -5) { const err = new Error('Invalid key: a point does not decode, is outside the subgroup or is a zero point where none may stand'); err.status = e.status; throw err; }
      throw e;
    }
  }
  close() { if (this.handle) native.groth16PkDestroy(this.handle); this.handle = null; }
}
function groth16ProvingKey(key) { return new Groth16Pk(key); }
function groth16Prove(pk, witnesses, rs) {
  if (!(pk instanceof Groth16Pk) || !pk.handle) throw new Error('Expected an open Groth16Pk');
  let ws = witnesses;
  if (!(witnesses instanceof Uint8Array)) {
    if (!witnesses.length) throw new Error('Expected one witness or more');
    ws = new Uint8Array(witnesses.length * pk.nVars * 32);
    witnesses.forEach((z, i) => {
      if (z.length !== pk.nVars) throw new Error('Invalid witness: expected ' + pk.nVars + ' field elements');
      ws.set(kzgPack(z, 32, 'field element', shareIdBytes), i * pk.nVars * 32);
    });
  }
  const n = ws.length / (pk.nVars * 32);
  if (!n || !Number.isInteger(n)) throw new Error('Expected one witness or more of ' + pk.nVars + ' field elements of 32 bytes');
  let pairs = null;
  if (rs !== null && rs !== undefined) {
    if (rs.length !== n) throw new Error('Expected one pair [r, s] per witness');
    pairs = new Uint8Array(n * 64);
    rs.forEach((p, i) => { if (p.length !== 2) throw new Error('Expected one pair [r, s] per witness'); pairs.set(kzgPack(p, 32, 'blinding scalar', shareIdBytes), i * 64); });
  }
  const res = native.groth16Prove(pk.handle, ws, pairs);
  return { proofs: Array.from({ length: n }, (_, i) => res.out.subarray(192 * i, 192 * i + 192)), status: res.status };
}

// Points are held as affine wire bytes (what the engine consumes) or as the zero point.  The reference's constructor form
// new PointG1(x: Fp, y: Fp, z?: Fp) (index.ts:291) is accepted too: the projective triple is made affine on the host.
class PointG1 {
  constructor(aff, zero = false, z) {
    if (aff instanceof Fp) {
      const x = aff, y = zero; z = z === undefined ? Fp.ONE : z;
      if (!(y instanceof Fp) || !(z instanceof Fp)) throw new Error('Expected Fp coordinates');
      if (z.isZero()) { this.aff = new Uint8Array(96); this.zero = true; return; }
      const zi = z.invert();
      this.aff = concat(x.multiply(zi).toBytes(), y.multiply(zi).toBytes()); this.zero = false; return;
    }
    this.aff = aff; this.zero = zero;
  }
  // coordinates as the reference exposes them (affine representative, z = 1; the zero point is (1, 1, 0) as getZero(), math.ts:910-912)
  get x() { return this.zero ? Fp.ONE : Fp.fromBytes(this.aff.subarray(0, 48)); }
  get y() { return this.zero ? Fp.ONE : Fp.fromBytes(this.aff.subarray(48)); }
  get z() { return this.zero ? Fp.ZERO : Fp.ONE; }
  getZero() { return PointG1.ZERO; }
  fromAffineTuple(xy) { return new PointG1(xy[0], xy[1], Fp.ONE); }
  toAffineBatch(points) { return points.map((p) => p.toAffine()); }
  normalizeZ(points) { return points; }
  toString() { return this.zero ? 'Point<Zero>' : `Point<x=${this.x}, y=${this.y}>`; }
  // index.ts:452-454: millerLoop(P.pairingPrecomputes(), this.toAffine()); a Q whose table is already memoised is paired through the prepared path
  millerLoop(Q) {
    if (Q._lineTable && !this.zero) { ensureInit(); return Fp12.fromBytes(native.pairingPrepared(this.aff, Q._lineTable, false, false)); }
    return pairing(this, Q, false);
  }
  clearCofactor() {                                                                       // [x]P + P with x = |z| (index.ts:401-405), for any point of the curve
    if (this.zero) return this;
    ensureInit();
    const { out, status } = native.clearCofactor(false, this.aff);
    return status[0] === 1 ? PointG1.ZERO : new PointG1(out);
  }
  calcMultiplyPrecomputes() {} clearMultiplyPrecomputes() {}                               // window tables of the reference's host ladder: nothing to cache here
  static get ZERO() { return new PointG1(new Uint8Array(96), true); }
  static get BASE() {
    return new PointG1(hexToBytes('17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb' +
      '08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1'));
  }
  isZero() { return this.zero; }
  // reference index.ts:298-327
  // reference index.ts:331-350
  static async hashToCurve(msg, options) {
    msg = ensureBytes(msg); ensureInit();
    const dst = stringToBytes((options && options.DST) || htfDefaults.DST);
    return new PointG1(native.hashToCurve(0, msg, Uint32Array.from([0, msg.length]), dst));
  }
  static async encodeToCurve(msg, options) {
    msg = ensureBytes(msg); ensureInit();
    const dst = stringToBytes((options && options.DST) || htfDefaults.DST);
    return new PointG1(native.hashToCurve(1, msg, Uint32Array.from([0, msg.length]), dst));
  }
  static fromHex(bytes) {
    bytes = ensureBytes(bytes); ensureInit();
    if (bytes.length === 48) {
      const { out, status } = native.g1Decompress(bytes);
      if (status[0] === 1) return PointG1.ZERO;
      if (status[0]) throw new Error(G1_STATUS[status[0]]);
      return new PointG1(out);
    } else if (bytes.length === 96) {
      const { out, status } = native.decodePoints(0, bytes, 96);      // infinity flag, coordinates reduced by the Fp constructor, assertValidity (index.ts:317-325)
      if (status[0] === 1) return PointG1.ZERO;
      if (status[0]) throw new Error(G1_STATUS[status[0]]);
      return new PointG1(out);
    }
    throw new Error('Invalid point G1, expected 48/96 bytes');
  }
  assertValidity() {
    if (this.zero) return this;
    ensureInit();
    const st = native.g1Validate(this.aff).status[0];
    if (st) throw new Error(G1_STATUS[st]);
    return this;
  }
  negate() {
    if (this.zero) return this;
    const y = toBig(this.aff.subarray(48));
    const ny = y === 0n ? 0n : CURVE.P - y;
    return new PointG1(concat(this.aff.subarray(0, 48), hexToBytes(ny.toString(16).padStart(96, '0'))));
  }
  add(rhs) { return PointG1.sum([this, rhs]); }
  subtract(rhs) { return this.add(rhs.negate()); }
  double() { return this.add(this); }
  // reference math.ts:1048-1167 (multiplyUnsafe / multiply / multiplyPrecomputed: same group element), the engine's ladder
  multiply(scalar) {
    const k = scalarBytes(scalar);
    if (this.zero) return PointG1.ZERO;
    ensureInit();
    const { out, status } = native.g1Mul(this.aff, k);
    return status[0] ? PointG1.ZERO : new PointG1(out);
  }
  multiplyUnsafe(scalar) { return this.multiply(scalar); }
  multiplyPrecomputed(scalar) { return this.multiply(scalar); }
  static fromPrivateKey(privateKey) { return PointG1.BASE.multiply(normalizePrivKey(privateKey)); }
  static sum(points) {
    ensureInit();
    const nz = points.filter((p) => !p.zero);
    if (!nz.length) return PointG1.ZERO;
    const { out, status } = native.g1Sum(concat(...nz.map((p) => p.aff)));
    return status[0] === 1 ? PointG1.ZERO : new PointG1(out);
  }
  // sum_i [k_i]P_i on the GPU (bucket method); scalars: bigint | number, any non-negative value below 2^256.  Not in the reference
  // (its aggregatePublicKeys is the unweighted sum): the building block of random-linear-combination batch verification
  static msm(points, scalars) {
    ensureInit();
    if (points.length !== scalars.length) throw new Error('points / scalars length mismatch');
    const keep = points.map((p, i) => i).filter((i) => !points[i].zero);
    if (!keep.length) return PointG1.ZERO;
    const { out, status } = native.g1Msm(concat(...keep.map((i) => points[i].aff)), concat(...keep.map((i) => hexToBytes(BigInt(scalars[i]).toString(16).padStart(64, '0')))));
    return status[0] === 1 ? PointG1.ZERO : new PointG1(out);
  }
  // t-of-n threshold shares -> the group's public key: sum_k [lambda_k]share_k (combineSharesBatch above)
  static async combineShares(shares, ids) { return (await combineSharesBatch(PointG1, [{ shares, ids }]))[0]; }
  static combineSharesBatch(groups) { return combineSharesBatch(PointG1, groups); }
  // commitment polynomial (coefficients lowest degree first) -> the public keys of the shares with these identifiers (evalCommitmentBatch above)
  static async evalCommitment(coefs, ids) { return (await evalCommitmentBatch(PointG1, [{ coefs, ids }]))[0]; }
  static evalCommitmentBatch(groups) { return evalCommitmentBatch(PointG1, groups); }
  // KZG commitments and proofs are G1 points: verify_kzg_proof_batch / verify_blob_kzg_proof_batch of EIP-4844 (above), synchronous and on a worker thread
  static verifyKzgProofBatch(commitments, zs, ys, proofs, tauG2, opts) { return verifyKzgProofBatch(commitments, zs, ys, proofs, tauG2, opts); }
  static verifyKzgProofBatchAsync(commitments, zs, ys, proofs, tauG2, opts) { return verifyKzgProofBatchAsync(commitments, zs, ys, proofs, tauG2, opts); }
  static verifyBlobKzgProofBatch(blobs, commitments, proofs, tauG2, opts) { return verifyBlobKzgProofBatch(blobs, commitments, proofs, tauG2, opts); }
  static verifyBlobKzgProofBatchAsync(blobs, commitments, proofs, tauG2, opts) { return verifyBlobKzgProofBatchAsync(blobs, commitments, proofs, tauG2, opts); }
  // the prover's side against a KzgSetup (above): commitments, proofs at given points, blob proofs (commitments given, or computed first and returned)
  static get KzgSetup() { return KzgSetup; }
  static blobToKzgCommitments(setup, blobs) { return blobToKzgCommitments(setup, blobs); }
  static blobToKzgCommitmentsAsync(setup, blobs) { return blobToKzgCommitmentsAsync(setup, blobs); }
  static computeKzgProofs(setup, blobs, zs) { return computeKzgProofs(setup, blobs, zs); }
  static computeKzgProofsAsync(setup, blobs, zs) { return computeKzgProofsAsync(setup, blobs, zs); }
  static computeBlobKzgProofs(setup, blobs, commitments) { return computeBlobKzgProofs(setup, blobs, commitments); }
  static computeBlobKzgProofsAsync(setup, blobs, commitments) { return computeBlobKzgProofsAsync(setup, blobs, commitments); }
  // PeerDAS (above): the transform over Fr, the cells of blobs, and cells with their proofs against a KzgMonomialSetup
  static get KzgMonomialSetup() { return KzgMonomialSetup; }
  static frNtt(log2n, rows, toEvals, shifts) { return frNtt(log2n, rows, toEvals, shifts); }
  static frNttAsync(log2n, rows, toEvals, shifts) { return frNttAsync(log2n, rows, toEvals, shifts); }
  static computeCells(log2n, log2cell, blobs) { return computeCells(log2n, log2cell, blobs); }
  static computeCellsAsync(log2n, log2cell, blobs) { return computeCellsAsync(log2n, log2cell, blobs); }
  static computeCellsAndKzgProofs(setup, log2cell, blobs) { return computeCellsAndKzgProofs(setup, log2cell, blobs); }
  static computeCellsAndKzgProofsAsync(setup, log2cell, blobs) { return computeCellsAndKzgProofsAsync(setup, log2cell, blobs); }
  static recoverCells(log2n, log2cell, cellIndices, cells) { return recoverCells(log2n, log2cell, cellIndices, cells); }
  static recoverCellsAsync(log2n, log2cell, cellIndices, cells) { return recoverCellsAsync(log2n, log2cell, cellIndices, cells); }
  static recoverCellsAndKzgProofs(setup, log2cell, cellIndices, cells) { return recoverCellsAndKzgProofs(setup, log2cell, cellIndices, cells); }
  static recoverCellsAndKzgProofsAsync(setup, log2cell, cellIndices, cells) { return recoverCellsAndKzgProofsAsync(setup, log2cell, cellIndices, cells); }
  static verifyCellKzgProofBatch(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts) {
    return verifyCellKzgProofBatch(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts);
  }
  static verifyCellKzgProofBatchAsync(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts) {
    return verifyCellKzgProofBatchAsync(setup, log2cell, commitments, commitmentIndices, cellIndices, cells, proofs, tauCG2, opts);
  }
  // Groth16 (above): a verifying key on the device and the batched check of proofs against it
  static get Groth16Vk() { return Groth16Vk; }
  static verifyGroth16Batch(vk, proofs, inputs, opts) { return verifyGroth16Batch(vk, proofs, inputs, opts); }
  static verifyGroth16BatchAsync(vk, proofs, inputs, opts) { return verifyGroth16BatchAsync(vk, proofs, inputs, opts); }
  // the Groth16 prover (above): a proving key on the device and proofs from witnesses
  static get Groth16Pk() { return Groth16Pk; }
  static groth16ProvingKey(key) { return groth16ProvingKey(key); }
  static groth16Prove(pk, witnesses, rs) { return groth16Prove(pk, witnesses, rs); }
  equals(rhs) { return this.zero === rhs.zero && (this.zero || bytesToHex(this.aff) === bytesToHex(rhs.aff)); }
  // reference index.ts:359-381
  toHex(isCompressed = false) {
    this.assertValidity();
    if (isCompressed) {
      if (this.zero) return 'c' + '0'.repeat(95);
      const x = toBig(this.aff.subarray(0, 48)), y = toBig(this.aff.subarray(48));
      const flag = (y * 2n) / CURVE.P;
      return (x + flag * (1n << 381n) + (1n << 383n)).toString(16).padStart(96, '0');
    }
    if (this.zero) return '4'.padEnd(192, '0');
    return bytesToHex(this.aff);
  }
  toRawBytes(isCompressed = false) { return hexToBytes(this.toHex(isCompressed)); }
  toAffine() { return [this.x, this.y]; }     // [Fp, Fp] (math.ts:949-958); the zero point gives (1, 1) scaled by an undefined inverse in the reference: not meaningful
}

class PointG2 {
  constructor(aff, zero = false, z) {      // aff = x.c0 || x.c1 || y.c0 || y.c1 (192 bytes), or the reference's (x: Fp2, y: Fp2, z?: Fp2) (index.ts:472)
    if (aff instanceof Fp2) {
      const x = aff, y = zero; z = z === undefined ? Fp2.ONE : z;
      if (!(y instanceof Fp2) || !(z instanceof Fp2)) throw new Error('Expected Fp2 coordinates');
      if (z.isZero()) { this.aff = new Uint8Array(192); this.zero = true; return; }
      const zi = z.invert();
      this.aff = concat(x.multiply(zi).toBytes(), y.multiply(zi).toBytes()); this.zero = false; return;
    }
    this.aff = aff; this.zero = zero;
  }
  get x() { return this.zero ? Fp2.ONE : Fp2.fromBytes(this.aff.subarray(0, 96)); }
  get y() { return this.zero ? Fp2.ONE : Fp2.fromBytes(this.aff.subarray(96)); }
  get z() { return this.zero ? Fp2.ZERO : Fp2.ONE; }
  getZero() { return PointG2.ZERO; }
  fromAffineTuple(xy) { return new PointG2(xy[0], xy[1], Fp2.ONE); }
  toAffine() { return [this.x, this.y]; }
  toAffineBatch(points) { return points.map((p) => p.toAffine()); }
  normalizeZ(points) { return points; }
  toString() { return this.zero ? 'Point<Zero>' : `Point<x=${this.x}, y=${this.y}>`; }
  calcMultiplyPrecomputes() {} clearMultiplyPrecomputes() {}      // caches of the reference's host path
  // reference index.ts:659-672 (clear_cofactor_bls12381_g2: [x^2 - x - 1]P + [x - 1]psi(P) + psi^2(2P)), for any point of the curve
  clearCofactor() {
    if (this.zero) return this;
    ensureInit();
    const { out, status } = native.clearCofactor(true, this.aff);
    return status[0] === 1 ? PointG2.ZERO : new PointG2(out);
  }
  // reference index.ts:695-711: the 68 line triples of calcPairingPrecomputes (math.ts:1331-1371), memoised on the point.  Computed on the GPU
  // (nbls_g2_prepare); the wire form is kept beside the Fp2 view so that PointG1.millerLoop can hand the table straight back to the engine.
  clearPairingPrecomputes() { this._PPRECOMPUTES = undefined; this._lineTable = undefined; }
  pairingPrecomputes() {
    if (this._PPRECOMPUTES) return this._PPRECOMPUTES;
    if (this.zero) throw new Error('No pairings at point of Infinity');
    ensureInit();
    const t = native.g2Prepare(this.aff);
    this._lineTable = t;
    const ell = [];
    for (let j = 0; j < 68; j++) ell.push([0, 1, 2].map((k) => Fp2.fromBytes(t.subarray(288 * j + 96 * k, 288 * j + 96 * k + 96))));
    this._PPRECOMPUTES = ell;
    return ell;
  }
  static get ZERO() { return new PointG2(new Uint8Array(192), true); }
  static get BASE() {
    return new PointG2(hexToBytes('024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8' +
      '13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e' +
      '0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801' +
      '0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be'));
  }
  isZero() { return this.zero; }
  // reference index.ts:481-490
  static async hashToCurve(msg, options) {
    msg = ensureBytes(msg); ensureInit();
    const dst = stringToBytes((options && options.DST) || htfDefaults.DST);
    return new PointG2(native.hashToG2(msg, Uint32Array.from([0, msg.length]), dst));
  }
  // reference index.ts:491-497
  static async encodeToCurve(msg, options) {
    msg = ensureBytes(msg); ensureInit();
    const dst = stringToBytes((options && options.DST) || htfDefaults.DST);
    return new PointG2(native.hashToCurve(2, msg, Uint32Array.from([0, msg.length]), dst));
  }
  // reference index.ts:500-530: 96 bytes, or 192 bytes read as two 96-byte integers z1 || z2
  static fromSignature(hex) {
    hex = ensureBytes(hex); ensureInit();
    const half = hex.length / 2;
    if (half !== 48 && half !== 96) throw new Error('Invalid compressed signature length, must be 96 or 192');
    const { out, status } = native.decodePoints(2, hex, hex.length);
    if (status[0] === 1) return PointG2.ZERO;
    if (status[0]) throw new Error(G2_STATUS[status[0]]);
    return new PointG2(out);
  }
  // reference index.ts:532-579: 96 compressed bytes (flag rules, the root named by the S bit, NO subgroup check) or 192 uncompressed bytes
  // x.c1 || x.c0 || y.c1 || y.c0 with the infinity flag 0x40, followed by assertValidity
  static fromHex(bytes) {
    bytes = ensureBytes(bytes);
    const m_byte = bytes[0] & 0xe0;
    if (m_byte === 0x20 || m_byte === 0x60 || m_byte === 0xe0) throw new Error('Invalid encoding flag: ' + m_byte);
    const bitC = m_byte & 0x80;
    if (!((bytes.length === 96 && bitC) || (bytes.length === 192 && !bitC))) throw new Error('Invalid point G2, expected 96/192 bytes');
    ensureInit();
    const { out, status } = native.decodePoints(1, bytes, bytes.length);
    if (status[0] === 1) return PointG2.ZERO;
    if (status[0]) throw new Error(bytes.length === 96 ? 'Invalid compressed G2 point' : G2_STATUS[status[0]]);
    return new PointG2(out);
  }
  assertValidity() {
    if (this.zero) return this;
    ensureInit();
    const st = native.g2Validate(this.aff).status[0];
    if (st) throw new Error(G2_STATUS[st]);
    return this;
  }
  add(rhs) { return PointG2.sum([this, rhs]); }
  negate() {
    if (this.zero) return this;
    const neg = (b) => { const v = toBig(b); return hexToBytes((v === 0n ? 0n : CURVE.P - v).toString(16).padStart(96, '0')); };
    return new PointG2(concat(this.aff.subarray(0, 96), neg(this.aff.subarray(96, 144)), neg(this.aff.subarray(144, 192))));
  }
  subtract(rhs) { return this.add(rhs.negate()); }
  double() { return this.add(this); }
  multiply(scalar) {
    const k = scalarBytes(scalar);
    if (this.zero) return PointG2.ZERO;
    ensureInit();
    const { out, status } = native.g2Mul(this.aff, k);
    return status[0] ? PointG2.ZERO : new PointG2(out);
  }
  multiplyUnsafe(scalar) { return this.multiply(scalar); }
  multiplyPrecomputed(scalar) { return this.multiply(scalar); }
  static fromPrivateKey(privateKey) { return PointG2.BASE.multiply(normalizePrivKey(privateKey)); }
  static sum(points) {
    ensureInit();
    const nz = points.filter((p) => !p.zero);
    if (!nz.length) return PointG2.ZERO;
    const { out, status } = native.g2Sum(concat(...nz.map((p) => p.aff)));
    return status[0] === 1 ? PointG2.ZERO : new PointG2(out);
  }
  static msm(points, scalars) {
    ensureInit();
    if (points.length !== scalars.length) throw new Error('points / scalars length mismatch');
    const keep = points.map((p, i) => i).filter((i) => !points[i].zero);
    if (!keep.length) return PointG2.ZERO;
    const { out, status } = native.g2Msm(concat(...keep.map((i) => points[i].aff)), concat(...keep.map((i) => hexToBytes(BigInt(scalars[i]).toString(16).padStart(64, '0')))));
    return status[0] === 1 ? PointG2.ZERO : new PointG2(out);
  }
  // t-of-n threshold shares -> the group's signature: sum_k [lambda_k]share_k (combineSharesBatch above)
  static async combineShares(shares, ids) { return (await combineSharesBatch(PointG2, [{ shares, ids }]))[0]; }
  static combineSharesBatch(groups) { return combineSharesBatch(PointG2, groups); }
  // the same for schemes whose keys live in G2 (evalCommitmentBatch above)
  static async evalCommitment(coefs, ids) { return (await evalCommitmentBatch(PointG2, [{ coefs, ids }]))[0]; }
  static evalCommitmentBatch(groups) { return evalCommitmentBatch(PointG2, groups); }
  equals(rhs) { return this.zero === rhs.zero && (this.zero || bytesToHex(this.aff) === bytesToHex(rhs.aff)); }
  // reference index.ts:586-598
  toSignature() {
    if (this.zero) return hexToBytes('c' + '0'.repeat(191));
    const a = this.aff, x0 = a.subarray(0, 48), x1 = toBig(a.subarray(48, 96)), y0 = toBig(a.subarray(96, 144)), y1 = toBig(a.subarray(144, 192));
    const tmp = y1 > 0n ? y1 * 2n : y0 * 2n;
    const z1 = x1 + (tmp / CURVE.P) * (1n << 381n) + (1n << 383n);
    return concat(hexToBytes(z1.toString(16).padStart(96, '0')), x0);
  }
  toHex(isCompressed = false) {
    this.assertValidity();
    if (isCompressed) return bytesToHex(this.toSignature());
    if (this.zero) return '4'.padEnd(384, '0');
    const a = this.aff;
    return bytesToHex(concat(a.subarray(48, 96), a.subarray(0, 48), a.subarray(144, 192), a.subarray(96, 144)));
  }
  toRawBytes(isCompressed = false) { return hexToBytes(this.toHex(isCompressed)); }
}

// ---- reference index.ts:715-722
function pairing(P, Q, withFinalExponent = true) {
  if (P.isZero() || Q.isZero()) throw new Error('No pairings at point of Infinity');
  ensureInit();
  const { out, status } = native.pairingBatch(P.aff, Q.aff, withFinalExponent, true);
  if (status[0]) throw new Error(status[0] >= 10 ? G2_STATUS[status[0] - 10] : G1_STATUS[status[0]]);
  return Fp12.fromBytes(out);
}
// additive: n independent pairings in one call; points are PointG1[] / PointG2[] or packed affine byte arrays
function pairingBatch(Ps, Qs, withFinalExponent = true, validate = true) {
  ensureInit();
  const g1 = Ps instanceof Uint8Array ? Ps : concat(...Ps.map((p) => p.aff));
  const g2 = Qs instanceof Uint8Array ? Qs : concat(...Qs.map((q) => q.aff));
  return native.pairingBatch(g1, g2, withFinalExponent, validate);
}
function millerProduct(Ps, Qs, finalExp = true, validate = true) {
  ensureInit();
  const g1 = Ps instanceof Uint8Array ? Ps : concat(...Ps.map((p) => p.aff));
  const g2 = Qs instanceof Uint8Array ? Qs : concat(...Qs.map((q) => q.aff));
  return native.millerProduct(g1, g2, finalExp, validate);
}

function normP1(point) { return point instanceof PointG1 ? point : PointG1.fromHex(point); }
function normP2(point) { return point instanceof PointG2 ? point : PointG2.fromSignature(point); }
async function normP2Hash(point) { return point instanceof PointG2 ? point : PointG2.hashToCurve(point); }

// reference index.ts:269-279
function normalizePrivKey(key) {
  let int;
  if (key instanceof Uint8Array && key.length === 32) int = toBig(key);
  else if (typeof key === 'string' && key.length === 64) int = BigInt('0x' + key);
  else if (typeof key === 'number' && key > 0 && Number.isSafeInteger(key)) int = BigInt(key);
  else if (typeof key === 'bigint' && key > 0n) int = key;
  else throw new TypeError('Expected valid private key');
  int = ((int % CURVE.r) + CURVE.r) % CURVE.r;
  if (!(0n < int && int < CURVE.r)) throw new Error('Private key must be 0 < key < CURVE.r');
  return int;
}
const keyBytes = (k) => hexToBytes(normalizePrivKey(k).toString(16).padStart(64, '0'));
// reference index.ts:738-740: PointG1.fromPrivateKey(privateKey).toRawBytes(true)
function getPublicKeys(privateKeys) {
  ensureInit();
  const { out } = native.g1Mul(null, concat(...privateKeys.map(keyBytes)));
  return privateKeys.map((_, i) => new PointG1(out.slice(96 * i, 96 * i + 96)).toRawBytes(true));
}
function getPublicKey(privateKey) { return getPublicKeys([privateKey])[0]; }
// reference index.ts:744-752
async function sign(message, privateKey) {
  ensureInit();
  if (message instanceof PointG2) {
    message.assertValidity();
    const { out } = native.g2Mul(message.aff, keyBytes(privateKey));
    return new PointG2(out);
  }
  return (await signBatch([message], [privateKey]))[0];
}
async function signBatch(messages, privateKeys) {
  ensureInit();
  if (messages.length !== privateKeys.length) throw new Error('Expected equal number of messages and private keys');
  const msgs = messages.map(ensureBytes);
  const offs = new Uint32Array(msgs.length + 1);
  msgs.forEach((m, i) => { offs[i + 1] = offs[i] + m.length; });
  const { out } = await native.signBatchAsync(concat(...msgs), offs, stringToBytes(htfDefaults.DST), concat(...privateKeys.map(keyBytes)));   // worker thread: the event loop keeps running
  return msgs.map((_, i) => new PointG2(out.slice(192 * i, 192 * i + 192)).toSignature());
}

// reference index.ts:756-767: e(-P, H(m)) * e(G, S) == 1 with one final exponentiation.
// Wire-format inputs (96-byte signature, 48-byte key, message bytes: what a caller of the reference normally passes) take ONE engine call on a worker thread
// (nbls_verify_batch with n = 1: key decode + subgroup check, hash-to-G2 and signature decode overlap on three streams, then two Miller loops and one final
// exponentiation) and leave the event loop free; anything else -- point objects, other encodings, and every input the fast path rejects -- goes through the
// step-by-step form below, which raises the reference's exceptions.
async function verify(signature, message, publicKey) {
  ensureInit();
  if (!(signature instanceof PointG2) && !(message instanceof PointG2) && !(publicKey instanceof PointG1)) {
    let sig, msg, pk;
    try { sig = ensureBytes(signature); msg = ensureBytes(message); pk = ensureBytes(publicKey); } catch (e) { sig = null; }
    // the infinity flag (bit 6 of the first byte) is left to the slow path: the reference throws 'No pairings at point of Infinity' where verifyBatch's engine call answers false
    if (sig && sig.length === 96 && pk.length === 48 && !(sig[0] & 0x40) && !(pk[0] & 0x40)) {
      const r = await native.verifyBatchAsync(sig, msg, Uint32Array.of(0, msg.length), pk, stringToBytes(htfDefaults.DST));
      if (!r.code) return r.ok;
    }
  }
  const P = normP1(publicKey);
  const Hm = await normP2Hash(message);
  const S = normP2(signature);
  if (P.isZero() || Hm.isZero() || S.isZero()) throw new Error('No pairings at point of Infinity');
  const r = native.millerProduct(concat(P.negate().aff, PointG1.BASE.aff), concat(Hm.aff, S.aff), true, true);
  if (r.code) { const st = r.status[0] || r.status[1]; throw new Error(st >= 10 ? G2_STATUS[st - 10] : G1_STATUS[st]); }
  return Fp12.fromBytes(r.out).equals(Fp12.ONE);
}
// Sets that sign the same bytes (the attestations of one slot share a handful of signing roots) need ONE hash-to-G2 and ONE Miller loop per message: wire[i] = [sig, msg, ...] or
// null for the n sets of a call, w of them wire-format.  Returns null when no two wire sets have equal messages (the caller then makes the call it always made), else the distinct
// messages packed (msgs, offs) and index[k] = the message of the k-th wire set.  A Map keyed by the message bytes read as a latin1 string, one pass, no spread over n arrays.
// NBLS_JS_SHARED=0 in the environment: never group (tests compare the two routes).
function groupWireMessages(wire, w) {
  if (w < 2 || process.env.NBLS_JS_SHARED === '0') return null;
  const seen = new Map(), distinct = [], index = new Uint32Array(w);
  let total = 0;
  for (let i = 0, k = 0; i < wire.length; i++) {
    if (!wire[i]) continue;
    const msg = wire[i][1], key = Buffer.from(msg.buffer, msg.byteOffset, msg.length).toString('latin1');
    let g = seen.get(key);
    if (g === undefined) { g = distinct.length; seen.set(key, g); distinct.push(msg); total += msg.length; }
    index[k++] = g;
  }
  if (distinct.length === w) return null;
  const msgs = new Uint8Array(total), offs = new Uint32Array(distinct.length + 1);
  for (let g = 0; g < distinct.length; g++) { msgs.set(distinct[g], offs[g]); offs[g + 1] = offs[g] + distinct[g].length; }
  return { msgs, offs, index };
}
// verify(signature_i, message_i, publicKey_i) for n independent sets at once (no reference counterpart; blst's verify_multiple_aggregate_signatures): the wire-format sets
// take ONE engine call on a worker thread (nbls_verify_multiple: a random linear combination with weights seeded from the OS, n + 1 Miller loops and one final
// exponentiation, a per-set pass only when that check fails).  Sets with point objects, and every set the engine reports as one where verify throws (a point that does not
// decode, a zero point), go through verify itself, in index order: the first set that throws there throws the reference's message.  The inputs are packed into buffers
// allocated once (a spread of 100k+ arrays into one call throws RangeError).  When at least two wire sets have equal messages the call is nbls_verify_multiple_shared on the
// distinct messages (groupWireMessages): the same statuses, one hash and one Miller loop per message.
async function verifyMultipleSignatures(sets) {
  if (!Array.isArray(sets) || !sets.length) throw new Error('Expected non-empty array');
  ensureInit();
  const n = sets.length, wire = new Array(n);
  let w = 0, total = 0;
  for (let i = 0; i < n; i++) {
    const { signature, message, publicKey } = sets[i];
    wire[i] = null;
    if (signature instanceof PointG2 || message instanceof PointG2 || publicKey instanceof PointG1) continue;
    let sig, msg, pk;
    try { sig = ensureBytes(signature); msg = ensureBytes(message); pk = ensureBytes(publicKey); } catch (e) { continue; }
    if (sig.length !== 96 || pk.length !== 48) continue;
    wire[i] = [sig, msg, pk]; w++; total += msg.length;
  }
  let status = null;
  if (w) {
    const sigs = new Uint8Array(96 * w), pks = new Uint8Array(48 * w), msgs = new Uint8Array(total), offs = new Uint32Array(w + 1);
    for (let i = 0, k = 0; i < n; i++) {
      if (!wire[i]) continue;
      const [sig, msg, pk] = wire[i];
      sigs.set(sig, 96 * k); pks.set(pk, 48 * k); msgs.set(msg, offs[k]); offs[k + 1] = offs[k] + msg.length; k++;
    }
    const grp = groupWireMessages(wire, w);
    status = (grp ? await native.verifyMultipleSharedAsync(sigs, grp.msgs, grp.offs, grp.index, pks, stringToBytes(htfDefaults.DST))
      : await native.verifyMultipleAsync(sigs, msgs, offs, pks, stringToBytes(htfDefaults.DST))).status;   // worker thread: the event loop keeps running
  }
  let all = true;
  for (let i = 0, k = 0; i < n; i++) {
    if (wire[i]) {
      const st = status[k++];
      if (st === 0) continue;
      if (st === 9) { all = false; continue; }      // NBLS_ST_NOT_VERIFIED
    }
    const { signature, message, publicKey } = sets[i];
    if (!(await verify(signature, message, publicKey))) all = false;
  }
  return all;
}
// verify(signature_j, message_j, aggregatePublicKeys(publicKeys_j)) for n sets at once (no reference counterpart; blst's aggregate-verify of many sets): the wire-format sets take
// ONE engine call on a worker thread (nbls_verify_aggregates: the keys of every set summed on the device, then one random linear combination over the sets with weights seeded from
// the OS).  Sets with point objects, and every set the engine reports with a status other than 0 or 9 (a key or signature that does not decode, a zero aggregate or signature), go
// through verify(signature, message, aggregatePublicKeys(publicKeys)) itself, in index order: the first set that throws there throws the reference's message.  The inputs are packed
// in one pass into buffers allocated once (a spread of 100k+ arrays into one call throws RangeError).  Equal messages among the wire sets: nbls_verify_aggregates_shared, as in
// verifyMultipleSignatures.
async function verifyMultipleAggregateSignatures(sets) {
  if (!Array.isArray(sets) || !sets.length) throw new Error('Expected non-empty array');
  ensureInit();
  const n = sets.length, wire = new Array(n);
  let w = 0, total = 0, nkeys = 0;
  for (let i = 0; i < n; i++) {
    const { signature, message, publicKeys } = sets[i];
    wire[i] = null;
    if (!Array.isArray(publicKeys) || !publicKeys.length || signature instanceof PointG2 || message instanceof PointG2) continue;
    let sig, msg, ok = true;
    const keys = new Array(publicKeys.length);
    try {
      sig = ensureBytes(signature); msg = ensureBytes(message);
      for (let k = 0; k < publicKeys.length && ok; k++) {
        if (publicKeys[k] instanceof PointG1) { ok = false; break; }
        keys[k] = ensureBytes(publicKeys[k]);
        if (keys[k].length !== 48) ok = false;
      }
    } catch (e) { continue; }
    if (!ok || sig.length !== 96) continue;
    wire[i] = [sig, msg, keys]; w++; total += msg.length; nkeys += keys.length;
  }
  let status = null;
  if (w) {
    const sigs = new Uint8Array(96 * w), pks = new Uint8Array(48 * nkeys), msgs = new Uint8Array(total), offs = new Uint32Array(w + 1), koffs = new Uint32Array(w + 1);
    for (let i = 0, j = 0; i < n; i++) {
      if (!wire[i]) continue;
      const [sig, msg, keys] = wire[i];
      sigs.set(sig, 96 * j); msgs.set(msg, offs[j]); offs[j + 1] = offs[j] + msg.length;
      let at = koffs[j];
      for (let k = 0; k < keys.length; k++, at++) pks.set(keys[k], 48 * at);
      koffs[j + 1] = at; j++;
    }
    const grp = groupWireMessages(wire, w);
    status = (grp ? await native.verifyAggregatesSharedAsync(sigs, grp.msgs, grp.offs, grp.index, pks, koffs, stringToBytes(htfDefaults.DST))
      : await native.verifyAggregatesAsync(sigs, msgs, offs, pks, koffs, stringToBytes(htfDefaults.DST))).status;   // worker thread: the event loop keeps running
  }
  let all = true;
  for (let i = 0, j = 0; i < n; i++) {
    if (wire[i]) {
      const st = status[j++];
      if (st === 0) continue;
      if (st === 9) { all = false; continue; }      // NBLS_ST_NOT_VERIFIED
    }
    const { signature, message, publicKeys } = sets[i];
    if (!(await verify(signature, message, aggregatePublicKeys(publicKeys)))) all = false;
  }
  return all;
}
// reference index.ts:771-788
function aggregatePublicKeys(publicKeys) {
  if (!publicKeys.length) throw new Error('Expected non-empty array');
  const agg = PointG1.sum(publicKeys.map(normP1));
  if (publicKeys[0] instanceof PointG1) return agg.assertValidity();
  return agg.toRawBytes(true);
}
function aggregateSignatures(signatures) {
  if (!signatures.length) throw new Error('Expected non-empty array');
  const agg = PointG2.sum(signatures.map(normP2));
  if (signatures[0] instanceof PointG2) return agg.assertValidity();
  return agg.toSignature();
}
// reference index.ts:792-821
async function verifyBatch(signature, messages, publicKeys) {
  if (!messages.length) throw new Error('Expected non-empty messages array');
  if (publicKeys.length !== messages.length) throw new Error('Pubkey count should equal msg count');
  ensureInit();
  const allWire = !(signature instanceof PointG2) && messages.every((m) => !(m instanceof PointG2)) && publicKeys.every((k) => !(k instanceof PointG1)) &&
    publicKeys.every((k) => ensureBytes(k).length === 48) && ensureBytes(signature).length === 96;
  if (allWire) {
    // fast path: one engine call (hex inputs hash to distinct message objects in the reference, so no grouping applies)
    const msgs = messages.map(ensureBytes);
    const offs = new Uint32Array(msgs.length + 1); msgs.forEach((m, i) => { offs[i + 1] = offs[i] + m.length; });
    const r = await native.verifyBatchAsync(ensureBytes(signature), concat(...msgs), offs, concat(...publicKeys.map(ensureBytes)), stringToBytes(htfDefaults.DST));   // worker thread: the event loop keeps running
    if (r.code) { normP2(signature); publicKeys.forEach(normP1); throw new Error('invalid point'); }   // re-derive the reference's exception
    return r.ok;
  }
  const sig = normP2(signature);
  const nMessages = await Promise.all(messages.map(normP2Hash));
  const nPublicKeys = publicKeys.map(normP1);
  try {
    const g1 = [], g2 = [];
    for (const message of new Set(nMessages)) {            // group keys per identical message OBJECT (reference index.ts:804-809)
      const group = PointG1.sum(nMessages.map((m, i) => (m === message ? nPublicKeys[i] : null)).filter((p) => p));
      if (group.isZero() || message.isZero()) throw new Error('No pairings at point of Infinity');
      g1.push(group); g2.push(message);
    }
    if (sig.isZero()) throw new Error('No pairings at point of Infinity');
    g1.push(PointG1.BASE.negate()); g2.push(sig);
    const r = native.millerProduct(concat(...g1.map((p) => p.aff)), concat(...g2.map((p) => p.aff)), true, true);
    if (r.code) throw new Error('invalid point');
    return Fp12.fromBytes(r.out).equals(Fp12.ONE);
  } catch (e) {
    return false;
  }
}

// ---- utils (reference index.ts:94-149): host-side helpers around the signature API
const nodeCrypto = require('crypto');
const sha256 = async (message) => Uint8Array.from(nodeCrypto.createHash('sha256').update(message).digest());
const modBig = (a, b) => { const r = a % b; return r >= 0n ? r : b + r; };
// expand_message_xmd of RFC 9380 section 5.3.1 (reference index.ts:207-231); H is an async digest with 32-byte output and 64-byte blocks
async function expandMessageXMD(msg, DST, lenInBytes, H = sha256) {
  if (DST.length > 255) DST = await H(concat(stringToBytes('H2C-OVERSIZE-DST-'), DST));
  const bInBytes = 32, rInBytes = 64, ell = Math.ceil(lenInBytes / bInBytes);
  if (ell > 255) throw new Error('Invalid xmd length');
  const dstPrime = concat(DST, Uint8Array.of(DST.length));
  const lib = Uint8Array.of((lenInBytes >> 8) & 0xff, lenInBytes & 0xff);
  const b0 = await H(concat(new Uint8Array(rInBytes), msg, lib, Uint8Array.of(0), dstPrime));
  const blocks = [await H(concat(b0, Uint8Array.of(1), dstPrime))];
  for (let i = 2; i <= ell; i++) blocks.push(await H(concat(b0.map((v, k) => v ^ blocks[i - 2][k]), Uint8Array.of(i), dstPrime)));
  return concat(...blocks).slice(0, lenInBytes);
}
// hash_to_field (reference index.ts:236-267): count elements of F_{p^m}, each coordinate from L = ceil((log2 p + k) / 8) uniform bytes
async function hashToField(msg, count, options = {}) {
  const o = { DST: htfDefaults.DST, p: CURVE.P, m: 2, k: 128, expand: true, hash: sha256, ...options };
  const L = Math.ceil((o.p.toString(2).length + o.k) / 8), len = count * o.m * L;
  const bytes = o.expand ? await expandMessageXMD(msg, stringToBytes(o.DST), len, o.hash) : msg;
  const u = [];
  for (let i = 0; i < count; i++) {
    const e = [];
    for (let j = 0; j < o.m; j++) { const off = L * (j + i * o.m); e.push(modBig(toBig(bytes.subarray(off, off + L)), o.p)); }
    u.push(e);
  }
  return u;
}
const utils = {
  hashToField, expandMessageXMD, sha256, mod: modBig,
  hashToPrivateKey: (hash) => {          // FIPS 186 B.1.1: 40..1024 uniform bytes -> key (reference index.ts:105-113)
    hash = ensureBytes(hash);
    if (hash.length < 40 || hash.length > 1024) throw new Error('Expected 40-1024 bytes of private key as per FIPS 186');
    const num = modBig(toBig(hash), CURVE.r);
    if (num === 0n || num === 1n) throw new Error('Invalid private key');
    return hexToBytes(num.toString(16).padStart(64, '0'));
  },
  randomBytes: (bytesLength = 32) => Uint8Array.from(nodeCrypto.randomBytes(bytesLength)),
  randomPrivateKey: () => utils.hashToPrivateKey(utils.randomBytes(40)),
  bytesToHex, hexToBytes, stringToBytes,
  getDSTLabel() { return htfDefaults.DST; },
  setDSTLabel(newLabel) {
    if (typeof newLabel !== 'string' || newLabel.length > 2048 || newLabel.length === 0) throw new TypeError('Invalid DST');
    htfDefaults.DST = newLabel;
  },
};

module.exports = { CURVE, Fp, Fr, Fp2, Fp6, Fp12, PointG1, PointG2, pairing, pairingBatch, millerProduct, getPublicKey, getPublicKeys, sign, signBatch, verify, verifyBatch, verifyMultipleSignatures, verifyMultipleAggregateSignatures,
  aggregatePublicKeys, aggregateSignatures, utils, init: (dev, contexts) => { if (contexts === undefined) native.init(dev || 0); else native.init(dev || 0, contexts); inited = true; } };
