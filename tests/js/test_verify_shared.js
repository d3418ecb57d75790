// GPU test of the facade's verifyMultipleSignatures / verifyMultipleAggregateSignatures with repeated messages (noble-bls12-381_amd/js/index.js): wire-format sets that share
// messages take the native shared calls (nbls_verify_multiple_shared / nbls_verify_aggregates_shared) -- counted here through a wrapper around the addon -- and return or throw
// exactly what they do with the grouping disabled (NBLS_JS_SHARED=0), which is also what verify(...) per set gives; sets without equal messages make the call they always made.
'use strict';
const fs = require('fs'), zlib = require('zlib'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const addonPath = require.resolve(path.join(JS, 'nbls_napi.node'));
const real = require(addonPath);
const calls = {};
const counted = {};
for (const k of Object.keys(real)) counted[k] = (...a) => { calls[k] = (calls[k] || 0) + 1; return real[k](...a); };
require.cache[addonPath].exports = counted;       // the facade requires the same path: it gets the counting wrapper
const bls = require(path.join(JS, 'index.js'));
const load = (f) => JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(__dirname, '..', 'golden', f))).toString());
const gold = load('ref_vectors.json.gz');
const { bytesToHex, stringToBytes } = bls.utils;

async function outcome(f) { try { return { v: await f() }; } catch (e) { return { e: e.message }; } }
const taken = (names) => names.map((k) => calls[k] || 0);
const MULTI = ['verifyMultipleSharedAsync', 'verifyMultipleAsync'], AGG = ['verifyAggregatesSharedAsync', 'verifyAggregatesAsync'];
// f(sets) with the grouping on and off: the same outcome, the shared call taken exactly once when `shared`, else the plain one
async function both(f, names, sets, shared) {
  let before = taken(names);
  delete process.env.NBLS_JS_SHARED;
  const on = await outcome(() => f(sets));
  let after = taken(names);
  assert.deepStrictEqual([after[0] - before[0], after[1] - before[1]], shared ? [1, 0] : [0, 1], 'grouping on: ' + names[shared ? 0 : 1] + ' expected');
  process.env.NBLS_JS_SHARED = '0';
  before = taken(names);
  const off = await outcome(() => f(sets));
  after = taken(names);
  delete process.env.NBLS_JS_SHARED;
  assert.deepStrictEqual([after[0] - before[0], after[1] - before[1]], [0, 1], 'grouping off: the plain call expected');
  assert.deepStrictEqual(on, off);
  return on;
}

(async () => {
  const R = bls.CURVE.r, N = 600, M = 7;
  const sks = [];
  for (let i = 0; i < N; i++) sks.push(((BigInt(i) + 1n) * 0x9e3779b97f4a7c15f39cc0605cedc835n + 777n) % R);
  const pks = bls.getPublicKeys(sks);
  const roots = [];
  for (let g = 0; g < M; g++) roots.push(stringToBytes('signing root ' + g));
  roots.push(new Uint8Array(0));                                        // an empty message is a message
  const which = (i) => (i * 5 + (i >> 3)) % roots.length;
  const msgs = sks.map((_, i) => roots[which(i)]);
  const sigs = await bls.signBatch(msgs, sks);
  // even sets as Uint8Array, odd sets as hex strings
  const sets = sks.map((_, i) => (i % 2 === 0 ? { signature: sigs[i], message: msgs[i], publicKey: pks[i] }
    : { signature: bytesToHex(sigs[i]), message: bytesToHex(msgs[i]), publicKey: bytesToHex(pks[i]) }));
  const ref = (s) => bls.verify(s.signature, s.message, s.publicKey);
  assert.strictEqual(await ref(sets[0]), true);
  assert.strictEqual(await ref(sets[N - 1]), true);
  assert.deepStrictEqual(await both(bls.verifyMultipleSignatures, MULTI, sets, true), { v: true });
  // distinct messages: the call it always made
  const distinct = sets.slice(0, roots.length);
  assert.strictEqual(new Set(distinct.map((_, i) => which(i))).size, roots.length);
  assert.deepStrictEqual(await both(bls.verifyMultipleSignatures, MULTI, distinct, false), { v: true });
  // two signers of one message with their signatures exchanged
  const a = 10, b = sets.findIndex((_, i) => i > a && i % 2 === 0 && which(i) === which(a));
  const swapped = sets.slice();
  swapped[a] = { ...sets[a], signature: sets[b].signature }; swapped[b] = { ...sets[b], signature: sets[a].signature };
  assert.strictEqual(await ref(swapped[a]), false);
  assert.deepStrictEqual(await both(bls.verifyMultipleSignatures, MULTI, swapped, true), { v: false });
  // a set pointed at another root
  const wrong = sets.slice();
  wrong[77] = { ...sets[77], message: roots[(which(77) + 1) % M] };
  assert.strictEqual(await ref(wrong[77]), false);
  assert.deepStrictEqual(await both(bls.verifyMultipleSignatures, MULTI, wrong, true), { v: false });
  // a key outside the subgroup inside a group: verify throws, and so does the batch, with the same message (the forged set behind it changes nothing)
  const g1sub = gold.codec.g1.find((v) => /subgroup/.test(v.result)).hex;
  const bad = wrong.slice();
  bad[40] = { ...sets[40], publicKey: g1sub };
  const want = await outcome(() => ref(bad[40]));
  assert.ok(want.e, 'verify should throw');
  assert.deepStrictEqual(await both(bls.verifyMultipleSignatures, MULTI, bad, true), want);
  // point objects among the sets go through verify itself; the wire sets still share messages
  const pts = sets.slice(0, 30).map((s, i) => (i % 5 === 0 ? { ...s, publicKey: bls.PointG1.fromHex(s.publicKey) } : s));
  assert.deepStrictEqual(await both(bls.verifyMultipleSignatures, MULTI, pts, true), { v: true });

  // aggregates: 120 sets of 1 .. 9 keys over 5 roots
  const A = 120, idx = [], aggSks = [], amsgs = [];
  for (let j = 0; j < A; j++) {
    const s = [];
    let sum = 0n;
    for (let k = 0; k <= j % 9; k++) { const i = (j * 13 + 41 * k) % N; s.push(i); sum += sks[i]; }
    idx.push(s); aggSks.push(sum % R); amsgs.push(roots[(j * 7) % 5]);
  }
  const asigs = await bls.signBatch(amsgs, aggSks);
  const asets = idx.map((s, j) => (j % 2 === 0 ? { signature: asigs[j], message: amsgs[j], publicKeys: s.map((i) => pks[i]) }
    : { signature: bytesToHex(asigs[j]), message: bytesToHex(amsgs[j]), publicKeys: s.map((i) => bytesToHex(pks[i])) }));
  const aref = (s) => bls.verify(s.signature, s.message, bls.aggregatePublicKeys(s.publicKeys));
  assert.strictEqual(await aref(asets[0]), true);
  assert.strictEqual(await aref(asets[A - 1]), true);
  assert.deepStrictEqual(await both(bls.verifyMultipleAggregateSignatures, AGG, asets, true), { v: true });
  assert.deepStrictEqual(await both(bls.verifyMultipleAggregateSignatures, AGG, asets.slice(0, 5), false), { v: true });     // five sets, five roots
  const forged = asets.slice();
  forged[50] = { ...asets[50], signature: asets[55].signature };          // sets 50 and 55 sign the same root
  assert.strictEqual(amsgs[50], amsgs[55]);
  assert.strictEqual(await aref(forged[50]), false);
  assert.deepStrictEqual(await both(bls.verifyMultipleAggregateSignatures, AGG, forged, true), { v: false });
  const abad = forged.slice();
  abad[20] = { ...asets[20], publicKeys: asets[20].publicKeys.map((k, i) => (i === 1 ? g1sub : k)) };
  const awant = await outcome(() => aref(abad[20]));
  assert.ok(awant.e, 'aggregatePublicKeys should throw');
  assert.deepStrictEqual(await both(bls.verifyMultipleAggregateSignatures, AGG, abad, true), awant);
  assert.ok(calls.verifyMultipleSharedAsync >= 5 && calls.verifyAggregatesSharedAsync >= 3);
  console.log('JS shared-message verification ok');
})().catch((e) => { console.error(e); process.exit(1); });
