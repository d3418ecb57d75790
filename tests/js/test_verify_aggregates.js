// GPU test of the facade's verifyMultipleAggregateSignatures (noble-bls12-381_amd/js/index.js): 2,000 sets of 64 keys from Uint8Array and hex inputs, a forged set, a set with a key
// that does not decode (the reference's message is thrown), and sets with point objects, against verify(signature, message, aggregatePublicKeys(publicKeys)).
'use strict';
const fs = require('fs'), zlib = require('zlib'), path = require('path'), assert = require('assert');
const bls = require(path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js', 'index.js'));
const load = (f) => JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(__dirname, '..', 'golden', f))).toString());
const gold = load('ref_vectors.json.gz');
const { bytesToHex, stringToBytes } = bls.utils;

async function outcome(f) { try { return { v: await f() }; } catch (e) { return { e: e.message }; } }
const reference = (s) => bls.verify(s.signature, s.message, bls.aggregatePublicKeys(s.publicKeys));

(async () => {
  const R = bls.CURVE.r, POOL = 4096, N = 2000, K = 64;
  const sks = [];
  for (let i = 0; i < POOL; i++) sks.push(((BigInt(i) + 1n) * 0x9e3779b97f4a7c15f39cc0605cedc835n + 12345n) % R);
  const pks = bls.getPublicKeys(sks);
  const idx = [], msgs = [], aggSks = [];
  for (let j = 0; j < N; j++) {
    const s = [];
    let sum = 0n;
    for (let k = 0; k < K; k++) { const i = (j * K + 37 * k) % POOL; s.push(i); sum += sks[i]; }
    idx.push(s); msgs.push(stringToBytes('aggregate set ' + j)); aggSks.push(sum % R);
  }
  const sigs = await bls.signBatch(msgs, aggSks);
  // even sets as Uint8Array, odd sets as hex strings
  const sets = idx.map((s, j) => (j % 2 === 0 ? { signature: sigs[j], message: msgs[j], publicKeys: s.map((i) => pks[i]) }
    : { signature: bytesToHex(sigs[j]), message: bytesToHex(msgs[j]), publicKeys: s.map((i) => bytesToHex(pks[i])) }));
  assert.strictEqual(await reference(sets[0]), true);
  assert.strictEqual(await reference(sets[N - 1]), true);
  assert.strictEqual(await bls.verifyMultipleAggregateSignatures(sets), true);
  // one forged set
  const forged = sets.slice();
  forged[1234] = { ...sets[1234], message: stringToBytes('not what the keys signed') };
  assert.strictEqual(await reference(forged[1234]), false);
  assert.strictEqual(await bls.verifyMultipleAggregateSignatures(forged), false);
  // a key outside the subgroup: aggregatePublicKeys throws, and so does the batch, with the same message (the forged set behind it changes nothing)
  const g1sub = gold.codec.g1.find((v) => /subgroup/.test(v.result)).hex;
  const bad = forged.slice();
  bad[100] = { ...sets[100], publicKeys: sets[100].publicKeys.map((k, i) => (i === 5 ? g1sub : k)) };
  const want = await outcome(() => reference(bad[100]));
  assert.ok(want.e, 'aggregatePublicKeys should throw');
  assert.strictEqual((await outcome(() => bls.verifyMultipleAggregateSignatures(bad))).e, want.e);
  // {pk, -pk}: the aggregate is the zero point, verify throws
  const pk0 = bls.PointG1.fromHex(pks[0]);
  const zero = sets.slice(0, 8);
  zero[3] = { ...sets[3], publicKeys: [pks[0], pk0.negate().toRawBytes(true)] };
  const wantZero = await outcome(() => reference(zero[3]));
  assert.ok(wantZero.e, 'verify should throw on a zero aggregate');
  assert.strictEqual((await outcome(() => bls.verifyMultipleAggregateSignatures(zero))).e, wantZero.e);
  // point objects take verify(..., aggregatePublicKeys(...)) itself
  const pts = sets.slice(0, 12).map((s, j) => (j % 3 === 0 ? { ...s, publicKeys: s.publicKeys.map((k) => bls.PointG1.fromHex(k)) }
    : j % 3 === 1 ? { ...s, signature: bls.PointG2.fromSignature(s.signature) } : s));
  assert.strictEqual(await bls.verifyMultipleAggregateSignatures(pts), true);
  pts[6] = { ...pts[6], message: stringToBytes('changed') };
  assert.strictEqual(await reference(pts[6]), false);
  assert.strictEqual(await bls.verifyMultipleAggregateSignatures(pts), false);
  console.log('JS verifyMultipleAggregateSignatures ok');
})().catch((e) => { console.error(e); process.exit(1); });
