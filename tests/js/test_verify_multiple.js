// GPU test of the facade's verifyMultipleSignatures (noble-bls12-381_amd/js/index.js): it agrees with the facade's own verify on valid, invalid and throwing sets,
// and 131,072 sets (the reference's sign vectors repeated) resolve without RangeError.
'use strict';
const fs = require('fs'), zlib = require('zlib'), path = require('path'), assert = require('assert');
const bls = require(path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js', 'index.js'));
const load = (f) => JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(__dirname, '..', 'golden', f))).toString());
const gold = load('ref_vectors.json.gz'), td = load('ref_testdata.json.gz');

async function verifyEach(sets) {
  let all = true;
  for (const s of sets) if (!(await bls.verify(s.signature, s.message, s.publicKey))) all = false;
  return all;
}
async function outcome(f) { try { return { v: await f() }; } catch (e) { return { e: e.message }; } }

(async () => {
  const vs = td.sign_vectors.slice(0, 24);
  const pks = bls.getPublicKeys ? await bls.getPublicKeys(vs.map((v) => v[0])) : vs.map((v) => bls.getPublicKey(v[0]));
  const sets = vs.map((v, i) => ({ publicKey: pks[i], message: v[1], signature: v[2] }));
  assert.strictEqual(await bls.verifyMultipleSignatures(sets), true);
  // point objects take verify's own path
  const mixed = sets.map((s, i) => (i % 5 === 1 ? { ...s, publicKey: bls.PointG1.fromHex(s.publicKey) } : i % 5 === 2 ? { ...s, signature: bls.PointG2.fromSignature(s.signature) } : s));
  assert.strictEqual(await bls.verifyMultipleSignatures(mixed), true);
  // invalid sets: a wrong message, swapped signatures
  const bad = sets.map((s) => ({ ...s }));
  bad[3].message = bad[4].message; [bad[7].signature, bad[8].signature] = [bad[8].signature, bad[7].signature];
  assert.strictEqual(await verifyEach(bad), false);
  assert.strictEqual(await bls.verifyMultipleSignatures(bad), false);
  // throwing sets: the first one in index order throws verify's message
  const g1sub = gold.codec.g1.find((v) => /subgroup/.test(v.result)).hex, g2sub = gold.codec.g2.find((v) => /subgroup/.test(v.result)).hex;
  for (const [k, field, val] of [[5, 'publicKey', g1sub], [2, 'signature', g2sub], [6, 'publicKey', 'c0' + '00'.repeat(47)], [9, 'signature', 'c0' + '00'.repeat(95)]]) {
    const t = sets.map((s) => ({ ...s }));
    t[k][field] = val;
    t[k + 3].message = 'ff';                                                 // an invalid set behind it does not change what is thrown
    const want = await outcome(() => bls.verify(t[k].signature, t[k].message, t[k].publicKey));
    assert.ok(want.e, 'verify should throw for ' + field);
    const got = await outcome(() => bls.verifyMultipleSignatures(t));
    assert.strictEqual(got.e, want.e);
  }
  // 131,072 sets: packed into preallocated buffers, no spread
  const all = td.sign_vectors.map((v) => v);
  const allPks = bls.getPublicKeys ? await bls.getPublicKeys(all.map((v) => v[0])) : all.map((v) => bls.getPublicKey(v[0]));
  const big = [];
  for (let i = 0; big.length < 131072; i++) { const k = i % all.length; big.push({ publicKey: allPks[k], message: all[k][1], signature: all[k][2] }); }
  assert.strictEqual(await bls.verifyMultipleSignatures(big), true);
  big[131071] = { ...big[131071], message: 'abcd' };
  assert.strictEqual(await bls.verifyMultipleSignatures(big), false);
  console.log('JS verifyMultipleSignatures ok');
})().catch((e) => { console.error(e); process.exit(1); });
