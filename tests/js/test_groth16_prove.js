// GPU test of the facade's Groth16 prover (noble-bls12-381_amd/js/index.js: PointG1.groth16ProvingKey, PointG1.groth16Prove).  The case comes from
// tests/test_js_groth16_prove.py (argv[2]: a JSON file): an instance with its test-only proving and verifying keys (groth16_prove_cases.py), one witness with (r, s) and the
// bytes the Python binding made of them.  Hex, bigint and packed arrays in.
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const c = JSON.parse(fs.readFileSync(process.argv[2]).toString());
const { PointG1 } = bls;
const { hexToBytes, bytesToHex } = bls.utils;

(async () => {
  const big = (h) => BigInt('0x' + h);
  const matrices = c.matrices.map((m) => m.map((row) => row.map(([col, v]) => [col, big(v)])));
  const init = { log2n: c.log2n, nVars: c.nVars, nPublic: c.nPublic, matrices, ...c.points };
  const pk = PointG1.groth16ProvingKey(init);
  assert.ok(pk instanceof PointG1.Groth16Pk);
  assert.deepStrictEqual([pk.log2n, pk.nVars, pk.nPublic], [c.log2n, c.nVars, c.nPublic]);
  // the same (z, r, s) as the Python binding: the same bytes -- field elements as hex, then as bigint, then packed
  let r = PointG1.groth16Prove(pk, [c.z], [c.rs]);
  assert.deepStrictEqual(Array.from(r.status), [0]); assert.strictEqual(bytesToHex(r.proofs[0]), c.proof);
  r = PointG1.groth16Prove(pk, [c.z.map(big)], [c.rs.map(big)]);
  assert.strictEqual(bytesToHex(r.proofs[0]), c.proof);
  const packed = new Uint8Array(c.nVars * 32); c.z.forEach((h, i) => packed.set(hexToBytes(h), 32 * i));
  r = PointG1.groth16Prove(pk, packed, [c.rs.map(hexToBytes)]);
  assert.strictEqual(bytesToHex(r.proofs[0]), c.proof);
  // the verifier accepts it; with (r, s) from the OS two proofs differ and both are accepted
  const vk = new PointG1.Groth16Vk(c.vk);
  const inputs = c.z.slice(1, c.nPublic + 1);
  assert.strictEqual(PointG1.verifyGroth16Batch(vk, r.proofs, [inputs]).ok, true);
  const two = PointG1.groth16Prove(pk, [c.z, c.z]);
  assert.deepStrictEqual(Array.from(two.status), [0, 0]);
  assert.notStrictEqual(bytesToHex(two.proofs[0]), bytesToHex(two.proofs[1]));
  assert.strictEqual(PointG1.verifyGroth16Batch(vk, two.proofs, [inputs, inputs]).ok, true);
  // a witness that violates a row, between valid neighbours
  const bad = c.z.slice(); bad[c.nVars - 1] = (big(bad[c.nVars - 1]) ^ 1n).toString(16).padStart(64, '0');
  r = PointG1.groth16Prove(pk, [c.z, bad, c.z], [c.rs, c.rs, c.rs]);
  assert.deepStrictEqual(Array.from(r.status), [0, 24, 0]);
  assert.deepStrictEqual([bytesToHex(r.proofs[0]), bytesToHex(r.proofs[1]), bytesToHex(r.proofs[2])], [c.proof, '00'.repeat(192), c.proof]);
  // arguments that are refused
  assert.throws(() => PointG1.groth16Prove(pk, []), /one witness or more/);
  assert.throws(() => PointG1.groth16Prove(pk, [c.z.slice(1)]), /field elements/);
  assert.throws(() => PointG1.groth16Prove(pk, [c.z], [c.rs, c.rs]), /per witness/);
  assert.throws(() => PointG1.groth16ProvingKey({ ...init, hQuery: init.hQuery.slice(1) }), /hQuery/);
  assert.throws(() => PointG1.groth16ProvingKey({ ...init, nPublic: 0 }), /nPublic/);
  let err = null;
  try { PointG1.groth16ProvingKey({ ...init, deltaG1: 'c0' + '00'.repeat(47) }); } catch (e) { err = e; }
  assert.ok(err && /Invalid key/.test(err.message) && err.status[3] === 1 && err.status[0] === 0);
  pk.close();
  assert.throws(() => PointG1.groth16Prove(pk, [c.z]), /open Groth16Pk/);
  vk.close();
  console.log('JS Groth16 prove ok');
})().catch((e) => { console.error(e); process.exit(1); });
