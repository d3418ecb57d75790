// GPU test of the facade's Groth16 calls (noble-bls12-381_amd/js/index.js: PointG1.Groth16Vk, PointG1.verifyGroth16Batch and its Async twin).  The cases come from
// tests/test_js_groth16.py (argv[2]: a JSON file): a test-only key (groth16_cases.py), nine valid proofs with their inputs, and the inputs with one value off by one.
// Hex, bytes, points and packed arrays in; field elements as hex, bigint or 32 bytes.
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const c = JSON.parse(fs.readFileSync(process.argv[2]).toString());
const { PointG1, PointG2 } = bls;
const { hexToBytes } = bls.utils;

(async () => {
  const n = c.proofs.length, m = c.ic.length - 1, seed = hexToBytes(c.seed), zeros = Array(n).fill(0);
  const big = (h) => BigInt('0x' + h);
  const pack = (rows, w) => { const out = new Uint8Array(rows.length * w); rows.forEach((r, i) => out.set(r, i * w)); return out; };
  const vk = new PointG1.Groth16Vk({ alpha: c.alpha, beta: c.beta, gamma: c.gamma, delta: c.delta, ic: c.ic });
  assert.strictEqual(vk.inputs, m);
  // the nine valid proofs: hex in, synchronous; bytes and bigint in, on a worker thread; packed arrays; a key from points and bytes; the weights from the OS
  let r = PointG1.verifyGroth16Batch(vk, c.proofs, c.inputs, { seed });
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), zeros);
  r = await PointG1.verifyGroth16BatchAsync(vk, c.proofs.map(hexToBytes), c.inputs.map((row) => row.map(big)), { seed });
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), zeros);
  const packedProofs = pack(c.proofs.map(hexToBytes), 192), packedInputs = pack(c.inputs.map((row) => pack(row.map(hexToBytes), 32)), 32 * m);
  r = await PointG1.verifyGroth16BatchAsync(vk, packedProofs, packedInputs);
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), zeros);
  const vk2 = new PointG1.Groth16Vk({ alpha: PointG1.fromHex(c.alpha), beta: PointG2.fromSignature(c.beta), gamma: hexToBytes(c.gamma), delta: c.delta, ic: c.ic.map(hexToBytes) });
  r = PointG1.verifyGroth16Batch(vk2, packedProofs, c.inputs, { perItem: false });
  assert.strictEqual(r.ok, true); assert.strictEqual(r.status, null);
  vk2.close();
  assert.throws(() => PointG1.verifyGroth16Batch(vk2, c.proofs, c.inputs), /open Groth16Vk/);
  // the tampered case: one input off by one
  const want = zeros.slice(); want[c.bad] = 9;
  r = PointG1.verifyGroth16Batch(vk, c.proofs, c.inputs_bad, { seed });
  assert.strictEqual(r.ok, false); assert.deepStrictEqual(Array.from(r.status), want);
  r = await PointG1.verifyGroth16BatchAsync(vk, packedProofs, pack(c.inputs_bad.map((row) => pack(row.map(hexToBytes), 32)), 32 * m), { seed });
  assert.strictEqual(r.ok, false); assert.deepStrictEqual(Array.from(r.status), want);
  r = await PointG1.verifyGroth16BatchAsync(vk, c.proofs, c.inputs_bad, { seed, perItem: false });
  assert.strictEqual(r.ok, false); assert.strictEqual(r.status, null);
  // a proof whose B is the zero point: status 11, the neighbours untouched
  const proofs = c.proofs.map(hexToBytes); proofs[2] = proofs[2].slice(); proofs[2].fill(0, 48, 144); proofs[2][48] = 0xc0;
  const w2 = zeros.slice(); w2[2] = 11;
  r = PointG1.verifyGroth16Batch(vk, proofs, c.inputs, { seed });
  assert.strictEqual(r.ok, false); assert.deepStrictEqual(Array.from(r.status), w2);
  // arguments that are refused
  assert.throws(() => PointG1.verifyGroth16Batch(vk, [], []), /one proof or more/);
  assert.throws(() => PointG1.verifyGroth16Batch(vk, c.proofs, c.inputs.slice(1)), /as many/);
  assert.throws(() => PointG1.verifyGroth16Batch(vk, c.proofs, c.inputs.map((row) => row.slice(1))), /per proof/);
  assert.throws(() => PointG1.verifyGroth16Batch(vk, packedProofs.subarray(1), c.inputs), /192/);
  assert.throws(() => new PointG1.Groth16Vk({ alpha: c.alpha, beta: c.beta, gamma: c.gamma, delta: c.delta, ic: c.ic.slice(0, 1) }), /Invalid key/);
  let err = null;
  try { new PointG1.Groth16Vk({ alpha: c.alpha, beta: 'c0' + '00'.repeat(95), gamma: c.gamma, delta: c.delta, ic: c.ic }); } catch (e) { err = e; }
  assert.ok(err && /Invalid key/.test(err.message) && Array.from(err.status).join() === [0, 1, 0, 0].concat(Array(m + 1).fill(0)).join());
  vk.close();
  console.log('JS Groth16 ok');
})().catch((e) => { console.error(e); process.exit(1); });
