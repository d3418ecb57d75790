// GPU test of the facade's KZG calls (noble-bls12-381_amd/js/index.js: PointG1.verifyKzgProofBatch / verifyBlobKzgProofBatch and their *Async twins).  The cases come from
// tests/test_js_kzg.py (argv[2]: a JSON file): nine valid tuples from a test-only setup (kzg_cases.py), the tampered item, blobs with their commitments and proofs, and [tau]G2.
// Bytes, hex and points in; field elements as hex, bigint or 32 bytes.
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const c = JSON.parse(fs.readFileSync(process.argv[2]).toString());
const { PointG1, PointG2 } = bls;
const { hexToBytes } = bls.utils;

(async () => {
  const n = c.commitments.length, seed = hexToBytes(c.seed), zeros = Array(n).fill(0);
  const big = (h) => BigInt('0x' + h);
  // the nine valid tuples: hex in, synchronous; bytes and bigint in, on a worker thread; points in; the weights from the OS
  let r = PointG1.verifyKzgProofBatch(c.commitments, c.zs, c.ys, c.proofs, c.tau, { seed });
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), zeros);
  r = await PointG1.verifyKzgProofBatchAsync(c.commitments.map(hexToBytes), c.zs.map(big), c.ys.map(hexToBytes), c.proofs.map(hexToBytes), hexToBytes(c.tau), { seed });
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), zeros);
  r = await PointG1.verifyKzgProofBatchAsync(c.commitments.map((h) => PointG1.fromHex(h)), c.zs, c.ys, c.proofs.map((h) => PointG1.fromHex(h)), PointG2.fromSignature(c.tau));
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), zeros);
  r = PointG1.verifyKzgProofBatch(c.commitments, c.zs, c.ys, c.proofs, c.tau, { perItem: false });
  assert.strictEqual(r.ok, true); assert.strictEqual(r.status, null);
  // the tampered case: one y off by one
  const want = zeros.slice(); want[c.bad] = 9;
  r = PointG1.verifyKzgProofBatch(c.commitments, c.zs, c.ys_bad, c.proofs, c.tau, { seed });
  assert.strictEqual(r.ok, false); assert.deepStrictEqual(Array.from(r.status), want);
  r = await PointG1.verifyKzgProofBatchAsync(c.commitments, c.zs, c.ys_bad, c.proofs, c.tau, { seed, perItem: false });
  assert.strictEqual(r.ok, false); assert.strictEqual(r.status, null);
  // blobs
  const bz = Array(c.blobs.length).fill(0);
  r = PointG1.verifyBlobKzgProofBatch(c.blobs, c.blob_commitments, c.blob_proofs, c.tau, { seed });
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), bz);
  const blobs = c.blobs.map(hexToBytes); blobs[1][5] ^= 1;
  const bw = bz.slice(); bw[1] = 9;
  r = await PointG1.verifyBlobKzgProofBatchAsync(blobs, c.blob_commitments, c.blob_proofs, c.tau, { seed });
  assert.strictEqual(r.ok, false); assert.deepStrictEqual(Array.from(r.status), bw);
  // arguments that are refused
  assert.throws(() => PointG1.verifyKzgProofBatch([], [], [], [], c.tau), /non-empty/);
  assert.throws(() => PointG1.verifyKzgProofBatch(c.commitments, c.zs.slice(1), c.ys, c.proofs, c.tau), /as many/);
  assert.throws(() => PointG1.verifyKzgProofBatch(c.commitments, c.zs, c.ys, c.proofs, 'c0' + '00'.repeat(95), { seed }), /tau/);
  console.log('JS KZG ok');
})().catch((e) => { console.error(e); process.exit(1); });
