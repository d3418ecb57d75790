// GPU test of the facade's PointG1.verifyCellKzgProofBatch and its *Async twin (noble-bls12-381_amd/js/index.js).  The cases come from tests/test_js_kzg_verify_cells.py
// (argv[2]: a JSON file): five cells of two blobs of 32 elements, four elements per cell, with Python's and the oracle's proofs and [tau^4]G2.  Bytes and hex in.
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const c = JSON.parse(fs.readFileSync(process.argv[2]).toString());
const { PointG1 } = bls;
const { hexToBytes } = bls.utils;

(async () => {
  const setup = new PointG1.KzgMonomialSetup(c.monomial);
  const seed = { seed: hexToBytes(c.seed) };
  const call = (cells, opts, tau) => PointG1.verifyCellKzgProofBatch(setup, 2, c.commitments, c.commitment_index, c.cell_index, cells, c.proofs, tau || c.tau_c, opts);
  // a valid call: hex in, synchronous; bytes in, on a worker thread, the seed from the OS; the combined check alone
  let r = call(c.cells, seed);
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), [0, 0, 0, 0, 0]);
  r = await PointG1.verifyCellKzgProofBatchAsync(setup, 2, c.commitments.map(hexToBytes), c.commitment_index, c.cell_index, c.cells.map(hexToBytes), c.proofs.map(hexToBytes), hexToBytes(c.tau_c));
  assert.strictEqual(r.ok, true); assert.deepStrictEqual(Array.from(r.status), [0, 0, 0, 0, 0]);
  r = call(c.cells, { perItem: false });
  assert.strictEqual(r.ok, true); assert.strictEqual(r.status, null);
  // one element of one cell changed
  const cells = c.cells.slice(); cells[2] = c.tampered;
  r = call(cells, seed);
  assert.strictEqual(r.ok, false); assert.deepStrictEqual(Array.from(r.status), [0, 0, 9, 0, 0]);
  r = await PointG1.verifyCellKzgProofBatchAsync(setup, 2, c.commitments, c.commitment_index, c.cell_index, cells, c.proofs, c.tau_c, { perItem: false });
  assert.strictEqual(r.ok, false); assert.strictEqual(r.status, null);
  // [tau]G2 where [tau^4]G2 belongs; the zero point in its place; ragged arguments
  r = call(c.cells, seed, c.tau);
  assert.strictEqual(r.ok, false); assert.deepStrictEqual(Array.from(r.status), [9, 9, 9, 9, 9]);
  assert.throws(() => call(c.cells, seed, 'c0' + '00'.repeat(95)), /Invalid \[tau\]G2/);
  assert.throws(() => PointG1.verifyCellKzgProofBatch(setup, 2, c.commitments, [0, 1, 0, 1, 2], c.cell_index, c.cells, c.proofs, c.tau_c), /commitment index/);
  assert.throws(() => PointG1.verifyCellKzgProofBatch(setup, 2, c.commitments, c.commitment_index, [0, 15, 7, 1, 16], c.cells, c.proofs, c.tau_c), /cell index/);
  assert.throws(() => PointG1.verifyCellKzgProofBatch(setup, 7, c.commitments, c.commitment_index, c.cell_index, c.cells, c.proofs, c.tau_c), /log2cell/);
  assert.throws(() => call([c.cells[0].slice(2)].concat(c.cells.slice(1))), /cell/);
  setup.close();
  assert.throws(() => call(c.cells, seed), /open KzgMonomialSetup/);
  console.log('JS KZG verify cells ok');
})().catch((e) => { console.error(e); process.exit(1); });
