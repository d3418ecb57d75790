// GPU test of the facade's PeerDAS calls (noble-bls12-381_amd/js/index.js: PointG1.frNtt, PointG1.computeCells, PointG1.KzgMonomialSetup, PointG1.computeCellsAndKzgProofs and their
// *Async twins).  The cases come from tests/test_js_kzg_cells.py (argv[2]: a JSON file): two polynomials of 32 elements with their shifts, three blobs of 32 elements (the second
// refused, the third of degree < c) and Python's and the oracle's coefficients, cells and proofs.  Bytes and hex in.
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const c = JSON.parse(fs.readFileSync(process.argv[2]).toString());
const { PointG1 } = bls;
const { hexToBytes, bytesToHex } = bls.utils;

(async () => {
  const hex = (arr) => arr.map((b) => bytesToHex(b));
  // the transform: hex in, synchronous, with shifts; bytes in, on a worker thread, the way back
  let r = PointG1.frNtt(5, c.values, false, c.shifts);
  assert.deepStrictEqual(hex(r.rows), c.coefficients); assert.deepStrictEqual(Array.from(r.status), [0, 0]);
  r = await PointG1.frNttAsync(5, c.coefficients.map(hexToBytes), true, c.shifts.map((h) => BigInt('0x' + h)));
  assert.deepStrictEqual(hex(r.rows), c.values); assert.deepStrictEqual(Array.from(r.status), [0, 0]);
  r = PointG1.frNtt(5, c.values, false);
  assert.deepStrictEqual(hex(r.rows), c.plain_coefficients);
  r = PointG1.frNtt(5, c.values, false, ['00'.repeat(32), c.r]);
  assert.deepStrictEqual(Array.from(r.status), [5, 21]); assert.deepStrictEqual(hex(r.rows), ['00'.repeat(1024), '00'.repeat(1024)]);
  assert.throws(() => PointG1.frNtt(5, [c.values[0].slice(2)], false), /polynomial/);
  // cells
  const status = [0, 21, 0];
  r = PointG1.computeCells(5, 2, c.blobs);
  assert.deepStrictEqual(r.cells.map(hex), c.cells); assert.deepStrictEqual(Array.from(r.status), status);
  r = await PointG1.computeCellsAsync(5, 2, c.blobs.map(hexToBytes));
  assert.deepStrictEqual(r.cells.map(hex), c.cells); assert.deepStrictEqual(Array.from(r.status), status);
  assert.throws(() => PointG1.computeCells(5, 6, c.blobs), /log2cell/);
  // cells and proofs against the monomial basis
  const setup = new PointG1.KzgMonomialSetup(c.monomial);
  assert.strictEqual(setup.log2n, 5);
  r = PointG1.computeCellsAndKzgProofs(setup, 2, c.blobs);
  assert.deepStrictEqual(r.cells.map(hex), c.cells); assert.deepStrictEqual(r.proofs.map(hex), c.proofs); assert.deepStrictEqual(Array.from(r.status), status);
  assert.deepStrictEqual(c.proofs[2], Array(16).fill('c0' + '00'.repeat(47)));
  r = await PointG1.computeCellsAndKzgProofsAsync(setup, 2, c.blobs.map(hexToBytes));
  assert.deepStrictEqual(r.cells.map(hex), c.cells); assert.deepStrictEqual(r.proofs.map(hex), c.proofs); assert.deepStrictEqual(Array.from(r.status), status);
  setup.close();
  assert.throws(() => PointG1.computeCellsAndKzgProofs(setup, 2, c.blobs), /open KzgMonomialSetup/);
  const bad = c.monomial.slice(); bad[1] = 'c0' + '00'.repeat(47);
  assert.throws(() => new PointG1.KzgMonomialSetup(bad), (e) => /Invalid setup/.test(e.message) && e.status[1] === 1);
  console.log('JS KZG cells ok');
})().catch((e) => { console.error(e); process.exit(1); });
