// GPU test of the facade's recovery calls (noble-bls12-381_amd/js/index.js: PointG1.recoverCells, PointG1.recoverCellsAndKzgProofs and their *Async twins).  The cases come from
// tests/test_js_kzg_recover.py (argv[2]: a JSON file): two blobs of 32 elements in 16 cells with Python's cells and the oracle's proofs, an index list for each, and a list that
// is one cell short.  Bytes and hex in.
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const c = JSON.parse(fs.readFileSync(process.argv[2]).toString());
const { PointG1 } = bls;
const { hexToBytes, bytesToHex } = bls.utils;

(async () => {
  const hex = (arr) => arr.map((b) => bytesToHex(b));
  const given = c.indices.map((idx, i) => idx.map((k) => c.cells[i][k]));
  // the cells: hex in, synchronous; bytes in, on a worker thread
  let r = PointG1.recoverCells(5, 2, c.indices, given);
  assert.deepStrictEqual(r.cells.map(hex), c.cells); assert.deepStrictEqual(Array.from(r.status), [0, 0]);
  r = await PointG1.recoverCellsAsync(5, 2, c.indices, given.map((g) => g.map(hexToBytes)));
  assert.deepStrictEqual(r.cells.map(hex), c.cells); assert.deepStrictEqual(Array.from(r.status), [0, 0]);
  // a refused blob between two good ones: one cell short; then a cell given twice, and a changed element with half + 1 cells
  const zero = Array(16).fill('00'.repeat(128));
  const shortGiven = c.short.map((k) => c.cells[0][k]);
  r = PointG1.recoverCells(5, 2, [c.indices[0], c.short, c.indices[1]], [given[0], shortGiven, given[1]]);
  assert.deepStrictEqual(Array.from(r.status), [0, 22, 0]); assert.deepStrictEqual(r.cells.map(hex), [c.cells[0], zero, c.cells[1]]);
  r = PointG1.recoverCells(5, 2, [c.short.concat([c.short[0]])], [shortGiven.concat([shortGiven[0]])]);
  assert.deepStrictEqual(Array.from(r.status), [22]);
  const changed = given[1].slice(); changed[0] = c.changed;
  r = PointG1.recoverCells(5, 2, [c.indices[1]], [changed]);
  assert.deepStrictEqual(Array.from(r.status), [23]); assert.deepStrictEqual(r.cells.map(hex), [zero]);
  // the facade's argument handling
  assert.throws(() => PointG1.recoverCells(5, 6, c.indices, given), /log2cell/);
  assert.throws(() => PointG1.recoverCells(13, 6, c.indices, given), /log2n/);
  assert.throws(() => PointG1.recoverCells(5, 2, [], []), /non-empty/);
  assert.throws(() => PointG1.recoverCells(5, 2, c.indices, [given[0]]), /as many lists/);
  assert.throws(() => PointG1.recoverCells(5, 2, [c.indices[0].slice(1), c.indices[1]], given), /as many cell indices as cells/);
  assert.throws(() => PointG1.recoverCells(5, 2, [c.indices[0].map((k) => -k - 1), c.indices[1]], given), /Invalid cell index/);
  assert.throws(() => PointG1.recoverCells(5, 2, c.indices, [given[0].map((h) => h.slice(2)), given[1]]), /cell/);
  // cells and proofs against the monomial basis
  const setup = new PointG1.KzgMonomialSetup(c.monomial);
  r = PointG1.recoverCellsAndKzgProofs(setup, 2, c.indices, given);
  assert.deepStrictEqual(r.cells.map(hex), c.cells); assert.deepStrictEqual(r.proofs.map(hex), c.proofs); assert.deepStrictEqual(Array.from(r.status), [0, 0]);
  r = await PointG1.recoverCellsAndKzgProofsAsync(setup, 2, [c.indices[0], c.short, c.indices[1]], [given[0], shortGiven, given[1]].map((g) => g.map(hexToBytes)));
  assert.deepStrictEqual(Array.from(r.status), [0, 22, 0]);
  assert.deepStrictEqual(r.cells.map(hex), [c.cells[0], zero, c.cells[1]]);
  assert.deepStrictEqual(r.proofs.map(hex), [c.proofs[0], Array(16).fill('00'.repeat(48)), c.proofs[1]]);
  const same = PointG1.computeCellsAndKzgProofs(setup, 2, c.blobs);
  assert.deepStrictEqual(same.cells.map(hex), c.cells); assert.deepStrictEqual(same.proofs.map(hex), c.proofs);
  setup.close();
  assert.throws(() => PointG1.recoverCellsAndKzgProofs(setup, 2, c.indices, given), /open KzgMonomialSetup/);
  console.log('JS KZG recover ok');
})().catch((e) => { console.error(e); process.exit(1); });
