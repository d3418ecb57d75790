// GPU test of the facade's commitment evaluation (noble-bls12-381_amd/js/index.js: PointG1.evalCommitment / PointG2.evalCommitment / evalCommitmentBatch).  The cases come from
// tests/test_js_poly.py (argv[2]: a JSON file): commitments, identifiers and the bytes the Python binding's poly_eval gave for them.  Bytes or hex in give bytes out, points in
// give points out, identifiers may be bigint, number, hex or 32 bytes; a coefficient that does not decode throws Error.
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const cases = JSON.parse(fs.readFileSync(process.argv[2]).toString());
const { PointG1, PointG2 } = bls;
const { bytesToHex, hexToBytes } = bls.utils;

async function message(f) { try { await f(); return null; } catch (e) { assert(e instanceof Error); return e.message; } }

(async () => {
  for (const [Point, list, dec, enc] of [[PointG1, cases.g1, (h) => PointG1.fromHex(h), (p) => p.toHex(true)], [PointG2, cases.g2, (h) => PointG2.fromSignature(h), (p) => bytesToHex(p.toSignature())]]) {
    for (const c of list) {
      const ids = c.ids.map((x) => BigInt('0x' + x));
      // hex in -> bytes out
      const a = await Point.evalCommitment(c.coefs, ids);
      assert(a.every((b) => b instanceof Uint8Array));
      assert.deepStrictEqual(a.map(bytesToHex), c.out);
      // bytes in, identifiers as hex / 32 bytes / number where they fit
      const mixed = c.ids.map((x, i) => (i % 3 === 0 ? x : i % 3 === 1 ? hexToBytes(x) : (ids[i] < 1000n ? Number(ids[i]) : ids[i])));
      assert.deepStrictEqual((await Point.evalCommitment(c.coefs.map(hexToBytes), mixed)).map(bytesToHex), c.out);
      // points in -> points out
      const P = await Point.evalCommitment(c.coefs.map(dec), ids);
      assert(P.every((p) => p instanceof Point));
      assert.deepStrictEqual(P.map(enc), c.out);
    }
    // all groups in one call, objects and pairs
    const all = await Point.evalCommitmentBatch(list.map((c, i) => (i % 2 ? [c.coefs, c.ids] : { coefs: c.coefs, ids: c.ids })));
    assert.deepStrictEqual(all.map((g) => g.map(bytesToHex)), list.map((c) => c.out));
  }
  // a zero of the polynomial: 0xc0 00.. as bytes, the zero point as a point
  const z = cases.zero;
  assert.deepStrictEqual((await PointG1.evalCommitment(z.coefs, z.ids)).map(bytesToHex), z.out);
  assert.strictEqual(z.out[1], 'c' + '0'.repeat(95));
  const Z = await PointG1.evalCommitment(z.coefs.map((h) => PointG1.fromHex(h)), z.ids);
  assert(Z[1] instanceof PointG1 && Z[1].isZero() && !Z[0].isZero());
  // the throwing paths
  const c1 = cases.g1[0], c2 = cases.g2[0];
  assert.strictEqual(await message(() => PointG1.evalCommitment([c1.coefs[0], cases.g1_sub, c1.coefs[2]], [1, 2])), 'Invalid G1 point: must be of prime-order subgroup');
  assert.strictEqual(await message(() => PointG2.evalCommitment([c2.coefs[0], c2.coefs[1], cases.g2_root], [1, 2])), 'Failed to find a square root');
  // one bad group fails the batch call
  assert.strictEqual(await message(() => PointG1.evalCommitmentBatch([{ coefs: c1.coefs, ids: [1] }, { coefs: [cases.g1_sub], ids: [3] }])), 'Invalid G1 point: must be of prime-order subgroup');
  assert.strictEqual(await message(() => PointG1.evalCommitment([], [1])), 'Expected at least one coefficient and one identifier');
  assert.strictEqual(await message(() => PointG1.evalCommitment(c1.coefs, [])), 'Expected at least one coefficient and one identifier');
  assert.strictEqual(await message(() => PointG1.evalCommitmentBatch([])), 'Expected non-empty array');
  assert.strictEqual(await message(() => PointG1.evalCommitment(c2.coefs, [1])), 'Invalid coefficient: expected 48 compressed bytes');
  assert.strictEqual(await message(() => PointG1.evalCommitment([PointG1.fromHex(c1.coefs[0]), c1.coefs[1]], [1])), 'Expected the coefficients of a group to be all points or all compressed bytes');
  assert.strictEqual(await message(() => PointG1.evalCommitment(c1.coefs, [1n << 256n])), 'Invalid share identifier: expected 0 <= id < 2^256');
  console.log('JS commitment evaluation ok: ' + (cases.g1.length + cases.g2.length) + ' cases');
})().catch((e) => { console.error(e); process.exit(1); });
