// GPU test of the facade's threshold recombination (noble-bls12-381_amd/js/index.js: PointG2.combineShares / PointG1.combineShares / combineSharesBatch) on the cases the
// reference itself made (tests/golden/ref_fr.json.gz, tools/gen_golden_fr.mjs): bytes or hex in give bytes out, points in give a point out, identifiers may be bigint, number,
// hex or 32 bytes; identifiers that are zero or repeated mod r and shares that do not decode throw Error.
'use strict';
const fs = require('fs'), zlib = require('zlib'), path = require('path'), assert = require('assert');
const JS = path.join(__dirname, '..', '..', 'noble-bls12-381_amd', 'js');
const bls = require(path.join(JS, 'index.js'));
const load = (f) => JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(__dirname, '..', 'golden', f))).toString());
const fr = load('ref_fr.json.gz'), gold = load('ref_vectors.json.gz');
const { PointG1, PointG2 } = bls;
const { bytesToHex, hexToBytes } = bls.utils;

async function message(f) { try { await f(); return null; } catch (e) { assert(e instanceof Error); return e.message; } }

(async () => {
  const R = bls.CURVE.r;
  const cases = fr.threshold;
  for (const c of cases) {
    const ids = c.ids.map((x) => BigInt('0x' + x));
    // hex in -> bytes out
    const sig = await PointG2.combineShares(c.sig_shares, ids);
    assert(sig instanceof Uint8Array && bytesToHex(sig) === c.sig);
    const pk = await PointG1.combineShares(c.pk_shares, ids);
    assert(pk instanceof Uint8Array && bytesToHex(pk) === c.pk);
    // bytes in, identifiers as hex / 32 bytes / number where they fit
    const mixed = c.ids.map((x, i) => (i % 3 === 0 ? x : i % 3 === 1 ? hexToBytes(x) : (ids[i] < 1000n ? Number(ids[i]) : ids[i])));
    assert.strictEqual(bytesToHex(await PointG2.combineShares(c.sig_shares.map(hexToBytes), mixed)), c.sig);
    // points in -> a point out
    const P = await PointG2.combineShares(c.sig_shares.map((s) => PointG2.fromSignature(s)), ids);
    assert(P instanceof PointG2 && bytesToHex(P.toSignature()) === c.sig);
    const K = await PointG1.combineShares(c.pk_shares.map((s) => PointG1.fromHex(s)), ids);
    assert(K instanceof PointG1 && K.toHex(true) === c.pk);
    // the result verifies under the group key
    assert.strictEqual(await bls.verify(sig, hexToBytes(c.msg), pk), true);
  }
  // all groups in one call, objects and pairs
  const sigs = await PointG2.combineSharesBatch(cases.map((c, i) => (i % 2 ? [c.sig_shares, c.ids] : { shares: c.sig_shares, ids: c.ids })));
  assert.deepStrictEqual(sigs.map(bytesToHex), cases.map((c) => c.sig));
  const pks = await PointG1.combineSharesBatch(cases.map((c) => ({ shares: c.pk_shares, ids: c.ids })));
  assert.deepStrictEqual(pks.map(bytesToHex), cases.map((c) => c.pk));

  // the throwing paths
  const c = cases.find((x) => x.t === 3), ids = c.ids.map((x) => BigInt('0x' + x));
  const BAD_IDS = 'Invalid share identifiers: zero or repeated modulo CURVE.r';
  assert.strictEqual(await message(() => PointG2.combineShares(c.sig_shares, [ids[0], ids[1], ids[0]])), BAD_IDS);
  assert.strictEqual(await message(() => PointG2.combineShares(c.sig_shares, [ids[0], 0n, ids[2]])), BAD_IDS);
  assert.strictEqual(await message(() => PointG2.combineShares(c.sig_shares, [5n, 7n, 5n + R])), BAD_IDS);
  assert.strictEqual(await message(() => PointG1.combineShares(c.pk_shares, [R, 1n, 2n])), BAD_IDS);
  const g2sub = gold.codec.g2.find((v) => v.result.includes('subgroup')).hex, g2root = gold.codec.g2.find((v) => v.result === 'Failed to find a square root').hex;
  const g1sub = gold.codec.g1.find((v) => v.result.includes('subgroup')).hex;
  assert.strictEqual(await message(() => PointG2.combineShares([c.sig_shares[0], g2sub, c.sig_shares[2]], ids)), 'Invalid G2 point: must be of prime-order subgroup');
  assert.strictEqual(await message(() => PointG2.combineShares([c.sig_shares[0], c.sig_shares[1], g2root], ids)), 'Failed to find a square root');
  assert.strictEqual(await message(() => PointG1.combineShares([g1sub, c.pk_shares[1], c.pk_shares[2]], ids)), 'Invalid G1 point: must be of prime-order subgroup');
  assert.strictEqual(await message(() => PointG2.combineShares(c.sig_shares, ids.slice(1))), 'Expected as many share identifiers as shares, at least one');
  assert.strictEqual(await message(() => PointG2.combineShares([], [])), 'Expected as many share identifiers as shares, at least one');
  assert.strictEqual(await message(() => PointG2.combineSharesBatch([])), 'Expected non-empty array');
  assert.strictEqual(await message(() => PointG2.combineShares(c.pk_shares, ids)), 'Invalid share: expected 96 compressed bytes');
  assert.strictEqual(await message(() => PointG2.combineShares([PointG2.fromSignature(c.sig_shares[0]), c.sig_shares[1], c.sig_shares[2]], ids)),
    'Expected the shares of a group to be all points or all compressed bytes');
  assert.strictEqual(await message(() => PointG2.combineShares(c.sig_shares, [1n, 2n, -3n])), 'Invalid share identifier: expected 0 <= id < 2^256');
  assert.strictEqual(await message(() => PointG2.combineShares(c.sig_shares, [1n, 2n, 1n << 256n])), 'Invalid share identifier: expected 0 <= id < 2^256');
  assert.strictEqual(await message(() => PointG2.combineShares(c.sig_shares, [1, 2, 2.5])), 'Invalid share identifier: expected an integer');
  // one bad group fails the batch call, the others alone succeed
  assert.strictEqual(await message(() => PointG2.combineSharesBatch([{ shares: cases[1].sig_shares, ids: cases[1].ids }, { shares: c.sig_shares, ids: [1n, 1n, 2n] }])), BAD_IDS);
  // a zero share adds nothing; shares s and [2]s with identifiers 1 and 2 combine to the zero point
  const s = PointG2.fromSignature(c.sig_shares[0]);
  const Z = await PointG2.combineShares([s, s.double()], [1n, 2n]);
  assert(Z instanceof PointG2 && Z.isZero());
  assert.strictEqual(bytesToHex(await PointG2.combineShares([s.toSignature(), s.double().toSignature()], [1, 2])), 'c' + '0'.repeat(191));
  const withZero = await PointG2.combineShares([c.sig_shares[0], 'c' + '0'.repeat(191)], [1n, 2n]);          // lambda = (2, -1): [2]s
  assert.strictEqual(bytesToHex(withZero), bytesToHex(s.double().toSignature()));
  console.log('JS threshold recombination ok: ' + cases.length + ' reference cases');
})().catch((e) => { console.error(e); process.exit(1); });
