// Golden-vector generator, the scalar field and threshold recombination (our tooling): the reference's Fr class (math.ts:295-386) on edge and random operands, and a few
// t-of-n threshold cases driven through the reference -- a polynomial over Fr, shares sign(m, f(x_k)) and getPublicKey(f(x_k)), Lagrange coefficients computed by Fr, the
// combination by PointG2 / PointG1 multiply and add; the generator asserts that it equals sign(m, f(0)) / getPublicKey(f(0)).  Its own deterministic stream: the other fixture
// files stay byte-identical.  Runs the REAL reference (type-stripped copy under /tmp, tools/strip_ts.py).
// Driver: tools/gen_golden.py -> tests/golden/ref_fr.json.gz        node tools/gen_golden_fr.mjs /tmp/nbls_ref
import { createHash } from 'crypto';
import { pathToFileURL } from 'url';
import path from 'path';

const refDir = process.argv[2] || '/tmp/nbls_ref';

async function main() {
  const bls = await import(pathToFileURL(path.join(refDir, 'index.mjs')).href);
  const { Fr, PointG1, PointG2, CURVE } = bls;
  const r = CURVE.r;
  const hex = (u8) => Buffer.from(u8).toString('hex');
  const h32 = (v) => v.toString(16).padStart(64, '0');
  let ctr = 0;
  const rnd = (tag, bytes) => {
    let out = Buffer.alloc(0);
    while (out.length < bytes) {
      const c = Buffer.alloc(4); c.writeUInt32BE(ctr++);
      out = Buffer.concat([out, createHash('sha256').update('nbls-golden-fr').update(tag).update(c).digest()]);
    }
    return out.slice(0, bytes);
  };
  const r256 = (tag) => BigInt('0x' + rnd(tag, 32).toString('hex'));
  const attempt = (f) => { try { return h32(f().value); } catch (e) { return null; } };   // null: the reference throws (invert of 0)

  // ---- Fr: every operation on every pair of operands (any 256-bit value; the constructor reduces)
  const M = (1n << 256n) - 1n;
  const operands = [0n, 1n, 2n, r - 1n, r, r + 1n, 2n * r, 2n * r + 1n, M, M - 1n, (r - 1n) / 2n, 1n << 255n];
  for (let i = 0; i < 12; i++) operands.push(r256('op'));
  const exps = [0n, 1n, 2n, r - 2n, r - 1n, r, M, r256('e'), r256('e')];
  const ops = [];
  for (let i = 0; i < operands.length; i++) {
    const a = operands[i], b = operands[(i * 7 + 3) % operands.length], b2 = operands[(i * 5 + 1) % operands.length], e = exps[i % exps.length];
    for (const bb of [b, b2]) {
      const A = new Fr(a), B = new Fr(bb);
      ops.push({
        a: h32(a), b: h32(bb), e: h32(e),
        add: h32(A.add(B).value), sub: h32(A.subtract(B).value), neg: h32(A.negate().value), mul: h32(A.multiply(B).value), sqr: h32(A.square().value),
        inv: attempt(() => A.invert()), div: attempt(() => A.div(B)), pow: h32(A.pow(e).value),
      });
    }
  }

  // ---- threshold cases
  const lagrange = (ids) => ids.map((xk, k) => {
    let num = Fr.ONE, den = Fr.ONE;
    ids.forEach((xj, j) => { if (j !== k) { num = num.multiply(new Fr(xj)); den = den.multiply(new Fr(xj).subtract(new Fr(xk))); } });
    return num.div(den);
  });
  const cases = [];
  // [t, identifiers]: 1..n, a subset out of order, random 256-bit identifiers (some >= r)
  const shapes = [[1, [1n]], [2, [1n, 2n]], [2, [3n, 1n]], [3, [5n, 2n, 4n]], [3, [r256('id'), r256('id'), r + 7n]], [5, [1n, 2n, 3n, 4n, 5n]], [7, [9n, 8n, 1n, 3n, 4n, 6n, 10n]]];
  for (const [t, ids] of shapes) {
    const coef = [];
    for (let i = 0; i < t; i++) coef.push(new Fr(r256('poly')));
    const f = (x) => coef.reduceRight((acc, c) => acc.multiply(new Fr(x)).add(c), Fr.ZERO);
    const msg = rnd('msg', 32);
    const lam = lagrange(ids);
    const keys = ids.map((x) => f(x).value);
    const sigs = [], pks = [];
    for (const k of keys) { sigs.push(await bls.sign(msg, k)); pks.push(bls.getPublicKey(k)); }
    let S = PointG2.ZERO, K = PointG1.ZERO;
    sigs.forEach((s, k) => { S = S.add(PointG2.fromSignature(s).multiply(lam[k].value)); });
    pks.forEach((p, k) => { K = K.add(PointG1.fromHex(p).multiply(lam[k].value)); });
    const sig0 = await bls.sign(msg, coef[0].value), pk0 = bls.getPublicKey(coef[0].value);
    if (hex(S.toSignature()) !== hex(sig0) || K.toHex(true) !== hex(pk0)) throw new Error('recombination does not give sign(m, f(0)) / getPublicKey(f(0))');
    if (!(await bls.verify(sig0, msg, pk0))) throw new Error('group signature does not verify');
    cases.push({ t, msg: hex(msg), ids: ids.map(h32), lambda: lam.map((l) => h32(l.value)), sig_shares: sigs.map(hex), pk_shares: pks.map(hex), sig: hex(sig0), pk: hex(pk0) });
  }
  console.log(JSON.stringify({ r: h32(r), fr_ops: ops, threshold: cases }));
}
main().catch((e) => { console.error(e); process.exit(1); });
