// Golden-vector generator, fourth file (our tooling): the reference's hash-to-curve BEHIND expand_message_xmd on chosen uniform bytes (tests/h2c_cases.py: the edges of the
// 64-byte -> Fp reduction, exceptional SWU denominators, the a1 = 0 family of the norm-method square root, seeded ordinary elements, the degenerate items u0 = +-u1).
// For every case u = os2ip(64 bytes) mod p per element (hash_to_field's tail, index.ts:256-263), then exactly the calls of PointG1 / PointG2.hashToCurve and encodeToCurve
// (index.ts:331-350, 481-497): map_to_curve_simple_swu_*, PointG*.add(...).toAffine(), isogenyMapG*, clearCofactor.  A throw is recorded by its message.
// Runs the REAL reference (type-stripped copy under /tmp, tools/strip_ts.py).  Driver: tools/gen_golden.py (which writes the case list it reads) -> tests/golden/ref_h2c_map.json.gz
//        node tools/gen_golden4.mjs /tmp/nbls_ref /tmp/nbls_ref/h2c_cases.json
import { readFileSync } from 'fs';
import { pathToFileURL } from 'url';
import path from 'path';

const refDir = process.argv[2] || '/tmp/nbls_ref';
const casesPath = process.argv[3] || path.join(refDir, 'h2c_cases.json');

async function main() {
  const bls = await import(pathToFileURL(path.join(refDir, 'index.mjs')).href);
  const math = await import(pathToFileURL(path.join(refDir, 'math.mjs')).href);
  const { PointG1, PointG2, Fp, Fp2, CURVE } = bls;
  const { map_to_curve_simple_swu_9mod16, isogenyMapG2, map_to_curve_simple_swu_3mod4, isogenyMapG1 } = math;
  const b48 = (v) => v.toString(16).padStart(96, '0');
  const f2hex = (a) => b48(a.c0.value) + b48(a.c1.value);
  const g1aff = (P) => { const [x, y] = P.toAffine(); return b48(x.value) + b48(y.value); };
  const g2aff = (Q) => { const [x, y] = Q.toAffine(); return f2hex(x) + f2hex(y); };
  const cases = JSON.parse(readFileSync(casesPath, 'utf8'));
  const out = [];
  for (const c of cases) {
    const u = [];
    for (let o = 0; o < c.uniform.length; o += 128) u.push(BigInt('0x' + c.uniform.slice(o, o + 128)) % CURVE.P);
    const rec = { name: c.name, kind: c.kind, uniform: c.uniform, degenerate: c.degenerate, u: u.map(b48), result: 'ok', aff: null };
    try {
      if (c.kind === 0 || c.kind === 1) {
        rec.swu = [];
        const pts = [];
        for (let k = 0; k < u.length; k += 2) {
          const [x, y] = map_to_curve_simple_swu_9mod16(Fp2.fromBigTuple([u[k], u[k + 1]]));
          rec.swu.push(f2hex(x) + f2hex(y));
          pts.push([x, y]);
        }
        let x2 = pts[0][0], y2 = pts[0][1];
        if (c.kind === 0) [x2, y2] = new PointG2(pts[0][0], pts[0][1]).add(new PointG2(pts[1][0], pts[1][1])).toAffine();
        const [x3, y3] = isogenyMapG2(x2, y2);
        rec.aff = g2aff(new PointG2(x3, y3).clearCofactor());
      } else {
        const pts = u.map((v) => map_to_curve_simple_swu_3mod4(new Fp(v)));
        let x2 = pts[0][0], y2 = pts[0][1];
        if (c.kind === 2) [x2, y2] = new PointG1(pts[0][0], pts[0][1]).add(new PointG1(pts[1][0], pts[1][1])).toAffine();
        const [x3, y3] = isogenyMapG1(x2, y2);
        rec.aff = g1aff(new PointG1(x3, y3).clearCofactor());
      }
    } catch (e) { rec.result = e.message; rec.aff = null; }
    out.push(rec);
  }
  process.stdout.write(JSON.stringify({ cases: out }));
}
main().catch((e) => { console.error(e); process.exit(1); });
