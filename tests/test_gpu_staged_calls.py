"""The host-buffer pipelines that stage their inputs through one page-locked block (csrc/staging.h), where no other test goes (-m gpu): nbls_sign_batch and nbls_verify_batch
called on the C ABI with message offsets that do not start at zero and with tags of 255, 256 and 300 bytes; and the eight staged entry points interleaved on ONE context in
sizes 300, then 1, then 17, so that the staged block and the read-back block grow, then are reused while much larger than the call with another call's bytes still in them.
Everything is compared byte for byte: with the oracle, and with the same call on a context that has made no other call."""
import ctypes as C
import importlib
import random
import pytest

pytestmark = pytest.mark.gpu
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
NOT_VERIFIED = 9


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('noble-bls12-381_amd')


@pytest.fixture(scope='module')
def eng(pkg):
    return pkg.Engine(0)


def b32(v):
    return v.to_bytes(32, 'big')


def poly_at(coef, x):
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % R
    return acc


def py_lagrange(ids):
    x = [v % R for v in ids]
    out = []
    for k, xk in enumerate(x):
        num = den = 1
        for j, xj in enumerate(x):
            if j != k:
                num = num * xj % R
                den = den * (xj - xk) % R
        out.append(num * pow(den, -1, R) % R)
    return out


# ---- sign / verifyBatch on the C ABI: a first offset above zero, an empty message, oversize tags

JUNK = b'\xee' * 5
MSGS = [b'first message', b'', bytes(range(200))]


def packed(msgs):
    offs = [len(JUNK)]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    return JUNK + b''.join(msgs), (C.c_uint32 * len(offs))(*offs)


@pytest.mark.parametrize('dst_len', [255, 256, 300])
def test_sign_and_verify_batch_offsets_from_five_and_long_tags(eng, oracle, dst_len):
    rnd = random.Random(dst_len)
    dst = bytes(rnd.randrange(1, 256) for _ in range(dst_len))
    keys = [b32(rnd.randrange(1, R)) for _ in MSGS]
    want = [oracle.sign(m, k, dst) for m, k in zip(MSGS, keys)]
    assert all(st == 0 for st, _ in want)
    blob, offs = packed(MSGS)
    out, st = C.create_string_buffer(3 * 192), C.create_string_buffer(3)
    assert eng.lib.nbls_sign_batch(eng.h, 3, blob, offs, dst, len(dst), b''.join(keys), out, st) == 0
    assert st.raw == bytes(3)
    sigs = eng.compress_batch(out.raw, g2=True)
    assert [sigs[96 * i:96 * i + 96] for i in range(3)] == [s for _, s in want]
    pks = [oracle.get_public_key(k) for k in keys]
    agg = oracle.aggregate_signatures([s for _, s in want])
    agg = agg[1] if isinstance(agg, tuple) else agg
    for n, sig, msgs, keys_n in ((3, agg, MSGS, pks), (1, want[2][1], MSGS[2:], pks[2:])):
        blob, offs = packed(msgs)
        ok = C.c_int(-1)
        assert eng.lib.nbls_verify_batch(eng.h, n, sig, blob, offs, b''.join(keys_n), dst, len(dst), C.byref(ok)) == 0 and ok.value == 1, n
        assert oracle.verify_batch(sig, msgs, keys_n, dst) == 1
        flipped = bytearray(blob)
        flipped[-7] ^= 1      # a byte of the 200-byte message, the last one of both calls
        ok = C.c_int(-1)
        assert eng.lib.nbls_verify_batch(eng.h, n, sig, bytes(flipped), offs, b''.join(keys_n), dst, len(dst), C.byref(ok)) == 0 and ok.value == 0, n
        # the junk in front of the first offset is not part of any message
        other = b'\x11' * 5 + blob[5:]
        ok = C.c_int(-1)
        assert eng.lib.nbls_verify_batch(eng.h, n, sig, other, offs, b''.join(keys_n), dst, len(dst), C.byref(ok)) == 0 and ok.value == 1, n


# ---- the eight staged entry points on one context: 300, then 1, then 17 items or groups each

class Inputs:
    """what the eight calls take for k items / groups, made on the preparing context, and what Python integers say about them"""

    def __init__(self, eng, k):
        rnd = random.Random(7000 + k)
        self.k = k
        # sign, verify_multiple, verifyBatch: k messages (the first one empty) under k keys
        self.msgs = [bytes(rnd.randrange(256) for _ in range((i * 7) % 50)) for i in range(k)]
        self.keys = [b32(rnd.randrange(1, R)) for _ in range(k)]
        self.pks = eng.get_public_keys(self.keys)
        aff, _ = eng.sign_batch_affine(self.msgs, self.keys)
        c = eng.compress_batch(aff, g2=True)
        self.sigs = [c[96 * i:96 * i + 96] for i in range(k)]
        self.agg = eng.compress_batch(eng.point_sum(aff, g2=True)[0], g2=True)
        self.vm_sigs = list(self.sigs)
        if k > 1:
            self.vm_sigs[0] = self.sigs[1]      # set 0 does not verify: the per-set pass reads back through the same block as the combined result
        self.seed = bytes(rnd.randrange(256) for _ in range(32))
        # Fr
        self.a = [rnd.getrandbits(256) for _ in range(k)]
        self.b = [rnd.getrandbits(256) for _ in range(k)]
        # Lagrange, recombination (G2): k groups of three shares of a polynomial of degree two
        self.ids = [[rnd.getrandbits(256) for _ in range(3)] for _ in range(k)]
        self.coef = [[rnd.randrange(1, R) for _ in range(3)] for _ in range(k)]
        self.gmsgs = [b'group %d of %d' % (g, k) for g in range(k)]
        share_keys = [b32(poly_at(cf, x % R)) for cf, ids in zip(self.coef, self.ids) for x in ids]
        shares = eng.sign_batch([m for m in self.gmsgs for _ in range(3)], share_keys)
        self.share_groups = [(ids, shares[3 * g:3 * g + 3]) for g, ids in enumerate(self.ids)]
        # commitment polynomials (G1): the same polynomials, two identifiers each
        commits = eng.get_public_keys([b32(a) for cf in self.coef for a in cf])
        self.eval_ids = [[rnd.getrandbits(256) for _ in range(2)] for _ in range(k)]
        self.poly_groups = [(commits[3 * g:3 * g + 3], ids) for g, ids in enumerate(self.eval_ids)]
        # batched MSM (G1): k groups of four multiples of the generator
        self.mults = [[rnd.randrange(1, R) for _ in range(4)] for _ in range(k)]
        pts, _ = eng.point_mul_batch([b32(a) for g in self.mults for a in g])
        self.msm_pts = [pts[384 * g:384 * g + 384] for g in range(k)]
        self.msm_scalars = [[rnd.getrandbits(256) for _ in range(4)] for _ in range(k)]

    def calls(self):
        return [
            ('fr_op', lambda e: e.fr_op('mul', self.a, self.b)),
            ('sign', lambda e: e.sign_batch_affine(self.msgs, self.keys)),
            ('lagrange', lambda e: e.lagrange_at_zero(self.ids)),
            ('verify_multiple', lambda e: e.verify_multiple(self.vm_sigs, self.msgs, self.pks, seed=self.seed)),
            ('combine', lambda e: e.combine_shares(self.share_groups)),
            ('msm_batch', lambda e: e.msm_batch(self.msm_pts, [[b32(s) for s in g] for g in self.msm_scalars])),
            ('verify_batch', lambda e: e.verify_batch(self.agg, self.msgs, self.pks)),
            ('poly', lambda e: e.poly_eval(self.poly_groups)),
        ]


def test_eight_staged_calls_interleaved_on_one_context(pkg, eng, oracle):
    shared = pkg.Engine(0)
    for k in (300, 1, 17):
        inp = Inputs(eng, k)
        got = {}
        for name, call in inp.calls():
            got[name] = call(shared)
            fresh = pkg.Engine(0)
            want = call(fresh)
            fresh.close()
            assert got[name] == want, (k, name)
        # what has to come out whatever the size
        assert got['verify_batch'] is True
        assert got['verify_multiple'] == (k == 1, bytes([NOT_VERIFIED if i == 0 and k > 1 else 0 for i in range(k)]))
        if k != 17:
            continue
        assert got['fr_op'] == ([b32(x * y % R) for x, y in zip(inp.a, inp.b)], [0] * k)
        assert got['lagrange'] == ([[b32(v) for v in py_lagrange(ids)] for ids in inp.ids], [0] * k)
        sig = shared.compress_batch(got['sign'][0], g2=True)
        assert got['sign'][1] == bytes(k) and [sig[96 * i:96 * i + 96] for i in range(k)] == [oracle.sign(m, sk)[1] for m, sk in zip(inp.msgs, inp.keys)]
        assert got['combine'] == ([oracle.sign(m, b32(cf[0]))[1] for m, cf in zip(inp.gmsgs, inp.coef)], [0] * k)
        assert got['poly'] == ([[oracle.get_public_key(b32(poly_at(cf, x % R))) for x in ids] for cf, ids in zip(inp.coef, inp.eval_ids)], [[0, 0]] * k)
        gen = oracle.g1_generator()
        sums = [sum(a * s for a, s in zip(m, sc)) % R for m, sc in zip(inp.mults, inp.msm_scalars)]
        assert got['msm_batch'] == ([oracle.g1_mul(gen, v)[1] for v in sums], [0] * k)
        assert [oracle.verify(s, m, p) for s, m, p in zip(inp.vm_sigs, inp.msgs, inp.pks)] == [0] + [1] * (k - 1)
        assert oracle.verify_batch(inp.agg, inp.msgs, inp.pks) == 1
    shared.close()
