"""Helpers of the KZG tests (test_kzg_sim.py, test_kzg_abi.py, test_kzg_cases.py, test_gpu_kzg.py, test_gpu_kzg_adversarial.py): the scalar side in Python integers -- the roots of unity in bit-reversed order, the barycentric
formula as the issue states it, Horner's rule, the blob challenge by hashlib -- and a test-only trusted setup: with the secret TAU known, commitments and proofs are single
multiples of the generator, C = [p(tau)]G1 and pi = [(p(tau) - y) / (tau - z)]G1, taken from the oracle.  Nothing here calls the code under test."""
import hashlib

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
M256 = (1 << 256) - 1
TAU = 0x1f2e3d4c5b6a79880123456789abcdef0fedcba9876543210011223344556677 % R      # test-only: a real setup's secret is destroyed
NOT_VERIFIED, NON_CANONICAL = 9, 21
ZERO48 = b'\xc0' + bytes(47)
LANES = 256      # FR_EVAL_LANES: lane t of a workgroup owns the terms t, t + 256, ..


def b32(v):
    return v.to_bytes(32, 'big')


def bitrev(j, bits):
    return int(format(j, '0%db' % bits)[::-1], 2) if bits else 0


_roots = {}


def roots(log2_n):
    """w_j = omega^rev(j), omega = 7^((r - 1) / N)"""
    if log2_n not in _roots:
        n = 1 << log2_n
        omega = pow(7, (R - 1) // n, R)
        nat = [1] * n
        for i in range(1, n):
            nat[i] = nat[i - 1] * omega % R
        _roots[log2_n] = [nat[bitrev(j, log2_n)] for j in range(n)]
    return _roots[log2_n]


def eval_roots(f, z, log2_n):
    """p(z) for the polynomial with p(w_j) = f_j: the barycentric formula, f_j itself on a root"""
    w = roots(log2_n)
    n = len(w)
    assert len(f) == n
    for fj, wj in zip(f, w):
        if wj == z:
            return fj % R
    pre, run = [], 1      # 1 / (z - w_j) for every j from one inversion
    for wj in w:
        pre.append(run)
        run = run * (z - wj) % R
    inv, acc = pow(run, -1, R), 0
    for j in range(n - 1, -1, -1):
        acc = (acc + f[j] * w[j] % R * (inv * pre[j] % R)) % R
        inv = inv * (z - w[j]) % R
    return (pow(z, n, R) - 1) * pow(n, -1, R) % R * acc % R


def horner(coef, x):
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % R
    return acc


def evals_of(coef, log2_n):
    """a coefficient-form polynomial -> its values on the roots (bit-reversed order)"""
    return [horner(coef, w) for w in roots(log2_n)]


def blob_bytes(f):
    return b''.join(b32(v) for v in f)


def weight(seed, i):
    """the weight of item i of a batched check as include/nbls.h states it: r_i = BE64(SHA-256(seed || BE64(i))[0..8]) | 2^63"""
    return int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, 'big')).digest()[:8], 'big') | 1 << 63


def challenge(blob, commitment48, log2_n):
    """z = BE(SHA-256("FSBLOBVERIFY_V1_" || BE128(N) || blob || commitment)) mod r"""
    d = hashlib.sha256(b'FSBLOBVERIFY_V1_' + (1 << log2_n).to_bytes(16, 'big') + blob + commitment48).digest()
    return int.from_bytes(d, 'big') % R


class Setup:
    """[k]G1 compressed from the oracle (k = 0: the zero point's encoding) and [tau]G2 compressed by the engine's compress_batch on the oracle's point, as test_gpu_poly.py does"""
    def __init__(self, oracle, eng=None, tau=TAU):
        self.oracle, self.eng, self.tau, self.memo = oracle, eng, tau, {}

    def g1(self, k):
        k %= R
        if k == 0:
            return ZERO48
        if k not in self.memo:
            self.memo[k] = self.oracle.get_public_key(b32(k))
        return self.memo[k]

    def tau_g2(self, tau=None):
        pt = self.oracle.g2_mul(self.oracle.g2_generator(), self.tau if tau is None else tau)[1]
        return self.eng.compress_batch(pt, g2=True)[:96]

    def commit(self, f, log2_n):
        return self.g1(eval_roots(f, self.tau, log2_n))

    def proof(self, f, z, log2_n, y=None):
        """-> (y, proof) for the opening of f at z (y: the claimed value, by default the true one)"""
        pt = eval_roots(f, self.tau, log2_n)
        if y is None:
            y = eval_roots(f, z, log2_n)
        assert z != self.tau
        return y, self.g1((pt - y) * pow(self.tau - z, -1, R))

    def tuple_for(self, s, z, y):
        """-> (C, z, y, pi) with pi = [s]G1 and C = [y + s (tau - z)]G1: valid by construction, e(pi, [tau]G2) = e(C + [z]pi - [y]G1, G2) <=> s tau = c + z s - y.  No polynomial
        is needed, so s, z and y can be chosen freely (s = 0: the zero proof; y = s (z - tau): the zero commitment)"""
        return self.g1(y + s * (self.tau - z)), z, y, self.g1(s)

    def tuples_pooled(self, n, rnd, pool=32):
        """-> n valid tuples (C, z, y, pi) whose s and y come from a pool of non-zero values, z fresh: `pool` oracle multiplications for the proofs, one per commitment"""
        ss = [rnd.randrange(1, R) for _ in range(pool)]
        ys = [rnd.randrange(1, R) for _ in range(pool)]
        return [self.tuple_for(rnd.choice(ss), rnd.randrange(1, R), rnd.choice(ys)) for _ in range(n)]

    def blob_case(self, f, log2_n):
        """-> (blob, commitment, proof, z, y) of verify_blob_kzg_proof"""
        blob = blob_bytes(f)
        c = self.commit(f, log2_n)
        z = challenge(blob, c, log2_n)
        y, p = self.proof(f, z, log2_n)
        return blob, c, p, z, y
