"""Helpers of the Groth16 tests (test_groth16_cases.py, test_groth16_sim.py, test_groth16_abi.py, test_gpu_groth16.py): a test-only verifying key whose trapdoor scalars are
known, so that every point is a known multiple of a generator taken from the oracle, valid proofs by construction, the single-proof equation through the oracle's pairings, and
the weighted input sums in Python integers.  Nothing here calls the code under test."""
import ctypes as C
from kzg_cases import R, M256, ZERO48, NOT_VERIFIED, NON_CANONICAL, b32, weight  # noqa: F401  (weight: the weight function of every batched check)

ZERO96 = b'\xc0' + bytes(95)
ST_G16_C = 30
ONE12 = bytes(47) + b'\x01' + bytes(528)          # Fp12.ONE as 576 wire bytes
# the kernel's geometry (fr_exec.h: G16_TILE, G16_GROUPS, G16_ROWS_WG, G16_MAX_WG)
TILE, GROUPS, ROWS_WG, MAX_WG = 64, 16, 64, 1024


class Key:
    """alpha, beta, gamma, delta, ic_0 .. ic_m: the trapdoor of a key with m inputs.  alpha = [alpha]G1, beta = [beta]G2, .., IC_j = [ic_j]G1"""

    def __init__(self, oracle, m, rnd):
        self.oracle, self.m = oracle, m
        self.alpha, self.beta, self.gamma, self.delta = (rnd.randrange(1, R) for _ in range(4))
        self.ic = [rnd.randrange(1, R) for _ in range(m + 1)]
        self.g1gen, self.g2gen = oracle.g1_generator(), oracle.g2_generator()
        self.memo1, self.memo2 = {}, {}

    # ---- points from scalars
    def g1(self, k):
        """[k]G1 compressed (k = 0: the zero point's encoding)"""
        k %= R
        if k == 0:
            return ZERO48
        if k not in self.memo1:
            self.memo1[k] = self.oracle.get_public_key(b32(k))
        return self.memo1[k]

    def g1_aff(self, k):
        st, pt = self.oracle.g1_mul(self.g1gen, k % R)
        assert st == 0 and k % R
        return pt

    def g2_aff(self, k):
        k %= R
        assert k
        if k not in self.memo2:
            st, pt = self.oracle.g2_mul(self.g2gen, k)
            assert st == 0
            self.memo2[k] = pt
        return self.memo2[k]

    def g2(self, k):
        """[k]G2 compressed (k = 0: the zero point's encoding)"""
        if k % R == 0:
            return ZERO96
        out = C.create_string_buffer(96)
        self.oracle.lib.oracle_g2_compress(self.g2_aff(k), C.c_int(0), out)
        return out.raw

    def vk_points(self):
        """-> (alpha48, beta96, gamma96, delta96, [IC_0 .. IC_m] compressed): the arguments of nbls_groth16_vk_create"""
        return self.g1(self.alpha), self.g2(self.beta), self.g2(self.gamma), self.g2(self.delta), [self.g1(k) for k in self.ic]

    # ---- proofs in scalars
    def l_scalar(self, x):
        """the discrete logarithm of L = IC_0 + sum_j [x_j]IC_j"""
        assert len(x) == self.m
        return (self.ic[0] + sum(xj * kj for xj, kj in zip(x, self.ic[1:]))) % R

    def prove(self, x, rnd):
        """-> (a, b, c): a valid proof for the inputs x, A = [a]G1, B = [b]G2, C = [c]G1 with a b = alpha beta + gamma l + delta c"""
        while True:
            a, b = rnd.randrange(1, R), rnd.randrange(1, R)
            c = (a * b - self.alpha * self.beta - self.gamma * self.l_scalar(x)) * pow(self.delta, -1, R) % R
            if c:
                return a, b, c

    def holds_scalars(self, abc, x):
        a, b, c = abc
        return (a * b - self.alpha * self.beta - self.gamma * self.l_scalar(x) - self.delta * c) % R == 0

    def proof_bytes(self, abc):
        """A || B || C compressed: 192 bytes"""
        a, b, c = abc
        return self.g1(a) + self.g2(b) + self.g1(c)

    def inputs_for_zero_l(self, rnd):
        """a row x with L = the zero point: x_1 .. x_(m-1) random, x_m solves ic_0 + sum_j x_j ic_j = 0"""
        x = [rnd.randrange(R) for _ in range(self.m - 1)]
        rest = (self.ic[0] + sum(xj * kj for xj, kj in zip(x, self.ic[1:]))) % R
        x.append(-rest * pow(self.ic[self.m], -1, R) % R)
        assert self.l_scalar(x) == 0
        return x

    # ---- the single-proof equation through the oracle's pairings, on affine points
    def holds_pairing(self, a_aff, b_aff, c_aff, x):
        """e(A, B) e(L, -gamma) e(C, -delta) e(alpha, -beta) == 1; a zero L is a factor of one"""
        g1s, g2s = [a_aff, c_aff, self.g1_aff(self.alpha)], [b_aff, self.g2_aff(-self.delta), self.g2_aff(-self.beta)]
        l = self.l_scalar(x)
        if l:
            g1s.append(self.g1_aff(l)); g2s.append(self.g2_aff(-self.gamma))
        return self.oracle.miller_product(b''.join(g1s), b''.join(g2s), True) == ONE12

    def holds_pairing_scalars(self, abc, x):
        a, b, c = abc
        return self.holds_pairing(self.g1_aff(a), self.g2_aff(b), self.g1_aff(c), x)


def input_sums(rows, weights, pre=None):
    """-> ([S_0 .. S_m], statuses): S_0 = sum w_i, S_j = sum w_i x_ij mod r over the rows with pre[i] == 0 and every input < r; status = pre[i], else 21, else 0"""
    m = len(rows[0])
    sums, st = [0] * (m + 1), []
    for i, (row, w) in enumerate(zip(rows, weights)):
        p = pre[i] if pre is not None else 0
        bad = any(x >= R for x in row)
        st.append(p if p else NON_CANONICAL if bad else 0)
        if p or bad:
            continue
        sums[0] = (sums[0] + w) % R
        for j, x in enumerate(row):
            sums[j + 1] = (sums[j + 1] + w * x) % R
    return sums, st
