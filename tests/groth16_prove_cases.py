"""Helpers of the Groth16 prover's tests (test_groth16_prove_cases.py, test_groth16_prove_sim.py, test_groth16_prove_abi.py, test_gpu_groth16_prove.py): random satisfied
R1CS instances, the matrix-vector products and the quotient h = (a b - c) / (X^N - 1) in Python integers (the transforms are kzg_cells_cases.py's, shift 7), and a test-only
proving key on groth16_cases.Key whose trapdoor (tau, alpha, beta, gamma, delta) is known: every query point is a known multiple of a generator, the matching verifying key
comes with it, and the expected proof is three scalars -- no polynomial arithmetic between the witness and the expected bytes.  Nothing here calls the code under test."""
from kzg_cases import R, ZERO48, b32, bitrev
from kzg_cells_cases import omega, to_coeffs, to_evals
from groth16_cases import Key

UNSATISFIED, NON_CANONICAL = 24, 21
SHIFT = 7
ROW_WAVE_DEFAULT = 32          # g16p_exec.h G16P_ROW_WAVE_DEFAULT


def instance(log2_n, n_vars, m, rnd, lengths=None, z=None, skip=()):
    """-> (A, B, C, z): three matrices as lists of rows of (column, coefficient) and an assignment z (z_0 = 1) that satisfies them.  lengths: per row the entries of its A row
    and of its B row (default: 1 .. 3 each for 3/4 of the N rows); the columns of a row are distinct.  Each C row is the single entry a_j b_j / z_k on a column with z_k != 0.
    skip: columns no row of any matrix names.  z: given values (z[0] = 1), else random"""
    N = 1 << log2_n
    if z is None:
        z = [1] + [rnd.randrange(R) for _ in range(n_vars - 1)]
    if lengths is None:
        lengths = [(rnd.randrange(1, 4), rnd.randrange(1, 4)) for _ in range(3 * N // 4)]
    assert len(lengths) <= N and z[0] == 1 and len(z) == n_vars
    cols = [i for i in range(n_vars) if i not in skip]
    nonzero = [i for i in cols if z[i] % R]
    A, B, Cm = [], [], []
    for la, lb in lengths:
        ra = [(c, rnd.randrange(1, R)) for c in rnd.sample(cols, min(la, len(cols)))]
        rb = [(c, rnd.randrange(1, R)) for c in rnd.sample(cols, min(lb, len(cols)))]
        a, b = sum(v * z[c] for c, v in ra) % R, sum(v * z[c] for c, v in rb) % R
        k = rnd.choice(nonzero)
        A.append(ra); B.append(rb); Cm.append([(k, a * b * pow(z[k], -1, R) % R)])
    return A, B, Cm, z


def family(log2_n, n_free, rows, rnd, skip=()):
    """an instance with many witnesses: columns 0 .. n_free - 1 are free (column 0 is the one), row j multiplies two random combinations of up to three free columns into
    the variable n_free + j of its own: C row j = [(n_free + j, 1)].  -> (A, B, C, witness): witness(rnd) draws the free values and computes the others; n_vars = n_free + rows.
    The variables n_free .. are named by C alone: their a_query and b_query points are the zero point.  skip: free columns no row names at all"""
    assert rows <= 1 << log2_n
    cols = [i for i in range(n_free) if i not in skip]
    A = [[(c, rnd.randrange(1, R)) for c in rnd.sample(cols, min(rnd.randrange(1, 4), len(cols)))] for _ in range(rows)]
    B = [[(c, rnd.randrange(1, R)) for c in rnd.sample(cols, min(rnd.randrange(1, 4), len(cols)))] for _ in range(rows)]
    Cm = [[(n_free + j, 1)] for j in range(rows)]

    def witness(r):
        z = [1] + [r.randrange(R) for _ in range(n_free - 1)]
        return z + [sum(v * z[c] for c, v in ra) * sum(v * z[c] for c, v in rb) % R for ra, rb in zip(A, B)]
    return A, B, Cm, witness


def matvec(M, z, log2_n):
    """M z as N values in natural order (row j at index j); the rows past the last given one are empty"""
    out = [sum(v * z[c] for c, v in row) % R for row in M]
    return out + [0] * ((1 << log2_n) - len(out))


def bitrev_order(v, log2_n):
    """position rev(j) holds entry j: the order of nbls_fr_ntt's values"""
    out = [0] * len(v)
    for j, x in enumerate(v):
        out[bitrev(j, log2_n)] = x
    return out


def quotient(a, b, c, log2_n):
    """a, b, c: values in bit-reversed order -> the N coefficients of h = (a b - c) / (X^N - 1), through the coset of 7 as the issue's formulas state it"""
    kinv = pow(pow(SHIFT, 1 << log2_n, R) - 1, -1, R)
    ea, eb, ec = (to_evals(to_coeffs(v, log2_n), log2_n, SHIFT) for v in (a, b, c))
    return to_coeffs([(x * y - w) * kinv % R for x, y, w in zip(ea, eb, ec)], log2_n, SHIFT)


def poly_at(coef, x):
    acc = 0
    for cf in reversed(coef):
        acc = (acc * x + cf) % R
    return acc


class ProvingKey(Key):
    """the trapdoor key of one instance: tau, alpha, beta, gamma, delta known.  at[X][i] = the column polynomial X_i at tau = sum_j X[j][i] L_j(tau) with
    L_j(tau) = Z(tau) omega^j / (N (tau - omega^j)); k[i] = beta A_i + alpha B_i + C_i at tau; IC_i = [k_i / gamma]G1 for i <= m"""

    def __init__(self, oracle, log2_n, n_vars, m, matrices, rnd):
        Key.__init__(self, oracle, m, rnd)
        self.log2_n, self.n_vars, self.matrices = log2_n, n_vars, matrices
        N, w = 1 << log2_n, omega(log2_n)
        self.tau = rnd.randrange(2, R)
        self.zt = (pow(self.tau, N, R) - 1) % R
        assert self.zt
        ninv, lag, wj = pow(N, -1, R), [], 1
        for _ in range(N):
            lag.append(self.zt * wj % R * ninv % R * pow(self.tau - wj, -1, R) % R)
            wj = wj * w % R
        self.lagrange = lag
        self.at = []
        for M in matrices:
            col = [0] * n_vars
            for j, row in enumerate(M):
                for c, v in row:
                    col[c] = (col[c] + v * lag[j]) % R
            self.at.append(col)
        a, b, c = self.at
        self.k = [(self.beta * a[i] + self.alpha * b[i] + c[i]) % R for i in range(n_vars)]
        ginv = pow(self.gamma, -1, R)
        self.ic = [self.k[i] * ginv % R for i in range(m + 1)]
        self.dinv = pow(self.delta, -1, R)

    def h_scalars(self):
        """the discrete logarithms of h_query: tau^k Z(tau) / delta, k < N - 1"""
        out, t = [], self.zt * self.dinv % R
        for _ in range((1 << self.log2_n) - 1):
            out.append(t)
            t = t * self.tau % R
        return out

    def l_scalars(self):
        return [self.k[i] * self.dinv % R for i in range(self.m + 1, self.n_vars)]

    def points(self, h_query=None):
        """-> the arguments of Engine.groth16_pk behind the matrices (h_query: the N - 1 compressed points when the caller has made them elsewhere)"""
        a, b, _ = self.at
        return dict(alpha_g1_48=self.g1(self.alpha), beta_g1_48=self.g1(self.beta), beta_g2_96=self.g2(self.beta), delta_g1_48=self.g1(self.delta), delta_g2_96=self.g2(self.delta),
                    a_query48=[self.g1(x) for x in a], b_g1_query48=[self.g1(x) for x in b], b_g2_query96=[self.g2(x) for x in b], l_query48=[self.g1(x) for x in self.l_scalars()],
                    h_query48=[self.g1(x) for x in self.h_scalars()] if h_query is None else h_query)

    def proof_scalars(self, z, r, s):
        """a = alpha + (Az)(tau) + r delta;  b = beta + (Bz)(tau) + s delta;
        c = (sum_{i > m} k_i z_i + (Az)(tau) (Bz)(tau) - (Cz)(tau)) / delta + s a + r b - r s delta"""
        az, bz, cz = (sum(x * y for x, y in zip(col, z)) % R for col in self.at)
        a, b = (self.alpha + az + r * self.delta) % R, (self.beta + bz + s * self.delta) % R
        aux = sum(self.k[i] * z[i] for i in range(self.m + 1, self.n_vars))
        c = ((aux + az * bz - cz) * self.dinv + s * a + r * b - r * s * self.delta) % R
        return a, b, c

    def expected_proof(self, z, r, s):
        return self.proof_bytes(self.proof_scalars(z, r, s))

    def r_for_zero_a(self, z):
        """the r with A = the zero point: -(alpha + (Az)(tau)) / delta"""
        az = sum(x * y for x, y in zip(self.at[0], z)) % R
        return -(self.alpha + az) * self.dinv % R


def csr(M):
    """a matrix as the C ABI takes it: (offsets, columns, the coefficients' bytes)"""
    offs, cols, vals = [0], [], []
    for row in M:
        for c, v in row:
            cols.append(c); vals.append(b32(v))
        offs.append(len(cols))
    return offs, cols, b''.join(vals)


def scalar_arrays(z, r, s, h, m, mask_a, mask_b, mask_l, dead=False):
    """the three scalar arrays of a proof as g16p_exec.h states them: (z | 1 | r), (z | 1 | s), (z_aux | h_0 .. h_(N-2) | s | r | -r s), a masked entry zero, all zero where dead"""
    sa = [0 if k else x for x, k in zip(z, mask_a)] + [1, r]
    sb = [0 if k else x for x, k in zip(z, mask_b)] + [1, s]
    sc = [0 if k else x for x, k in zip(z[m + 1:], mask_l)] + h[:-1] + [s, r, -r * s % R]
    if dead:
        sa, sb, sc = ([0] * len(v) for v in (sa, sb, sc))
    return sa, sb, sc
