"""Helpers of the cell verifier's second tests (test_kzg_cells_adversarial_cases.py, test_gpu_kzg_cells_adversarial.py), on kzg_cases.py, kzg_cells_cases.py and
kzg_verify_cells_cases.py.  kzg_cases.Setup's test-only tau is known, so a cell tuple is four integers behind its bytes: the commitment C = [cm]G1, the proof pi = [q]G1, the
cell index k and the value I = I_k(tau) of the polynomial that interpolates the cell's c elements.  The cell holds exactly when  q tau^c = cm - I + s_k q  (mod r),  s_k = h_k^c,
and with a fixed seed the weights are known too (kzg_cases.weight), so `model` restates the combined check of nbls_kzg_verify_cells in those integers.  Nothing here calls the
code under test."""
import collections
from kzg_cases import R, ZERO48, horner, eval_roots, weight
from kzg_cells_cases import cell_shift, cell_quotient, to_evals
from kzg_verify_cells_cases import interp_coeffs, cell_bytes, cells_per_blob

CellItem = collections.namedtuple('CellItem', 'cm q k I cell_bytes C P')          # C = [cm]G1, P = pi = [q]G1, I = I_k(tau): the integers behind the bytes


def values(raw):
    """a cell's bytes -> its elements"""
    return [int.from_bytes(raw[j:j + 32], 'big') for j in range(0, len(raw), 32)]


class Forge:
    """the cell tuples of one shape (log2_n, log2_cell) over one Setup: valid by construction (tuple_for, honest) or with every integer chosen freely (item)"""
    def __init__(self, setup, log2_n, log2_cell):
        self.setup, self.shape, self.c, self.m = setup, (log2_n, log2_cell), 1 << log2_cell, cells_per_blob(log2_n, log2_cell)
        self.tau_c = pow(setup.tau, self.c, R)
        self._coeffs, self._cm, self._s = {}, {}, {}

    def s(self, k):
        """s_k = h_k^c, the constant of cell k's vanishing polynomial X^c - s_k"""
        if k not in self._s:
            self._s[k] = pow(cell_shift(k, *self.shape), self.c, R)
        return self._s[k]

    def coeffs(self, t):
        """a_(k,.) of the item's cell"""
        key = (t.k, t.cell_bytes)
        if key not in self._coeffs:
            self._coeffs[key] = interp_coeffs(values(t.cell_bytes), t.k, *self.shape)
        return self._coeffs[key]

    def at_tau(self, k, v):
        """I_k(tau) for the c values v: interp_coeffs and Horner's rule"""
        return horner(interp_coeffs([x % R for x in v], k, *self.shape), self.setup.tau)

    def item(self, cm, q, k, v):
        """every integer as given: the tuple holds or not"""
        assert len(v) == self.c and 0 <= k < self.m
        return CellItem(cm % R, q % R, k, self.at_tau(k, v), cell_bytes([x % R for x in v]), self.setup.g1(cm), self.setup.g1(q))

    def tuple_for(self, k, v, q):
        """like Setup.tuple_for: any cell index, any c values and any q, with cm = q tau^c + I - s_k q -- valid by construction, no polynomial needed (q = 0: the zero proof)"""
        return self.item(q * self.tau_c + self.at_tau(k, v) - self.s(k) * q, q, k, v)

    def honest(self, blob, k):
        """cell k of a kzg_verify_cells_cases.Blob: cm = p(tau) by the barycentric formula on the blob's values, q = q_k(tau), the integer behind cell_proof"""
        log2_n, log2_cell = self.shape
        assert (blob.log2_n, blob.log2_cell) == self.shape
        if id(blob) not in self._cm:
            self._cm[id(blob)] = (blob, eval_roots(blob.f, self.setup.tau, log2_n))
        cm = self._cm[id(blob)][1]
        q =horner(cell_quotient(blob.coef, k, log2_n, log2_cell), self.setup.tau)
        t = CellItem(cm, q, k, self.at_tau(k, blob.cells[k]), blob.cell(k), blob.commitment, blob.proof(k))
        assert (t.C, t.P) == (self.setup.g1(cm), self.setup.g1(q))
        return t

    def with_values(self, t, v):
        """the same commitment, proof and index over other elements"""
        return self.item(t.cm, t.q, t.k, v)

    def with_element(self, t, j, delta):
        v = values(t.cell_bytes)
        v[j] = (v[j] + delta) % R
        return self.with_values(t, v)

    def with_q(self, t, q):
        return t._replace(q=q % R, P=self.setup.g1(q))

    def with_cm(self, t, cm):
        return t._replace(cm=cm % R, C=self.setup.g1(cm))

    def defect(self, t):
        """q tau^c - cm + I - s_k q: zero exactly when the tuple holds"""
        return (t.q * self.tau_c - t.cm + t.I - self.s(t.k) * t.q) % R

    def holds(self, t):
        return self.defect(t) == 0

    def unit_at_tau(self, k, j):
        """the value at tau of the Lagrange polynomial of element j of cell k: what one added to that element adds to I_k(tau)"""
        return self.at_tau(k, [int(i == j) for i in range(self.c)])

    def cell_with_coeffs(self, k, a):
        """the c values whose interpolation polynomial at cell k has the coefficients a"""
        return to_evals([x % R for x in a], self.shape[1], shift=cell_shift(k, *self.shape))

    def model(self, items, seed):
        """the combined check in integers, r_j = weight(seed, j) by position -> ([sum r cm is zero, sum r s q is zero, every S_i is zero: the three parts of B are the zero
        point], A = sum r q is zero, B is zero, the check accepts).  B = sum r cm - sum_i S_i tau^i + sum r s q, and verifier_frame.h's rule -- A = B = O accepts, exactly one of them
        zero rejects, else the pairings decide tau^c A = B -- is `tau^c A = B` in the integers"""
        r = [weight(seed, j) for j in range(len(items))]
        s1 = sum(rj * t.cm for rj, t in zip(r, items)) % R
        s2 = sum(rj * self.s(t.k) * t.q for rj, t in zip(r, items)) % R
        col = [sum(rj * self.coeffs(t)[i] for rj, t in zip(r, items)) % R for i in range(self.c)]
        assert horner(col, self.setup.tau) == sum(rj * t.I for rj, t in zip(r, items)) % R
        a, b = sum(rj * t.q for rj, t in zip(r, items)) % R, (s1 + s2 - horner(col, self.setup.tau)) % R
        za, zb = a == 0, b == 0
        accepts = (za and zb) or (not za and not zb and a * self.tau_c % R == b)
        assert accepts == (a * self.tau_c % R == b)
        return [s1 == 0, s2 == 0, not any(col)], za, zb, accepts

    def weighted_defect(self, items, seed, at=None):
        """sum_j r_j defect_j over the places `at` (default: all): the combined check accepts exactly when the sum over all places is zero"""
        at = range(len(items)) if at is None else at
        return sum(weight(seed, j) * self.defect(items[j]) for j in at) % R


def call_args(items, extra_commitments=()):
    """the arguments of nbls_kzg_verify_cells for the items in their order: every distinct commitment once, in the order of first use, then `extra_commitments`"""
    cs, where, ci = [], {}, []
    for t in items:
        if t.C not in where:
            where[t.C] = len(cs)
            cs.append(t.C)
        ci.append(where[t.C])
    return cs + list(extra_commitments), ci, [t.k for t in items], [t.cell_bytes for t in items], [t.P for t in items]


def solve2(a, b, c, d, e, f):
    """x, y with a x + b y = e and c x + d y = f (mod r)"""
    det = (a * d - b * c) % R
    assert det
    inv = pow(det, -1, R)
    return (e * d - b * f) * inv % R, (a * f - e * c) * inv % R


def balance(r, xs):
    """x with sum_j r_j xs_j + r_last x = 0, r of one more entry than xs"""
    return -sum(rj * x for rj, x in zip(r, xs)) * pow(r[len(xs)], -1, R) % R


# The zero-flag matrix of the combined check: row -> ([sum r cm, sum r s q, every S_i: is zero], A is zero, B is zero), stated here, built by matrix_rows and asserted with
# Forge.model before any call.  All sixteen combinations of the three flags with A zero or not are here (no flag and A not zero with B not zero is every ordinary call).  Valid
# tuples give B = tau^c A, so among them B is zero exactly when A is.  Hence two kinds of row CANNOT be built from valid tuples and are forged instead (FORGED_ROWS: some tuple
# does not hold, the call must reject): exactly two flags with A zero -- B would be the third part alone, not zero, against B = tau^c A = O --, and all three flags with A not
# zero -- B = O against tau^c A != O.
MATRIX = {'none, A zero':              ([False, False, False], True, True),
          'none, A zero, B not':       ([False, False, False], True, False),
          'none, B zero':              ([False, False, False], False, True),
          'cm':                        ([True, False, False], False, False),
          'cm, A zero':                ([True, False, False], True, True),
          'sq':                        ([False, True, False], False, False),
          'sq, A zero':                ([False, True, False], True, True),
          'S, zero cells':             ([False, False, True], False, False),
          'S, cancelling cells':       ([False, False, True], False, False),
          'S, A zero':                 ([False, False, True], True, True),
          'cm and sq':                 ([True, True, False], False, False),
          'cm and sq, A zero':         ([True, True, False], True, False),
          'cm and S':                  ([True, False, True], False, False),
          'cm and S, A zero':          ([True, False, True], True, False),
          'sq and S':                  ([False, True, True], False, False),
          'sq and S, A zero':          ([False, True, True], True, False),
          'all three, A zero':         ([True, True, True], True, True),
          'all three, A not zero':     ([True, True, True], False, True)}
FORGED_ROWS = {'none, A zero, B not', 'none, B zero', 'cm and sq, A zero', 'cm and S, A zero', 'sq and S, A zero', 'all three, A not zero'}
S_ROWS = [name for name in MATRIX if 'S' in name or 'all three' in name]          # the rows in which the part -sum [S_i][tau^i]G1 is the zero point


def matrix_rows(fg, seed, rnd):
    """row name -> the items of a call that reaches it under `seed`: two or three cells, every commitment and every proof a non-zero point"""
    r = [weight(seed, j) for j in range(3)]
    k = [1, fg.m - 1, 2]          # three cell indices with three different s_k
    s = [fg.s(x) for x in k]
    d = [(fg.tau_c - x) % R for x in s]
    assert len(set(s)) == 3 and all(d)
    rv = lambda: rnd.randrange(2, R)
    cell = lambda: [rv() for _ in range(fg.c)]
    zero = [0] * fg.c
    inv = lambda x: pow(x, -1, R)

    def cell_at(kk, want):
        """random values moved by a constant, which moves I_k(tau) by that constant, so that I_k(tau) = want"""
        w = cell()
        shift = (want - fg.at_tau(kk, w)) % R
        return [(x + shift) % R for x in w]

    def three_q():
        """q_0, q_1, q_2 with sum r q = 0 and sum r s q = 0"""
        q0 = rv()
        q1, q2 = solve2(r[1], r[2], r[1] * s[1], r[2] * s[2], -r[0] * q0, -r[0] * s[0] * q0)
        return [q0, q1, q2]
    rows = {}
    q0 = rv()
    sq1 = balance([r[0] * s[0], r[1] * s[1]], [q0])          # r_0 s_0 q_0 + r_1 s_1 q_1 = 0
    a1 = balance(r, [q0])                                    # r_0 q_0 + r_1 q_1 = 0
    # -- valid rows
    t0 = fg.tuple_for(k[0], cell(), q0)
    rows['none, A zero'] = [t0, fg.tuple_for(k[1], cell(), a1)]          # (two cell indices: with one, sum r s q = s sum r q would be zero with A)
    v1 = cell()
    cm1 = balance(r, [t0.cm])
    rows['cm'] = [t0, fg.tuple_for(k[1], v1, (cm1 - fg.at_tau(k[1], v1)) * inv(d[1]))]
    rows['cm, A zero'] = [t0, fg.tuple_for(k[1], cell_at(k[1], cm1 - a1 * d[1]), a1)]
    rows['sq'] = [t0, fg.tuple_for(k[1], cell(), sq1)]
    rows['sq, A zero'] = [fg.tuple_for(kk, cell(), q) for kk, q in zip(k, three_q())]
    rows['S, zero cells'] = [fg.tuple_for(k[0], zero, q0), fg.tuple_for(k[1], zero, rv())]
    a0 = cell()
    rows['S, cancelling cells'] = [fg.tuple_for(k[0], fg.cell_with_coeffs(k[0], a0), q0),
                                   fg.tuple_for(k[1], fg.cell_with_coeffs(k[1], [-r[0] * x * inv(r[1]) for x in a0]), rv())]
    rows['S, A zero'] = [fg.tuple_for(k[0], zero, q0), fg.tuple_for(k[1], zero, a1)]
    rows['cm and sq'] = [t0, fg.tuple_for(k[1], cell_at(k[1], cm1 - sq1 * d[1]), sq1)]
    rows['cm and S'] = [fg.tuple_for(k[0], zero, q0), fg.tuple_for(k[1], zero, balance([r[0] * d[0], r[1] * d[1]], [q0]))]
    rows['sq and S'] = [fg.tuple_for(k[0], zero, q0), fg.tuple_for(k[1], zero, sq1)]
    rows['all three, A zero'] = [fg.tuple_for(k[0], zero, q0), fg.tuple_for(k[0], zero, a1)]
    # -- forged rows: at least one tuple does not hold
    rows['none, A zero, B not'] = [fg.with_element(rows['none, A zero'][0], 0, 1), rows['none, A zero'][1]]
    f = [fg.item(rv(), q0, k[0], cell()), fg.item(rv(), rv(), k[1], cell())]
    q2, v2 = rv(), cell()
    b2 = balance(r, [t.cm + fg.s(t.k) * t.q - t.I for t in f])          # the third cell's share of B, so that the three shares cancel
    rows['none, B zero'] = f + [fg.item(b2 - s[2] * q2 + fg.at_tau(k[2], v2), q2, k[2], v2)]
    qs = three_q()
    cms = [rv(), rv()]
    rows['cm and sq, A zero'] = [fg.item(cm, q, kk, cell()) for cm, q, kk in zip(cms + [balance(r, cms)], qs, k)]
    c0 = rv()
    rows['cm and S, A zero'] = [fg.item(c0, q0, k[0], zero), fg.item(balance(r, [c0]), a1, k[1], zero)]
    rows['sq and S, A zero'] = [fg.item(rv(), q, kk, zero) for q, kk in zip(three_q(), k)]
    rows['all three, A not zero'] = [fg.item(c0, q0, k[0], zero), fg.item(balance(r, [c0]), sq1, k[1], zero)]
    assert set(rows) == set(MATRIX)
    return rows


__all__ = ['MATRIX', 'FORGED_ROWS', 'S_ROWS', 'matrix_rows','CellItem', 'Forge', 'ZERO48', 'values', 'call_args', 'solve2', 'balance']
