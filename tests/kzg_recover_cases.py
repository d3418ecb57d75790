"""Helpers of the recovery tests (test_kzg_recover_cases.py, test_kzg_recover_sim.py, test_kzg_recover_abi.py, test_gpu_kzg_recover.py): recover_cells_and_kzg_proofs of
EIP-7594 in Python integers by the SPECIFICATION's route (recover_polynomialcoeff), not the device's: the received values E (zero where a cell is missing) times the vanishing
polynomial Z of the missing cells, one transform of size 2 N to coefficients, the values of that product and of Z on the coset of 7, their quotient, one transform of size 2 N
back with the shift 7.  The project's extension is in the bit-reversed order over 2 N (ext[i] = p(w_i), ext[N + i] = p(g w_i)), which is what to_coeffs / to_evals of
kzg_cells_cases.py take at log2_n + 1.  On top of it the contract of nbls_kzg_recover_cells: the rules on the index set, the canonical check, and the comparison of the recomputed
cells with every given one.  Nothing here calls the code under test."""
from kzg_cases import R, NON_CANONICAL, bitrev
from kzg_cells_cases import omega, to_evals, to_coeffs, cells, borders

BAD_CELLS, INCONSISTENT = 22, 23
COSET = 7          # the multiplicative generator: 7 H meets no root of unity


def n_cells(log2_n, log2_cell):
    return 2 << (log2_n - log2_cell)


def cell_root(k, log2_n, log2_cell):
    """s_k = h_k^c: entry k of the table of the M roots in bit-reversed order"""
    lm = log2_n + 1 - log2_cell
    return pow(omega(lm), bitrev(k, lm), R)


def indices_ok(idx, log2_n, log2_cell):
    m = n_cells(log2_n, log2_cell)
    return len(idx) >= m // 2 and all(0 <= k < m for k in idx) and len(set(idx)) == len(idx)


def vanishing(missing, log2_n, log2_cell):
    """the coefficients of Z(x) = prod over the missing k of (x^c - s_k), 2 N of them (its degree is at most N)"""
    zs = [1]
    for k in missing:
        s, nxt = cell_root(k, log2_n, log2_cell), [0] * (len(zs) + 1)
        for i, a in enumerate(zs):
            nxt[i + 1] = (nxt[i + 1] + a) % R
            nxt[i] = (nxt[i] - a * s) % R
        zs = nxt
    out = [0] * (2 << log2_n)
    for i, a in enumerate(zs):
        out[i << log2_cell] = a
    return out


def recover_coeffs(idx, given, log2_n, log2_cell):
    """recover_polynomialcoeff: the cells `given` (lists of c integers < r) with the numbers idx (a valid index set) -> the first N coefficients of the quotient"""
    n, c, m, big = 1 << log2_n, 1 << log2_cell, n_cells(log2_n, log2_cell), log2_n + 1
    ext = [0] * (2 * n)
    for k, cell in zip(idx, given):
        ext[c * k:c * k + c] = cell
    zc = vanishing([k for k in range(m) if k not in set(idx)], log2_n, log2_cell)
    zv = to_evals(zc, big)
    pz = to_coeffs([e * z % R for e, z in zip(ext, zv)], big)
    num, den = to_evals(pz, big, COSET), to_evals(zc, big, COSET)
    assert all(den)
    return to_coeffs([a * pow(b, -1, R) % R for a, b in zip(num, den)], big, COSET)[:n]


def recover(idx, given, log2_n, log2_cell):
    """the contract of nbls_kzg_recover_cells for one blob: -> (status, the 2 N / c cells or None, the N coefficients or None)"""
    if not indices_ok(idx, log2_n, log2_cell):
        return BAD_CELLS, None, None
    if any(v >= R for cell in given for v in cell):
        return NON_CANONICAL, None, None
    coef = recover_coeffs(idx, given, log2_n, log2_cell)
    out = cells(to_evals(coef, log2_n), log2_n, log2_cell)
    if any(out[k] != list(cell) for k, cell in zip(idx, given)):
        return INCONSISTENT, None, None
    return 0, out, coef


def patterns(log2_n, log2_cell, rnd):
    """(name, index list): the index sets the tests walk; every one of them is valid"""
    m = n_cells(log2_n, log2_cell)
    every = list(range(m))
    shuffled, drop = rnd.sample(every, m), rnd.randrange(m)
    out = [('first half', every[:m // 2]), ('second half', every[m // 2:]), ('even', every[0::2]), ('odd', every[1::2]), ('random half', sorted(rnd.sample(every, m // 2))),
           ('random half + 1', sorted(rnd.sample(every, m // 2 + 1))), ('all but one', [k for k in every if k != drop]), ('all', every),
           ('descending', sorted(rnd.sample(every, m // 2 + (m > 2)), reverse=True)), ('shuffled', shuffled[:m // 2 + m // 4])]
    return out


def blobs_for(log2_n, log2_cell, rnd):
    """(name, coefficients): random, the zero polynomial, degree < c, and a single non-zero coefficient at each of borders(log2_n)"""
    n, c = 1 << log2_n, 1 << log2_cell
    out = [('random', [rnd.randrange(R) for _ in range(n)]), ('zero', [0] * n), ('degree < c', [rnd.randrange(1, R) for _ in range(c)] + [0] * (n - c))]
    for i in borders(log2_n):
        v = [0] * n
        v[i] = rnd.randrange(1, R)
        out.append(('single@%d' % i, v))
    return out
