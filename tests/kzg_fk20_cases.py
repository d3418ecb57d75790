"""Helpers of the FK20 tests (test_kzg_fk20_cases.py, test_kzg_fk20_sim.py, test_gpu_kzg_fk20.py): the identities behind nbls_kzg_compute_cells_and_proofs_fk20 in Python
integers.  With N = 2^log2_n coefficients p_i, c = 2^log2_cell per cell, n' = N / c, M = 2 n' cells and omega = omega_M:

  1. proof_k = sum_(u <= n' - 2) [s_k^u] h_u,   h_u = sum_(j < c) sum_(t <= n' - 2 - u) [p_(j + c (t + u + 1))] [tau^(j + c t)]G1
  2. X^[j][v] = sum_(t <= n' - 2) [omega^(v t)] [tau^(j + c (n' - 2 - t))]G1          (fixed; c M points)
  3. a^[j][v] = sum_(t < n') p_(j + c t) omega^(v t),  y^_v = sum_j [a^[j][v]] X^[j][v],  h_u = IDFT_M(y^)_(n' - 1 + u)
  4. proof_k = sum_v [B[k][v]] y^_v,  B[k][v] = 1 / M sum_(u <= n' - 2) s_k^u omega^(-v (n' - 1 + u))

THE ORDER OF v, written once: position i of every array stands for the exponent v = bitrev(i, log2 M) -- omega^v is then entry i of the table of the M roots in bit-reversed
order, which is what the device's Fr network leaves from natural input.  Points are kept as their discrete logarithms (tau is known to the tests), so [a]P is a product mod r.
Nothing here calls the code under test."""
from kzg_cases import R, bitrev
from kzg_cells_cases import omega, cell_shift

FK_LANES = 256   # FR_FK_LANES: the lanes of a workgroup of the scalars kernel


def dims(log2_n, log2_cell):
    """(N, c, n', M, log2 M)"""
    lm = log2_n + 1 - log2_cell
    return 1 << log2_n, 1 << log2_cell, 1 << (log2_n - log2_cell), 1 << lm, lm


def pos_root(i, lm):
    """omega_M^v for position i: v = bitrev(i)"""
    return pow(omega(lm), bitrev(i, lm), R)


def s_of(k, log2_n, log2_cell):
    """s_k = h_k^c"""
    return pow(cell_shift(k, log2_n, log2_cell), 1 << log2_cell, R)


def h_direct(coef, u, tau, log2_n, log2_cell):
    """identity 1's h_u as a multiple of the generator"""
    _, c, np_, _, _ = dims(log2_n, log2_cell)
    return sum(coef[j + c * (t + u + 1)] * pow(tau, j + c * t, R) for j in range(c) for t in range(np_ - 1 - u)) % R


def scalars(coef, log2_n, log2_cell):
    """a^[j][i]: the per-blob scalars, position order"""
    _, c, np_, M, lm = dims(log2_n, log2_cell)
    w = [pos_root(i, lm) for i in range(M)]
    return [[sum(coef[j + c * t] * pow(w[i], t, R) for t in range(np_)) % R for i in range(M)] for j in range(c)]


def scalars_flat(coef, log2_n, log2_cell):
    """one blob's part of pass A's scalar array: entry i * c + j"""
    _, c, _, M, _ = dims(log2_n, log2_cell)
    a = scalars(coef, log2_n, log2_cell)
    return [a[j][i] for i in range(M) for j in range(c)]


def xhat(tau, log2_n, log2_cell):
    """X^[j][i] as multiples of the generator"""
    _, c, np_, M, lm = dims(log2_n, log2_cell)
    w = [pos_root(i, lm) for i in range(M)]
    return [[sum(pow(w[i], t, R) * pow(tau, j + c * (np_ - 2 - t), R) for t in range(np_ - 1)) % R for i in range(M)] for j in range(c)]


def yhat(coef, tau, log2_n, log2_cell):
    _, c, _, M, _ = dims(log2_n, log2_cell)
    a, x = scalars(coef, log2_n, log2_cell), xhat(tau, log2_n, log2_cell)
    return [sum(a[j][i] * x[j][i] for j in range(c)) % R for i in range(M)]


def idft(yh, lm):
    """y_m = 1 / M sum_i y^_i omega^(-v(i) m)"""
    M = 1 << lm
    wi = [pow(pos_root(i, lm), -1, R) for i in range(M)]
    minv = pow(M, -1, R)
    return [minv * sum(yh[i] * pow(wi[i], m, R) for i in range(M)) % R for m in range(M)]


def matrix(log2_n, log2_cell):
    """B[k][i]"""
    _, _, np_, M, lm = dims(log2_n, log2_cell)
    wi = [pow(pos_root(i, lm), -1, R) for i in range(M)]
    minv = pow(M, -1, R)
    s = [s_of(k, log2_n, log2_cell) for k in range(M)]
    out = []
    for k in range(M):
        row = []
        for i in range(M):
            term, acc, step = pow(wi[i], np_ - 1, R), 0, s[k] * wi[i] % R          # the sum term by term: s_k^u wi^(n' - 1 + u)
            for _ in range(np_ - 1):
                acc += term
                term = term * step % R
            row.append(minv * acc % R)
        out.append(row)
    return out


def proofs_fk20(coef, tau, log2_n, log2_cell):
    """every proof of the blob, as multiples of the generator, by identities 2 - 4"""
    _, _, _, M, _ = dims(log2_n, log2_cell)
    B, yh = matrix(log2_n, log2_cell), yhat(coef, tau, log2_n, log2_cell)
    return [sum(B[k][i] * yh[i] for i in range(M)) % R for k in range(M)]
