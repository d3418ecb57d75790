"""Helpers of the large-transform tests (test_fr_ntt_large_cases.py, test_fr_ntt_large_sim.py, test_fr_ntt_large_abi.py, test_gpu_fr_ntt_large.py) in Python integers: the
decimation network of fr_exec.h stage by stage, its split into runs of global stages and shifted tails, the closed form of a sparse polynomial's values, and the composition of
a large transform from two transforms of at most 2^12 elements.  Nothing here calls the code under test."""
from kzg_cases import R, bitrev
from kzg_cells_cases import omega, to_evals, to_coeffs


def table(log2_n):
    """T_N[j] = omega_N^rev(j): the table of roots in bit-reversed order"""
    w = omega(log2_n)
    return [pow(w, bitrev(j, log2_n), R) for j in range(1 << log2_n)]


def stage(a, log2_n, j, tab):
    """stage j of the network towards the values, in place: 2^j blocks of half-length N / 2^(j+1), block blk with zeta = tab[2 blk]"""
    n = 1 << log2_n
    half = n >> (j + 1)
    for blk in range(1 << j):
        z = tab[2 * blk]
        for i in range(2 * half * blk, 2 * half * blk + half):
            x, y = a[i], a[i + half] * z % R
            a[i], a[i + half] = (x + y) % R, (x - y) % R
    return a


def global_stages(coef, log2_n, k):
    """the first k stages with the table of 2^k roots only (the prefix property)"""
    a, tab = list(coef), table(k) if k else [1]
    for j in range(k):
        stage(a, log2_n, j, tab)
    return a


def run_stages(a, log2_n, j0, j1, tab):
    """the stages j0 .. j1 - 1 as independent networks over the j1 - j0 bits of `row`, index = hi 2^(L - j0) + row 2^(L - j1) + lo: per (hi, lo) a column is gathered, run
    through its own stages -- stage j0 + k has the block number (hi << k) | (the top k bits of row) -- and scattered back"""
    q = j1 - j0
    for hi in range(1 << j0):
        for lo in range(1 << (log2_n - j1)):
            idx = [(hi << (log2_n - j0)) + (row << (log2_n - j1)) + lo for row in range(1 << q)]
            col = [a[i] for i in idx]
            for k in range(q):
                half = 1 << (q - 1 - k)
                for top in range(1 << k):
                    z = tab[2 * ((hi << k) | top)]
                    for r in range(2 * half * top, 2 * half * top + half):
                        x, y = col[r], col[r + half] * z % R
                        col[r], col[r + half] = (x + y) % R, (x - y) % R
            for i, v in zip(idx, col):
                a[i] = v
    return a


def block_shift(log2_n, t, block):
    """s_B = omega_N^rev_K(B), K = log2_n - t: block B of 2^t elements holds, after K stages, p mod (X^(2^t) - T_N[B]), and s_B^(2^t) = T_N[B]"""
    return pow(omega(log2_n), bitrev(block, log2_n - t), R)


def split_runs(k, p):
    """the K global stages in ceil(K / P) runs whose lengths differ by one at most, the longer ones first: [(j0, j1), ..]"""
    runs = (k + p - 1) // p
    base, more, out, j = k // runs, k % runs, [], 0
    for i in range(runs):
        q = base + (1 if i < more else 0)
        out.append((j, j + q))
        j += q
    return out


def compose_to_evals(coef, log2_n, t, shift=1):
    """to_evals of size 2^log2_n from transforms of size 2^K and 2^t: the K global stages are, for every column c of index = row 2^t + c, the size-2^K network over row
    (fact 2); block B then goes through the size-2^t transform with the shift s_B (fact 3)"""
    k, n = log2_n - t, 1 << log2_n
    s, a = 1, []
    for c in coef:
        a.append(c * s % R)
        s = s * shift % R
    for c in range(1 << t):
        col = to_evals(a[c::1 << t], k)
        a[c::1 << t] = col
    out = []
    for b in range(1 << k):
        out += to_evals(a[b << t:(b + 1) << t], t, block_shift(log2_n, t, b))
    assert len(out) == n
    return out


def compose_to_coeffs(vals, log2_n, t, shift=1):
    """the way back: the tails towards the coefficients with s_B, the columns towards the coefficients, then (1 / s)^i"""
    k = log2_n - t
    a = []
    for b in range(1 << k):
        a += to_coeffs(vals[b << t:(b + 1) << t], t, block_shift(log2_n, t, b))
    for c in range(1 << t):
        a[c::1 << t] = to_coeffs(a[c::1 << t], k)
    sinv, s, out = pow(shift, -1, R), 1, []
    for v in a:
        out.append(v * s % R)
        s = s * sinv % R
    return out


def sparse_eval(terms, log2_n, j, shift=1):
    """position j of the values of p = sum c_k X^(e_k), terms = [(e_k, c_k), ..]: p(shift * omega_N^rev(j))"""
    x = shift * pow(omega(log2_n), bitrev(j, log2_n), R) % R
    return sum(c * pow(x, e, R) for e, c in terms) % R
