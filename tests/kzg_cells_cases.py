"""Helpers of the PeerDAS tests (test_kzg_cells_cases.py, test_kzg_cells_sim.py, test_kzg_cells_abi.py, test_gpu_kzg_cells.py): the transform between coefficients and values in
Python integers -- an O(N log N) network of the textbook shape (bit-reversal first, natural-order twiddles: not the one the device runs), checked against Horner's rule by
test_kzg_cells_cases.py --, the cells of EIP-7594 (compute_cells: the extension evaluated on the coset g <omega_N>, g = omega_2N), the quotient of a cell's proof by the
recurrence and by schoolbook long division, and the monomial basis of kzg_cases.py's test-only setup: with tau known, a cell's proof is [q_k(tau)]G1, one multiple of the
generator from the oracle.  Nothing here calls the code under test."""
from kzg_cases import R, b32, bitrev, roots, horner

LANES = 512      # FR_NTT_LANES: lane t of a workgroup owns the elements t, t + 512, .. and the butterflies t, t + 512, .. of a stage


def omega(log2_n):
    return pow(7, (R - 1) >> log2_n, R)


_twiddles = {}


def _stage_twiddles(w, n):
    """per stage of _dft the half-block of powers of that stage's root, memoised: the tests transform many polynomials of one size"""
    if (w, n) not in _twiddles:
        out, size = [], 2
        while size <= n:
            wl, t, tw = pow(w, n // size, R), 1, []
            for _ in range(size // 2):
                tw.append(t)
                t = t * wl % R
            out.append(tw)
            size *= 2
        _twiddles[(w, n)] = out
    return _twiddles[(w, n)]


def _dft(v, w):
    """natural order in, natural order out: X[m] = sum_t v[t] w^(m t), len(v) a power of two, w a primitive root of that order"""
    n = len(v)
    bits = n.bit_length() - 1
    a = [v[bitrev(i, bits)] for i in range(n)]
    for tw in _stage_twiddles(w, n):
        half = len(tw)
        for start in range(0, n, 2 * half):
            for j, t in enumerate(tw, start):
                x, y = a[j], a[j + half] * t % R
                a[j], a[j + half] = (x + y) % R, (x - y) % R
    return a


def to_evals(coef, log2_n, shift=1):
    """coefficients (natural order) -> the values p(shift * w_j) in bit-reversed order"""
    n = 1 << log2_n
    assert len(coef) == n
    s, scaled = 1, []
    for c in coef:
        scaled.append(c * s % R)
        s = s * shift % R
    x = _dft(scaled, omega(log2_n))
    return [x[bitrev(j, log2_n)] for j in range(n)]


def to_coeffs(vals, log2_n, shift=1):
    """the way back; shift != 0"""
    n = 1 << log2_n
    assert len(vals) == n
    x = _dft([vals[bitrev(m, log2_n)] for m in range(n)], pow(omega(log2_n), -1, R))
    ninv, sinv, s, out = pow(n, -1, R), pow(shift, -1, R), 1, []
    for v in x:
        out.append(v * ninv % R * s % R)
        s = s * sinv % R
    return out


def coset_shift(log2_n):
    """g = omega_2N"""
    return omega(log2_n + 1)


def cells(f, log2_n, log2_cell):
    """compute_cells: the blob f (values on w_j, bit-reversed order) -> its 2 N / c cells of c values each"""
    ext = list(f) + to_evals(to_coeffs(f, log2_n), log2_n, coset_shift(log2_n))
    c = 1 << log2_cell
    return [ext[c * k:c * k + c] for k in range(len(ext) // c)]


def cell_shift(k, log2_n, log2_cell):
    """h_k = g^rev(k) over log2_n + 1 - log2_cell bits: coset_for_cell(k) = h_k <omega_c>"""
    return pow(coset_shift(log2_n), bitrev(k, log2_n + 1 - log2_cell), R)


def cell_points(k, log2_n, log2_cell):
    h, wc = cell_shift(k, log2_n, log2_cell), omega(log2_cell)
    return [h * pow(wc, bitrev(j, log2_cell), R) % R for j in range(1 << log2_cell)]


def cell_quotient(coef, k, log2_n, log2_cell):
    """the floor quotient of p by X^c - s_k, s_k = h_k^c, by the recurrence q_i = p_(i+c) + s_k q_(i+c); N coefficients, the top c of them zero"""
    n, c = 1 << log2_n, 1 << log2_cell
    s = pow(cell_shift(k, log2_n, log2_cell), c, R)
    q = [0] * n
    for i in range(n - c - 1, -1, -1):
        q[i] = (coef[i + c] + s * q[i + c]) % R
    return q


def cell_quotient_schoolbook(coef, k, log2_n, log2_cell):
    """the same by long division, the divisor written out as a polynomial: -> (quotient of N coefficients, remainder of c)"""
    n, c = 1 << log2_n, 1 << log2_cell
    d = [(-pow(cell_shift(k, log2_n, log2_cell), c, R)) % R] + [0] * (c - 1) + [1]
    rem, q = list(coef), [0] * n
    for top in range(n - 1, c - 1, -1):
        lead = rem[top]
        q[top - c] = lead
        for i, di in enumerate(d):
            rem[top - c + i] = (rem[top - c + i] - lead * di) % R
    assert not any(rem[c:])
    return q, rem[:c]


_monomial = {}


def monomial_setup(setup, log2_n):
    """the N compressed points [tau^i]G1, natural order"""
    key = (setup.tau, log2_n)
    if key not in _monomial:
        t, pts = 1, []
        for _ in range(1 << log2_n):
            pts.append(setup.g1(t))
            t = t * setup.tau % R
        _monomial[key] = pts
    return _monomial[key]


def cell_proof(setup, coef, k, log2_n, log2_cell):
    """[q_k(tau)]G1"""
    return setup.g1(horner(cell_quotient(coef, k, log2_n, log2_cell), setup.tau))


def borders(log2_n):
    """the indices on either side of every place a lane's range ends, and the two ends"""
    n = 1 << log2_n
    return sorted({0, n - 1} | {i for b in range(LANES, n, LANES) for i in (b - 1, b)} | ({n // 2 - 1, n // 2} if n > 1 else set()))


def structured(log2_n, rnd):
    """(name, polynomial as N integers): the structured inputs of the transform's tests, for either direction"""
    n = 1 << log2_n
    out = [('zero', [0] * n), ('constant', [rnd.randrange(1, R)] + [0] * (n - 1)), ('X', [0, 1] + [0] * (n - 2)), ('X^(N-1)', [0] * (n - 1) + [1]), ('all r-1', [R - 1] * n),
           ('random', [rnd.randrange(R) for _ in range(n)])]
    for i in borders(log2_n):
        v = [0] * n
        v[i] = rnd.randrange(1, R)
        out.append(('single@%d' % i, v))
    return out


def rows(vals):
    return b''.join(b32(v) for v in vals)
