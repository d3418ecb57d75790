"""Helpers of the KZG prover's tests (test_kzg_prove_sim.py, test_kzg_prove_abi.py, test_gpu_kzg_prove.py): the quotient of an opening in Python integers -- the within-domain
formula taken literally from EIP-4844's compute_quotient_eval_within_domain -- and the Lagrange basis of kzg_cases.py's test-only setup, [L_j(tau)]G1 from the oracle.  With tau
known, sum_j q_j L_j(tau) = (p(tau) - y) / (tau - z), also for z on a root, so the expected commitments and proofs are Setup.commit / Setup.proof: single multiples of the
generator, and equality with the device's bytes is exact.  Nothing here calls the code under test."""
from kzg_cases import R, LANES, b32, roots, eval_roots


def inv_all(vals):
    """1 / v mod r for every v (none zero) from one modular inversion"""
    pre, run = [], 1
    for v in vals:
        pre.append(run)
        run = run * v % R
    inv, out = pow(run, -1, R), [0] * len(vals)
    for k in range(len(vals) - 1, -1, -1):
        out[k] = inv * pre[k] % R
        inv = inv * vals[k] % R
    return out


def quotient(f, z, log2_n):
    """-> (y, [q_j]) of compute_kzg_proof_impl: q_j = (f_j - y) / (w_j - z); where z = w_m, q_m = sum_{j != m} (f_j - y) w_j / (z (z - w_j))"""
    w = roots(log2_n)
    n = len(w)
    assert len(f) == n
    y = eval_roots(f, z, log2_n)
    q = [0] * n
    m = w.index(z) if z in w else None
    js = [j for j in range(n) if j != m]
    for j, i in zip(js, inv_all([(w[j] - z) % R for j in js])):
        q[j] = (f[j] - y) * i % R
    if m is not None:
        for j, i in zip(js, inv_all([z * (z - w[j]) % R for j in js])):
            q[m] = (q[m] + (f[j] - y) * w[j] % R * i) % R
    return y, q


def structured(log2_n, rnd):
    """(name, f, z): the structured polynomials and evaluation points of test_kzg_sim.py -- z on the two sides of every place a lane's range ends"""
    n, w = 1 << log2_n, roots(log2_n)
    polys = {'random': [rnd.randrange(R) for _ in range(n)], 'zero': [0] * n, 'constant': [rnd.randrange(1, R)] * n, 'X': list(w),
             'r-1': [R - 1 if j == n // 2 else rnd.randrange(R) for j in range(n)]}
    points = [('random', rnd.randrange(R)), ('0', 0), ('r-1', R - 1)] + [('w%d' % j, w[j]) for j in on_roots(log2_n)]
    return [(pn + '@' + zn, f, z) for pn, f in polys.items() for zn, z in points]


def on_roots(log2_n):
    n = 1 << log2_n
    return sorted({0, n - 1, min(LANES - 1, n - 1), min(LANES, n - 1), max(n - LANES, 0), min(n - LANES + 1, n - 1) if n > LANES else 1})


_lagrange = {}


def lagrange_setup(setup, log2_n):
    """the N compressed points [L_j(tau)]G1 in bit-reversed order, L_j(tau) = (tau^N - 1) / N * w_j / (tau - w_j)"""
    key = (setup.tau, log2_n)
    if key not in _lagrange:
        w = roots(log2_n)
        n = len(w)
        fac = (pow(setup.tau, n, R) - 1) * pow(n, -1, R) % R
        _lagrange[key] = [setup.g1(fac * wj % R * pow(setup.tau - wj, -1, R)) for wj in w]
    return _lagrange[key]


def rows(vals):
    return b''.join(b32(v) for v in vals)
