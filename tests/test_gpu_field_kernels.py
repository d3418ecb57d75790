"""The stand-alone field kernels on the device (-m gpu), fed directly through nbls_field_kernel_raw: the Montgomery inverse (nbls_fp_inv_kernel, nbls_fp_inv_wide_kernel) and
the four fixed-exponent powers (nbls_fp_pow_kernel, nbls_fp2_pow_kernel, nbls_pow_wide_kernel), each in both of its forms, on the structured operand lists the host simulator
is checked on (tests/field_cases.py, tests/test_vm_sim.py::test_fp_inverse_edge_cases / ::test_pow_chains).  The host runs the algorithms through a host policy; the device has
its own -- ds_swizzle broadcasts, DPP row shifts and quad_perm swaps, readlane, a ballot, __clzll -- and inside the pipelines it only ever sees pseudo-random values, on which
paths such as negate_exact's zero low limbs or the `small` window of the inverse's approximation are taken with probability about 2^-28.

Every element is checked against Python integers (Fp.invert math.ts:134-156, Fp.pow / Fp.sqrt 251-264, Fp2.pow 463-465 with the exponents of Fp2.sqrt and sqrt_div_fp2,
521-538, 1196-1198): exact limbs, the stated bound of its form, the value mod p; and byte for byte against the simulator's function of the same form."""
import ctypes as C
import importlib
import pytest
import field_cases as fc
import vmsim_py

pytestmark = pytest.mark.gpu
P = fc.P
INV = 4
KINDS = {0: 'pow_p+1_4', 1: 'fp2pow_p2+7_16', 2: 'fp2pow_p2-9_16', 3: 'pow_p-3_4', 4: 'inverse'}
FORMS = {1: 'per-lane', 2: 'limb-per-lane'}
ALL = [pytest.param(k, f, id='%s-%s' % (KINDS[k], FORMS[f])) for k in KINDS for f in FORMS]
PREFIXES = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257)      # four elements per wavefront (wide inverse), pairs of lanes (one-lane Fp2 power), wavefront and block ends


@pytest.fixture(scope='module')
def eng():
    return importlib.import_module('noble-bls12-381_amd').Engine(0)


def is_fp2(kind):
    return kind in (1, 2)


def bound(kind, form):
    """the stated bound of a stored value, times ten: below 2 p (one-lane inverse), 21 p / 10 (wide inverse), 4 p (one-lane powers), 2 p (wide powers)"""
    return (20 if form == 1 else 21) if kind == INV else (40 if form == 1 else 20)


class Cases:
    """the operand lists as integers and raw bytes, the Python-integer results, and the simulator's and the device's outputs for the whole list of every (kind, form), each
    computed once on first use"""

    def __init__(self, eng):
        self.eng = eng
        self.sim = vmsim_py.load()
        self.sim.nbls_sim_fp_pow_wide.restype = C.c_ulong
        self.sim.nbls_sim_wide_violations.restype = C.c_ulong
        self._want, self._sim, self._dev = {}, {}, {}

    def values(self, kind):
        """the flat list of raw values (Fp2: c0, c1, c0, c1, ...)"""
        if kind == INV:
            return fc.inverse_inputs()
        if is_fp2(kind):
            return tuple(c for pr in fc.fp2_pow_inputs() for c in pr)
        return fc.pow_inputs()

    def structured(self, kind):
        """(first element, count) of the structured part of the list, in elements (Fp2: pairs; the whole list, so that it reaches past 257)"""
        if kind == INV:
            return 2000, len(fc.inverse_inputs()) - 2000
        if is_fp2(kind):
            return 0, len(fc.fp2_pow_inputs())
        return 0, fc.N_POW_STRUCTURED

    def want(self, kind):
        """what every output value is congruent to, flat"""
        if kind not in self._want:
            if kind == INV:
                w = [fc.inverse_expected(x) for x in fc.inverse_inputs()]
            elif is_fp2(kind):
                w = [c for pr in fc.fp2_pow_inputs() for c in fc.fp2_pow_expected(pr, kind)]
            else:
                w = [fc.pow_expected(x, kind) for x in fc.pow_inputs()]
            self._want[kind] = w
        return self._want[kind]

    def sim_out(self, kind, form):
        if (kind, form) not in self._sim:
            xs = self.values(kind)
            n = len(xs) // (2 if is_fp2(kind) else 1)
            src = C.create_string_buffer(fc.raw(xs), fc.RAW * len(xs)); dst = C.create_string_buffer(fc.RAW * len(xs))
            if kind == INV:
                self.sim.nbls_sim_wide_violations()
                (self.sim.nbls_sim_fp_inv if form == 1 else self.sim.nbls_sim_fp_inv_wide)(C.c_uint(n), src, dst)
                assert self.sim.nbls_sim_wide_violations() == 0
            elif form == 1:
                self.sim.nbls_sim_fp_pow(C.c_uint(n), src, dst, kind)
            else:
                assert self.sim.nbls_sim_fp_pow_wide(C.c_uint(n), src, dst, kind) == 0      # no violated 32 / 64-bit assumption in the host model: the inputs are inside the contract
            self._sim[(kind, form)] = dst.raw
        return self._sim[(kind, form)]

    def dev_out(self, kind, form):
        if (kind, form) not in self._dev:
            xs = self.values(kind)
            self._dev[(kind, form)] = self.eng.field_kernel_raw(kind, form, len(xs) // (2 if is_fp2(kind) else 1), fc.raw(xs))[:fc.RAW * len(xs)]
        return self._dev[(kind, form)]


@pytest.fixture(scope='module')
def cases(eng):
    return Cases(eng)


def check_elements(out, xs, want, kind, limit10, what):
    """the simulator tests' own checks of every element: exact limbs, zero padding, the value bound and the value mod p"""
    assert len(out) == fc.RAW * len(xs)
    for k, x in enumerate(xs):
        w = fc.words(out, k)
        assert all(l < (1 << 28) for l in w[:14]) and w[14] == 0 and w[15] == 0, (what, KINDS[kind], k, hex(x), [hex(l) for l in w])
        got = sum(l << (28 * i) for i, l in enumerate(w[:14]))
        assert 10 * got < limit10 * P, (what, KINDS[kind], k, hex(x), hex(got))
        assert got % P == want[k], (what, KINDS[kind], k, hex(x), hex(got))


@pytest.mark.parametrize('kind,form', ALL)
def test_whole_lists_against_python_and_the_simulator(cases, kind, form):
    """every operand of the shared lists (3,171 inversion inputs; the Fp power inputs; the Fp2 pairs) through one form of one kernel: the per-element checks against Python
    integers, then byte for byte against the simulator's function of that form (the two forms of a kernel return different representatives, so the comparison is per form)"""
    out = cases.dev_out(kind, form)
    xs = cases.values(kind)
    check_elements(out, xs, cases.want(kind), kind, bound(kind, form), FORMS[form])
    ref = cases.sim_out(kind, form)
    diff = [k for k in range(len(xs)) if out[fc.RAW * k:fc.RAW * k + fc.RAW] != ref[fc.RAW * k:fc.RAW * k + fc.RAW]]
    assert not diff, (KINDS[kind], FORMS[form], len(diff), [(k, hex(xs[k])) for k in diff[:4]])


@pytest.mark.parametrize('kind,form', ALL)
def test_position_in_the_launch(eng, cases, kind, form):
    """prefixes of the structured list whose ends fall inside a row group, a lane pair, a wavefront and a block: each gives the first n results of the full run and writes
    nothing behind element n; the list rotated by one and by three elements, so that every structured value meets more than one lane, row and wavefront position"""
    per = 2 if is_fp2(kind) else 1                      # raw elements per element of the launch
    first, count = cases.structured(kind)
    esz = fc.RAW * per
    xs = cases.values(kind)[per * first:per * (first + count)]
    blob = fc.raw(xs)
    full = cases.dev_out(kind, form)[esz * first:esz * (first + count)]
    assert eng.field_kernel_raw(kind, form, count, blob)[:esz * count] == full      # a launch of the structured part alone: a result does not depend on its neighbours
    for n in PREFIXES:
        assert n <= count
        out = C.create_string_buffer(b'\x7f' * (esz * (n + 2)), esz * (n + 2))
        got = eng.field_kernel_raw(kind, form, n, blob[:esz * n], out)
        assert got[:esz * n] == full[:esz * n], (KINDS[kind], FORMS[form], n)
        assert got[esz * n:] == b'\x7f' * (2 * esz), (KINDS[kind], FORMS[form], n)
    for rot in (1, 3):
        got = eng.field_kernel_raw(kind, form, count, blob[esz * rot:] + blob[:esz * rot])[:esz * count]
        assert got == full[esz * rot:] + full[:esz * rot], (KINDS[kind], FORMS[form], rot)


@pytest.mark.parametrize('kind', list(KINDS), ids=list(KINDS.values()))
@pytest.mark.parametrize('n', [1, 5000])
def test_dispatch_of_the_pipelines(eng, cases, kind, n):
    """form 0 -- what run_pow / run_inv_buf take for this n: one limb per lane for a single element, one element per lane for 5,000 -- gives the expected values"""
    per = 2 if is_fp2(kind) else 1
    xs, want = cases.values(kind), cases.want(kind)
    first, _ = cases.structured(kind)
    m = len(xs) // per
    idx = [(first + i) % m for i in range(n)]            # the list cycled, from its structured part on
    vals = [xs[per * i + c] for i in idx for c in range(per)]
    out = eng.field_kernel_raw(kind, 0, n, fc.raw(vals))[:fc.RAW * per * n]
    check_elements(out, vals, [want[per * i + c] for i in idx for c in range(per)], kind, max(bound(kind, 1), bound(kind, 2)), 'dispatch n=%d' % n)


def test_inversion_threshold_selects_the_form(eng, cases):
    """NBLS_TUNE_INV_WIDE_MAX moves run_inv_buf's choice: never wide -> byte-equal to the one-lane form, always wide -> byte-equal to the one-limb-per-lane form"""
    xs = cases.values(INV)
    blob = fc.raw(xs)
    try:
        eng.set_inv_wide_max(0)
        assert eng.field_kernel_raw(INV, 0, len(xs), blob)[:len(blob)] == cases.dev_out(INV, 1)
        eng.set_inv_wide_max(1 << 30)
        assert eng.field_kernel_raw(INV, 0, len(xs), blob)[:len(blob)] == cases.dev_out(INV, 2)
    finally:
        eng.set_inv_wide_max(4096)
    assert cases.dev_out(INV, 1) != cases.dev_out(INV, 2)      # the comparison above can tell the forms apart


def test_arguments(eng):
    """NBLS_EINVAL for an unknown kind or form and for missing buffers with n > 0; n = 0 is NBLS_OK and touches nothing"""
    f = eng.lib.nbls_field_kernel_raw
    one = fc.raw([1])
    out = C.create_string_buffer(b'\x7f' * 128, 128)
    for kind, form in ((-1, 1), (5, 1), (0, -1), (0, 3), (4, 3)):
        assert f(eng.h, kind, form, 1, one, out) == -1, (kind, form)
    assert f(eng.h, 0, 1, 1, None, out) == -1 and f(eng.h, 0, 1, 1, one, None) == -1
    assert f(None, 0, 1, 1, one, out) == -1
    for kind in KINDS:
        for form in (0, 1, 2):
            assert f(eng.h, kind, form, 0, None, None) == 0
            assert f(eng.h, kind, form, 0, one, out) == 0
    assert out.raw == b'\x7f' * 128
