"""Device tests of hash-to-curve BEHIND expand_message_xmd on chosen uniform bytes (nbls_map_uniform_batch, csrc/pipelines_codec.cpp): the 64-byte -> Fp reduction, both SWU maps,
the addition on the isogenous curve, the isogenies and cofactor clearing on the inputs where they branch (tests/h2c_cases.py), in every form the pipelines dispatch to -- the Fp2
and the norm-method square root, the plain and two-lane point chains, the wide and the one-lane exponentiation kernels -- and at every position of a wavefront.  Expected bytes are
the reference's own (tests/golden/ref_h2c_map.json.gz, tools/gen_golden4.mjs); tests/test_oracle.py holds the fixture to the case lists and counts the classes they cover."""
import ctypes as C
import hashlib
import importlib

import pytest
import torch

import goldenio
from goldenio import hx

pytestmark = pytest.mark.gpu
EINVAL = -1
NORM_MIN_DEFAULT, PT_LS2_MAX_DEFAULT = 32768, 4096
IN_BYTES, OUT_BYTES = {0: 256, 1: 128, 2: 128, 3: 64}, {0: 192, 1: 192, 2: 96, 3: 96}

_CASES = goldenio.load('ref_h2c_map.json.gz')['cases']
ORDINARY = {k: [v for v in _CASES if v['kind'] == k and not v['degenerate']] for k in range(4)}
DEGENERATE = {k: [v for v in _CASES if v['kind'] == k and v['degenerate']] for k in (0, 2)}
S = ORDINARY[0]


@pytest.fixture(scope='module')
def engine():
    pkg = importlib.import_module('noble-bls12-381_amd')
    return pkg.Engine(0)


@pytest.fixture
def eng(engine):
    try:
        yield engine
    finally:
        engine.set_h2c_norm_min(NORM_MIN_DEFAULT); engine.set_pt_ls2_max(PT_LS2_MAX_DEFAULT)


def tiled(vs, n):
    return (vs * (n // len(vs) + 1))[:n]


def check(eng, kind, vs, what):
    """one call on the items vs: every output is the fixture's, every status 0"""
    a = OUT_BYTES[kind]
    out, st = eng.map_uniform_batch(kind, b''.join(hx(v['uniform']) for v in vs))
    bad = [(i, v['name']) for i, v in enumerate(vs) if out[a * i:a * i + a] != hx(v['aff']) or st[i] != 0]
    assert not bad, (what, len(bad), bad[:8])


def test_case_lists_are_the_size_the_dispatch_thresholds_need():
    assert 128 < len(S) < 200 and 2 * len(S) <= 3072 < 2 * 1600        # |S|: two elements per item in the wide exponentiation kernels; 1,600 items: the one-lane kernels
    assert all(len(ORDINARY[k]) > 40 for k in (1, 2, 3)) and all(len(DEGENERATE[k]) == 3 for k in (0, 2))


@pytest.mark.parametrize('norm_min', [1 << 30, 0])
def test_form_matrix(eng, norm_min):
    """S in one call by the Fp2 (h2c_a / h2c_b1) or the norm-method square root (h2c_na / nm / nb) x the point chains in their two-lane or plain forms, with the powers in the wide
    kernels; then 1,600 items, whose 3,200 elements put the powers in the one-lane kernels"""
    eng.set_h2c_norm_min(norm_min)
    for ls2_max in (PT_LS2_MAX_DEFAULT, 0):
        eng.set_pt_ls2_max(ls2_max)
        check(eng, 0, S, ('S', norm_min, ls2_max))
    eng.set_pt_ls2_max(PT_LS2_MAX_DEFAULT)
    check(eng, 0, tiled(S, 1600), ('1600', norm_min))


@pytest.mark.parametrize('norm_min', [1 << 30, 0])
def test_single_items(eng, norm_min):
    """n = 1, the shape of verify / sign: t = 0 (the exceptional denominator), a delta = 0 case, the all-ones string, t = (0, p - 1)"""
    eng.set_h2c_norm_min(norm_min)
    by_name = {v['name']: v for v in S}
    delta0 = next(v for v in S if v['name'].startswith('u0: a1=0 leg1') and 'delta=0' in v['name'])
    for v in (by_name['u0: t=(0,0)'], by_name['u1: t=(0,0)'], delta0, by_name['u0: c0=2^512-1'], by_name['u1: c1=2^512-1'], by_name['u0: t=(0,p-1)']):
        check(eng, 0, [v], ('single', norm_min))


@pytest.mark.parametrize('norm_min', [1 << 30, 0])
def test_wavefront_positions(eng, norm_min):
    """S rotated by 1 and by 63: the structured items move through the first and last lanes of a wavefront and into the ragged last one; the same bytes, permuted"""
    eng.set_h2c_norm_min(norm_min)
    for r in (1, 63):
        check(eng, 0, S[r:] + S[:r], ('rotated', r, norm_min))


@pytest.mark.parametrize('kind', [1, 2, 3])
def test_other_kinds(eng, kind):
    """G2 encode, G1 hash and G1 encode on their lists (the powers in the wide kernels) and tiled to 3,200 items (3,200 elements and more: the one-lane kernels)"""
    check(eng, kind, ORDINARY[kind], ('list', kind))
    check(eng, kind, tiled(ORDINARY[kind], 3200), ('3200', kind))


@pytest.mark.parametrize('kind,norm_min', [(0, 1 << 30), (0, 0), (2, NORM_MIN_DEFAULT)])
def test_degenerate_items_leave_their_neighbours_alone(eng, kind, norm_min):
    """u0 = +-u1 mod p at the first lane, at lane 31 and at the end of a call of ordinary items: outside the contract, pinned as the zero point (status 1, zero bytes: pt_add_generic
    gives (0 : 0 : 0) or (0 : Y : 0), the isogeny and the complete cofactor formulas keep Z = 0); every ordinary item is still the fixture's, and the call succeeds"""
    eng.set_h2c_norm_min(norm_min)
    vs = list(ORDINARY[kind][:70])
    d = DEGENERATE[kind]
    vs[0:0] = [d[0]]; vs[31:31] = [d[1]]; vs.append(d[2])
    assert vs[0] is d[0] and vs[31] is d[1] and vs[-1] is d[2]
    a = OUT_BYTES[kind]
    out, st = eng.map_uniform_batch(kind, b''.join(hx(v['uniform']) for v in vs))
    for i, v in enumerate(vs):
        if v['degenerate']:
            assert st[i] == 1 and out[a * i:a * i + a] == bytes(a), (i, v['name'])
        else:
            assert st[i] == 0 and out[a * i:a * i + a] == hx(v['aff']), (i, v['name'])


def test_agreement_with_the_message_path(eng, oracle):
    """the uniform bytes of 8 messages through map_uniform_batch == the message calls, for each kind"""
    msgs = [hashlib.sha256(b'h2c-map-%d' % i).digest()[:1 + 5 * i] for i in range(8)]
    dst = b'NBLS-TEST-V01-CS02-with-expander-SHA256-128'
    for kind, (g2, encode) in {0: (True, False), 1: (True, True), 2: (False, False), 3: (False, True)}.items():
        uni = b''.join(oracle.expand_message_xmd(m, dst, IN_BYTES[kind]) for m in msgs)
        out, st = eng.map_uniform_batch(kind, uni)
        assert out == eng.hash_to_curve_batch(msgs, dst, g2=g2, encode=encode) and st == bytes(8), kind


def test_refusals(eng):
    """NBLS_EINVAL before any device work: unknown kinds, a missing context or buffers with n > 0; n = 0 is fine; nothing is allocated and the context works afterwards"""
    lib, h = eng.lib, eng.h
    v = S[0]
    uni, out, st = hx(v['uniform']), C.create_string_buffer(192), C.create_string_buffer(1)
    assert lib.nbls_map_uniform_batch(h, 0, 1, uni, out, st) == 0 and out.raw == hx(v['aff'])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        assert lib.nbls_map_uniform_batch(h, -1, 1, uni, out, st) == EINVAL
        assert lib.nbls_map_uniform_batch(h, 4, 1, uni, out, st) == EINVAL
        assert lib.nbls_map_uniform_batch(None, 0, 1, uni, out, st) == EINVAL
        assert lib.nbls_map_uniform_batch(h, 0, 1, None, out, st) == EINVAL
        assert lib.nbls_map_uniform_batch(h, 0, 1, uni, None, st) == EINVAL
        assert lib.nbls_map_uniform_batch(h, 4, 0, None, None, None) == EINVAL
        assert lib.nbls_map_uniform_batch(h, 0, 0, None, None, None) == 0
    with pytest.raises(Exception):
        eng.map_uniform_batch(5, uni)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    out2 = C.create_string_buffer(192)
    assert lib.nbls_map_uniform_batch(h, 0, 1, uni, out2, None) == 0 and out2.raw == hx(v['aff'])        # status may be NULL
