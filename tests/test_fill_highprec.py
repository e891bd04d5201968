"""The high-precision reference of the covariance fill on the CPU: NumPy's own evaluation of every kernel meets the
bound the device is held to (tests/test_fill_gpu.py) -- so the bound's constants are not tuned to the device --, the
generator reproduces the committed fixture, and the long-double derivative of the gradient tests agrees with mpmath."""
import json
import os

import numpy as np
import pytest

from oracle import kernel_formulas as kf
from tests import _fill_fixture as ff


def test_fixture_covers_every_kernel_and_regime():
    cases, d = ff.load()
    kernels = {c['kernel'] for c in cases}
    assert len(kernels) == 21 + 6 + 1
    assert {c['regime'] for c in cases} == {'R1', 'R2', 'R3', 'R4', 'R5', 'R6'}
    assert max(len(c['ops']) for c in cases) >= 13            # deep7: seven kernels, seven stack slots
    for c in cases:
        assert c['n'] <= 1000 and 40 <= d['t_' + c['tset']].size <= 200
    size = sum(os.path.getsize(os.path.join(ff.GOLDEN, 'fill_highprec.' + e)) for e in ('npz', 'json'))
    assert size < 2 * 2**20


def test_numpy_evaluation_meets_the_bound():
    cases, d = ff.load()
    fails = []
    for c in cases:
        K = ff.numpy_matrix(c, d['t_' + c['tset']])
        for seq in ((False, True) if c['seq'] else (False,)):
            v = ff.violations(K, c, d, seq=seq)
            if v:
                fails.append('%s%s: %d elements, e.g. %r' % (c['name'], ' (seq)' if seq else '', len(v), v[0]))
    assert not fails, '\n'.join(fails)


def test_generator_reproduces_the_fixture():
    """A handful of cases regenerated (the whole fixture: python oracle/gen_fill_highprec.py, about a minute) --
    one per kind of reference: exact only, with NumPy's rounding sequence, a harmonic kernel, a degenerate one and the
    deep composite."""
    pytest.importorskip('mpmath')
    from oracle import gen_fill_highprec as gen
    cases, d = ff.load()
    names = ['QuasiPeriodic_R5_3', 'SquaredExponential_R6_0', 'HarmonicPeriodic_R2_0', 'deep7_R1_0', 'RationalQuadratic_R4_0']
    meta, arrays = gen.generate(set(names))
    assert sorted(m['name'] for m in meta) == sorted(names)
    for key in ('t_R1', 't_R2', 't_R3', 't_R5', 't_R6'):
        assert np.array_equal(arrays[key], d[key])
    want = {c['name']: c for c in cases}
    for m in meta:
        c = want[m['name']]
        assert json.dumps({k: m[k] for k in ('expr', 'ops', 'pars', 'n')}) == \
            json.dumps({k: c[k] for k in ('expr', 'ops', 'pars', 'n')})
        for key in ('i', 'j', 'hi', 'lo', 'kappa'):
            got = arrays[key][m['off']:m['off'] + m['n']]
            assert np.array_equal(got, d[key][c['off']:c['off'] + c['n']], equal_nan=True), (m['name'], key)
        if c['seq']:
            for key in ('seq_hi', 'seq_lo', 'seq_kappa'):
                got = arrays[key][m['seq_off']:m['seq_off'] + m['n']]
                assert np.array_equal(got, d[key][c['seq_off']:c['seq_off'] + c['n']], equal_nan=True), (m['name'], key)


@pytest.mark.parametrize('expr', ['c.Periodic(0.9, 0.3, 0.8)', 'c.NewPeriodic(1.2, 0.9, 0.3, 0.8)',
                                  'c.SquaredExponential(1.0, 0.1)', 'c.QuasiPeriodic(1.0, 16.0, 0.3, 0.7)',
                                  'c.RQP(1.2, 0.9, 16.0, 0.3, 0.7)', 'c.GammaExp(1.2, 1.5, 0.1)',
                                  'c.Derivative(c.QuasiPeriodic(1.1, 16.0, 0.3, 0.6))',
                                  'c.SquaredExponential(1.0, 8.0) * c.Periodic(1.0, 0.3, 0.5)'])
def test_long_double_derivative_agrees_with_mpmath(expr):
    """oracle.kernel_formulas.dk_dpars_longdouble (the gradient tests' reference) within 1e-11 of mpmath's derivative at
    sampled elements, at the short period and short length scale of those tests."""
    mpmath = pytest.importorskip('mpmath')
    from gpyrn_amd import covfunc
    mp = mpmath.mp
    mp.dps = 40
    k = eval(expr, {'c': covfunc})
    ops, pars = k._device_program()
    ops, pars = [tuple(int(v) for v in o) for o in ops], [float(v) for v in pars]
    rng = np.random.default_rng(4)
    ti, tj = rng.uniform(0, 60, 40), rng.uniform(0, 60, 40)
    ti[:5] = tj[:5] + rng.uniform(-0.5, 0.5, 5)                  # and a few close pairs
    got = kf.dk_dpars_longdouble(np, ops, pars, ti, tj, np.zeros(40, dtype=bool))
    A = kf.mp_arith(mp)
    for l in range(len(pars)):
        want = []
        for a, b in zip(ti, tj):
            def f(v, a=a, b=b):
                q = [mp.mpf(x) for x in pars]
                q[l] = v
                return kf.program(A, ops, q, mp.mpf(a), mp.mpf(b), False)
            want.append(float(mp.diff(f, mp.mpf(pars[l]))))
        want = np.array(want)
        scale = np.abs(want).max()
        np.testing.assert_allclose(np.asarray(got[l], dtype=float), want, rtol=1e-11, atol=1e-11 * scale,
                                   err_msg='%s parameter %d' % (expr, l))
