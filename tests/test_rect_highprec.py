"""The high-precision reference of prediction's rectangular fills (tests/golden/rect_highprec, oracle/gen_rect_highprec.py)
on the CPU: the fixture holds what the device tests rely on (tests/test_rect_fill_gpu.py), NumPy's own evaluation of
gpyrn_amd.covfunc on the rectangular arguments -- the delta terms of the two forms added here, as include/gprn_hip.h states
them -- meets the bound of tests/_fill_fixture.py in every case, and the generator reproduces the committed fixture."""
import json
import os

import numpy as np
import pytest

from oracle import kernel_formulas as kf
from tests import _fill_fixture as ff

WHITENOISE = kf.KID['WHITENOISE']


def test_fixture_has_the_square_fixtures_cases_and_the_times_the_device_tests_need():
    meta, d = ff.load_rect()
    cases = meta['cases']
    square, _ = ff.load()
    assert [(c['name'], c['expr'], c['ops'], c['pars']) for c in cases] == \
        [(c['name'], c['expr'], c['ops'], c['pars']) for c in square]
    assert {c['regime'] for c in cases} == {'R1', 'R2', 'R3', 'R4', 'R5', 'R6'}
    ns = meta['ns']
    assert ns == 137 and meta['tiny_nugget'] == 1.25e-12 and meta['setup_nugget'] == 1e-6
    assert {c['kernel'] for c in cases if not c['nugget']} == {'Polynomial', 'HarmonicPeriodic', 'QuasiHarmonicPeriodic'}
    # (numpy_rect spells the delta of WhiteNoise out for the kernel on its own)
    assert all(len(c['ops']) == 1 for c in cases if any(o[0] == 0 and o[1] == WHITENOISE for o in c['ops']))
    for reg in ('R1', 'R2', 'R3', 'R5', 'R6'):
        t, ts = d['t_' + reg], d['ts_' + reg]
        assert t.size == 200 and ts.size == ns
        assert (ts < t.min()).sum() >= ns // 10 and (ts > t.max()).sum() >= ns // 10
        assert ((ts > t.min()) & (ts < t.max())).sum() >= ns // 2
        same = ts[:, None] == t[None, :]
        assert same.any(axis=1).sum() >= 8                                  # bit-equal to data times
        assert same[:16, :16].sum() >= 2 and not np.array_equal(same[:16, :16], same[:16, :16].T)
        assert same[ns - 1, t.size - 1]
        twins = (ts[:, None] == ts[None, :]).sum() - ns
        assert twins >= 2                                                   # two t* equal to each other
        assert not np.all(np.diff(ts) > 0)                                  # rows in no order
        if reg in ('R2', 'R6'):
            assert t.min() > 2.4e6                                          # absolute BJD
    for c in cases:
        t, ts = d['t_' + c['tset']], d['ts_' + c['tset']]
        s = slice(c['off'], c['off'] + c['n'])
        i, j = d['i'][s].astype(int), d['j'][s].astype(int)
        assert c['n'] <= 300 and len(set(zip(i, j))) == c['n']
        have = set(zip(i, j))
        assert all((a, b) in have for a in range(16) for b in range(16))
        pairs = set(zip(*np.nonzero(ts[:, None] == t[None, :])))
        assert pairs <= have and c['co_n'] == len(pairs)
        assert (i == ns - 1).sum() >= 8 and (j == t.size - 1).sum() >= 8
        co = d['co_k'][c['co_off']:c['co_off'] + c['co_n']]
        assert set(zip(i[co], j[co])) == pairs
    for e in ('npz', 'json'):
        assert os.path.getsize(os.path.join(ff.GOLDEN, 'rect_highprec.' + e)) < 2**20


def _numpy_fill(meta, c, d, form):
    """(K* as a matrix that holds the sample, k** as a column) from NumPy's evaluation of covfunc, the form's deltas added"""
    t, ts = d['t_' + c['tset']], d['ts_' + c['tset']]
    s = slice(c['off'], c['off'] + c['n'])
    i, j = d['i'][s].astype(int), d['j'][s].astype(int)
    nug = ff.rect_nugget(meta, c, form)
    delta = (ts[i] == t[j]) if form == ff.POST else np.zeros(i.size, dtype=bool)
    Ks = np.full((ts.size, t.size), np.nan)
    Ks[i, j] = ff.numpy_rect(c, ts, t, i, j, delta) + np.where(delta, nug, 0.0)
    a = np.arange(ts.size)
    kss = ff.numpy_rect(c, ts, ts, a, a, np.ones(ts.size, dtype=bool)) + nug
    return Ks, kss[:, None]


def test_numpy_evaluation_meets_the_bound():
    meta, d = ff.load_rect()
    fails = []
    for c in meta['cases']:
        for form in (ff.REF, ff.POST):
            Ks, kss = _numpy_fill(meta, c, d, form)
            (ck, dk), (cs, ds) = ff.rect_views(c, d, form, meta['ns'])
            for what, v in (('K*', ff.violations(Ks, ck, dk)), ('k**', ff.violations(kss, cs, ds))):
                if v:
                    fails.append('%s form %d %s: %d elements, e.g. %r' % (c['name'], form, what, len(v), v[0]))
    assert not fails, '\n'.join(fails)


def test_the_two_forms_differ_exactly_as_documented():
    """The posterior form is the reference form but for the delta terms: K* differs at coincident pairs alone -- by the
    nugget, and for WhiteNoise by w^2 --, k** by the two nuggets' difference."""
    meta, d = ff.load_rect()
    for c in meta['cases']:
        co = slice(c['co_off'], c['co_off'] + c['co_n'])
        ref_hi = d['hi'][c['off']:c['off'] + c['n']][d['co_k'][co]]
        post_hi = d['co_hi'][co]
        fin = np.isfinite(post_hi) & np.isfinite(ref_hi)
        q = c['kss_off']
        kr, kp = d['kss_hi'][q:q + meta['ns']], d['kss_hi'][q + meta['ns']:q + 2 * meta['ns']]
        if c['kernel'] == 'WhiteNoise':
            assert np.all(ref_hi == 0.0) and np.allclose(post_hi, c['pars'][0]**2 + 1e-6, rtol=1e-15)
        elif c['nugget']:
            assert np.allclose((post_hi - ref_hi)[fin], 1e-6, rtol=0, atol=1e-15 * np.abs(post_hi[fin]).max(initial=1.0))
            ok = np.isfinite(kr) & np.isfinite(kp)
            assert np.allclose((kp - kr)[ok], 1e-6 - 1.25e-12, rtol=0, atol=1e-15 * np.abs(kp[ok]).max(initial=1.0))
        else:
            assert np.array_equal(post_hi, ref_hi, equal_nan=True) and np.array_equal(kr, kp, equal_nan=True)


def test_generator_reproduces_the_fixture():
    """A handful of cases regenerated (the whole fixture: python oracle/gen_rect_highprec.py, about a minute): a kernel in
    r, the delta kernel, a two-argument kernel without nugget in BJD, a degenerate one and the deep composite."""
    pytest.importorskip('mpmath')
    from oracle import gen_rect_highprec as gen
    meta, d = ff.load_rect()
    names = ['QuasiPeriodic_R5_3', 'WhiteNoise_R2_0', 'Polynomial_R2_0', 'SquaredExponential_R6_0', 'deep7_R1_0']
    got_meta, arrays = gen.generate(set(names))
    assert sorted(m['name'] for m in got_meta) == sorted(names)
    for key in d:
        if key.startswith('t'):
            assert np.array_equal(arrays[key], d[key]), key
    want = {c['name']: c for c in meta['cases']}
    for m in got_meta:
        c = want[m['name']]
        keys = ('expr', 'ops', 'pars', 'nugget', 'n', 'co_n')
        assert json.dumps({k: m[k] for k in keys}) == json.dumps({k: c[k] for k in keys})
        for group, off, n in ((gen.KEYS, 'off', c['n']), (gen.CO_KEYS, 'co_off', c['co_n']), (gen.KSS_KEYS, 'kss_off', 2 * meta['ns'])):
            for key in group:
                got = arrays[key][m[off]:m[off] + n]
                assert got.dtype == d[key].dtype
                assert np.array_equal(got, d[key][c[off]:c[off] + n], equal_nan=True), (m['name'], key)
