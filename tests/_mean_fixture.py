"""The high-precision reference of the mean functions (tests/golden/mean_highprec, tests/_gen_mean_fixtures.py) and the one
bound every evaluation of it is held to -- NumPy's own (tests/test_mean_keplerian.py) and the device's
(tests/test_mean_gpu.py) alike:

    |m - m_ref| <= (C0 |m_ref| + C1 kappa) 2^-53,        C0, C1 = 4, 2 (tests/_fill_fixture.py),

kappa = sum_u |u dm/du| over t, the parameters and the formula's rounded intermediates; the derivatives d m / d theta_k are
held to the same bound with their own kappa.  Where the reference is NaN, the evaluation is NaN."""
import json
import os

import numpy as np

from ._fill_fixture import C0, C1, EPS, GOLDEN

_cache = {}


def load():
    """(meta, arrays), read once and shared; the arrays are read-only"""
    if not _cache:
        with open(os.path.join(GOLDEN, 'mean_highprec.json')) as f:
            meta = json.load(f)
        d = np.load(os.path.join(GOLDEN, 'mean_highprec.npz'))
        arrays = {k: d[k] for k in d.files}
        for a in arrays.values():
            a.setflags(write=False)
        _cache['v'] = (meta, arrays)
    return _cache['v']


def build(case):
    from gpyrn_amd import meanfunc
    return eval(case['expr'], {'m': meanfunc, 'nan': float('nan')})


def times(case, d):
    return d['t_' + case['tset']]


def reference(case, d):
    """((hi, lo, kappa) of the value, each (n,); (hi, lo, kappa) of the derivatives, each (npar, n))"""
    s = slice(case['off'], case['off'] + case['n'])
    q = slice(case['doff'], case['doff'] + case['n'] * case['npar'])
    shape = (case['npar'], case['n'])
    return ((d['hi'][s], d['lo'][s].astype(float), d['kappa'][s].astype(float)),
            (d['dhi'][q].reshape(shape), d['dlo'][q].astype(float).reshape(shape), d['dkappa'][q].astype(float).reshape(shape)))


def allowed(ref, c0=C0):
    hi, lo, kappa = ref
    with np.errstate(invalid='ignore'):
        return (c0 * np.abs(hi) + C1 * kappa) * EPS


def violations(values, ref, c0=C0, ratios=None):
    """Indices at which `values` breaks the bound against ref = (hi, lo, kappa); c0 as _fill_fixture.violations' c0.
    ratios: a list that takes the largest error / allowed (finite references with a non-zero allowance only)."""
    hi, lo, kappa = ref
    values = np.asarray(values, dtype=float)
    assert values.shape == hi.shape, (values.shape, hi.shape)
    nan_ref = np.isnan(hi)
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs((values - hi) - lo)
        lim = allowed(ref, c0)
        bad = np.where(nan_ref, ~np.isnan(values), ~(err <= lim))
        if ratios is not None:
            ok = ~nan_ref & (lim > 0) & np.isfinite(values)
            ratios.append(float((err[ok] / lim[ok]).max()) if ok.any() else 0.0)
    return [tuple(int(i) for i in ix) for ix in np.argwhere(bad)]
