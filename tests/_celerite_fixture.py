"""tests/golden/celerite_highprec (tests/_gen_celerite_fixtures.py) as the functions of tests/_fill_fixture.py take it: the
square sample goes to `violations` as it stands, the rectangular one through `rect_views` after its prefix is dropped; the
derivatives are held norm-wise to tests/_dk_cases.DK_TOL."""
import json
import os

import numpy as np

from tests import _fill_fixture as ff

DK_TOL = 2e-11                 # tests/_dk_cases.DK_TOL (asserted equal in tests/test_celerite.py)


def load():
    """(meta, square arrays, rectangular arrays)"""
    with open(os.path.join(ff.GOLDEN, 'celerite_highprec.json')) as f:
        meta = json.load(f)
    d = np.load(os.path.join(ff.GOLDEN, 'celerite_highprec.npz'))
    sq = {k: d[k] for k in d.files if not k.startswith('rect_')}
    rect = {k[5:]: d[k] for k in d.files if k.startswith('rect_')}
    return meta, sq, rect


def has_nan(case):
    return any(v != v for v in case['pars'])


def kernel_of(case):
    from gpyrn_amd import covfunc
    return eval(case['expr'], {'c': covfunc, 'nan': float('nan')})


def dk_reference(case, d):
    """(n_par, n) derivatives of the case at its square sample, or None for a case without the record: a NaN parameter, or
    one of the three 1e6-radian cases dropped from the derivative bound (tests/_gen_celerite_fixtures.py)"""
    if case['dk_off'] is None:
        return None
    npar = len(case['pars'])
    return d['dk'][case['dk_off']:case['dk_off'] + npar * case['n']].reshape(npar, case['n'])


def dk_worst(dK, case, d, skip=()):
    """max over the parameters (but those in `skip`) of max |dK - ref| / max |ref| at the sample (dK: (n_par, N, N)); inf
    where a reference that is 0 throughout meets anything else"""
    ref = dk_reference(case, d)
    i, j = d['i'][case['off']:case['off'] + case['n']].astype(int), d['j'][case['off']:case['off'] + case['n']].astype(int)
    w = 0.0
    for l in range(ref.shape[0]):
        if l in skip:
            continue
        err, scale = float(np.abs(dK[l][i, j] - ref[l]).max()), float(np.abs(ref[l]).max())
        if not np.isfinite(err):
            return np.inf
        w = max(w, err / scale if scale > 0 else (0.0 if err == 0 else np.inf))
    return w


def rect_case(case):
    """the case as `_fill_fixture.rect_views` and `rect_nugget` read it"""
    return dict(case['rect'], nugget=case['nugget'], name=case['name'])


def numpy_dk(case, t):
    """NumPy's closed forms (covFunction._dk_dpars) on the full grid of the case's time set: (n_par, N, N)"""
    k = kernel_of(case)
    r = t[:, None] - t[None, :]
    with np.errstate(all='ignore'):
        return np.array([np.broadcast_to(np.asarray(x, dtype=float), r.shape) for x in k._dk_dpars(r)])
