"""The high-precision reference of the covariance fill (tests/golden/fill_highprec, oracle/gen_fill_highprec.py) and the
one bound every evaluation of it is held to -- the device's fill (tests/test_fill_gpu.py) and NumPy's own evaluation of
gpyrn_amd.covfunc (tests/test_fill_highprec.py) alike:

    |K - K_ref| <= (C0 + C1 kappa) 2^-53 |K_ref| + A_DENORM max(1, max |K_ref|),

kappa the element's condition number over r (or t_i, t_j) and the parameters.  Where the reference is NaN, K is NaN."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C0, C1 = 4.0, 2.0
EPS = 2.0 ** -53
# the denormal tail: an exponential that underflows keeps only the bits above 2^-1074, which a prefactor of the formula
# (Matern's polynomial, the derivative kernels' 1 / ell^4) then scales up -- 2^24 subnormal ulps, times theta^2
A_DENORM = 2.0 ** -1050


def load():
    with open(os.path.join(GOLDEN, 'fill_highprec.json')) as f:
        meta = json.load(f)
    d = np.load(os.path.join(GOLDEN, 'fill_highprec.npz'))
    return meta['cases'], {k: d[k] for k in d.files}


def case_arrays(case, d, seq=False):
    """(i, j, hi, lo, kappa) of one case; with `seq`, the reference that holds NumPy's rounded intermediates."""
    s = slice(case['off'], case['off'] + case['n'])
    i, j = d['i'][s].astype(np.int64), d['j'][s].astype(np.int64)
    if seq:
        q = slice(case['seq_off'], case['seq_off'] + case['n'])
        return i, j, d['seq_hi'][q], d['seq_lo'][q].astype(float), d['seq_kappa'][q].astype(float)
    return i, j, d['hi'][s], d['lo'][s].astype(float), d['kappa'][s].astype(float)


def violations(K, case, d, seq=False):
    """Elements of the sample where the matrix K breaks the bound: a list of (i, j, K, K_ref, allowed) tuples."""
    i, j, hi, lo, kappa = case_arrays(case, d, seq)
    k = K[i, j]
    nan_ref = np.isnan(hi)
    with np.errstate(invalid='ignore', over='ignore'):
        scale = max(1.0, float(np.nanmax(np.abs(hi))) if not nan_ref.all() else 1.0)
        err = np.abs((k - hi) - lo)
        allowed = np.where(hi == 0, 0.0, (C0 + C1 * kappa) * EPS * np.abs(hi)) + A_DENORM * scale
        bad = np.where(nan_ref, ~np.isnan(k), ~(err <= allowed))
        inf_ref = np.isinf(hi)
        bad = np.where(inf_ref, k != hi, bad)
    return [(int(a), int(b), float(x), float(y), float(z)) for a, b, x, y, z in
            zip(i[bad], j[bad], k[bad], hi[bad], allowed[bad])]


def numpy_matrix(case, t):
    """NumPy's own evaluation of the case's kernel (gpyrn_amd.covfunc.__call__) at the fixture's times, no nugget."""
    from gpyrn_amd import covfunc
    k = eval(case['expr'], {'c': covfunc, 'nan': float('nan')})
    with np.errstate(all='ignore'):
        if isinstance(k, (covfunc.Polynomial, covfunc.HarmonicPeriodic, covfunc.QuasiHarmonicPeriodic)):
            return np.asarray(k(t[:, None], t[None, :]), dtype=float)
        return np.asarray(k(t[:, None] - t[None, :]), dtype=float)
