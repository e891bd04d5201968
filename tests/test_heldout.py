"""Side-by-side cross-validation (gprn_elbocalc_batch_heldout, Context.elbocalc_batch_heldout, inference.heldout_batch /
cv_folds / cross_validate) without a GPU: the header, the binding and the library agree on the new symbol; the fold masks'
properties for both schemes; the argument checks that need no device; and the NumPy restatement of the held-out score that the
GPU tests compare against, itself against a direct evaluation of the Gaussian log density."""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import stats

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from gpyrn_amd.meanfield import inference
from tests import _heldout_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gprn_hip.h')


# ------------------------------------------------------------------ the symbol
def test_header_binding_and_method_agree_on_the_new_entry_point():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    proto = re.search(r'int\s+gprn_elbocalc_batch_heldout\s*\((.*?)\)\s*;', text, flags=re.S)
    assert proto, 'include/gprn_hip.h does not declare gprn_elbocalc_batch_heldout'
    args = [a.strip() for a in proto.group(1).split(',')]
    restype, argtypes = _hip.SIGNATURES['gprn_elbocalc_batch_heldout']
    assert len(args) == len(argtypes) == 21
    assert args[10].startswith('const uint8_t*') and args[-1].startswith('int*') and args[-2].startswith('double*')
    sig = inspect.signature(_hip.Context.elbocalc_batch_heldout).parameters
    assert list(sig)[1:8] == ['kernel_params', 'y_resid', 'jitters', 'mu', 'var', 'max_iter', 'fit_masks']
    assert sig['forced'].default is False
    for name in ('heldout_batch', 'cv_folds', 'cross_validate'):
        assert callable(getattr(inference, name))


def test_mask_lane_keeps_its_size():
    """The lane's row number lives in what was padding: tests/test_draw_batch_gpu.py restates sizeof(MaskLane) = 72."""
    src = open(os.path.join(ROOT, 'gpyrn_amd', 'csrc', 'batch_layout.h')).read()
    body = src[src.index('struct MaskLane {'):]
    body = body[:body.index('};')]
    assert len(re.findall(r'\*\s*\w+', body.split('int gp;')[0])) == 8       # eight pointers, then two ints: 64 + 8
    assert 'int gp;' in body and 'int row;' in body
    assert 'static_assert(sizeof(MaskLane) == 72' in src


# ------------------------------------------------------------------ cv_folds
def _object(p=3, q=2, N=40, mask=None, seed=0, **kw):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.uniform(0.0, 100.0, N))
    args = [a for _ in range(p) for a in (rng.normal(size=N), np.full(N, 0.1))]
    g = gpyrn.inference(q, t, *args, mask=mask, **kw)
    g.set_components([covfunc.SquaredExponential(1.0, 20.0) for _ in range(q)],
                     [covfunc.SquaredExponential(1.0, 60.0) for _ in range(q * p)],
                     [meanfunc.Constant(0.0) for _ in range(p)], [0.1] * p)
    return g


def _rules_hold(fit, D, q):
    assert not np.any(fit & ~D)
    assert fit.any(axis=1).all()
    if q >= 2:
        assert fit.any(axis=0)[D.any(axis=0)].all()


@pytest.mark.parametrize('scheme,kw', [('entries', {}), ('blocks', dict(block=4)), ('blocks', {})])
@pytest.mark.parametrize('p,q,k', [(3, 2, 4), (2, 1, 5), (1, 1, 3), (3, 2, 3)])
def test_cv_folds_hold_every_observed_entry_out_exactly_once(scheme, kw, p, q, k):
    g = _object(p=p, q=q, N=41)
    folds = g.cv_folds(k, scheme=scheme, rng=3, **kw)
    assert folds.shape == (k, p, 41) and folds.dtype == bool
    D = np.ones((p, 41), dtype=bool)
    for f in range(k):
        _rules_hold(np.asarray(folds[f]), D, q)
    times_held = (~np.asarray(folds)).sum(axis=0)
    assert folds.n_never_held == 0 and np.all(times_held == 1)
    if scheme == 'entries' and p <= k:                        # two outputs of one time never share a fold
        assert ((~np.asarray(folds)).sum(axis=1) <= 1).all()
    if scheme == 'blocks' and kw:                             # whole runs of `block` times go together
        held0 = ~np.asarray(folds)[:, 0, :]                   # (k, N) of output 0
        which = held0.argmax(axis=0)
        assert all(len(set(which[s:s + 4])) == 1 for s in range(0, 40, 4))
    again = g.cv_folds(k, scheme=scheme, rng=3, **kw)
    other = g.cv_folds(k, scheme=scheme, rng=4, **kw)
    assert np.array_equal(folds, again)
    assert not np.array_equal(folds, other) or scheme == 'blocks'
    assert np.array_equal(folds, g.cv_folds(k, scheme=scheme, rng=np.random.RandomState(3), **kw))


def test_cv_folds_under_a_from_series_mask_count_what_no_fold_can_hold():
    rng = np.random.RandomState(0)
    t1 = np.sort(rng.uniform(0.0, 100.0, 34))
    t2 = np.sort(rng.uniform(0.0, 100.0, 28))
    shared = t1[::5]
    t2 = np.unique(np.concatenate([t2, shared]))
    series = [(t1, rng.normal(size=t1.size), np.full(t1.size, 0.1)), (t2, rng.normal(size=t2.size), np.full(t2.size, 0.1))]
    for q in (1, 2):
        g = gpyrn.inference.from_series(q, series)
        D = np.asarray(g.mask)
        for scheme in ('entries', 'blocks'):
            folds = np.asarray(g.cv_folds(4, scheme=scheme, rng=1))
            never = g.cv_folds(4, scheme=scheme, rng=1).n_never_held
            for f in range(4):
                _rules_hold(folds[f], D, q)
            times_held = (D[None] & ~folds).sum(axis=0)
            assert np.all(times_held[~D] == 0) and np.all(times_held <= 1)
            assert never == int((D & (times_held == 0)).sum())
            if q == 1:
                assert never == 0
            elif scheme == 'entries':
                # with q = 2 a time with ONE observed output can never lose it; the shared times lose one output per fold
                alone = D.sum(axis=0) == 1
                assert never == int(alone.sum()) and np.all(times_held[:, ~alone][D[:, ~alone]] == 1)


def test_cv_folds_refuse_what_has_no_valid_split():
    with pytest.raises(ValueError, match='k >= 2'):
        _object().cv_folds(1)
    with pytest.raises(ValueError, match='p = 1'):
        _object(p=1, q=2).cv_folds(3)
    with pytest.raises(ValueError, match='scheme'):
        _object().cv_folds(3, scheme='times')
    with pytest.raises(ValueError, match='block'):
        _object().cv_folds(3, scheme='blocks', block=0)


# ------------------------------------------------------------------ argument checks that need no device
def test_heldout_batch_checks_its_masks_before_any_device():
    g = _object(p=3, q=2, N=40)
    x = g.get_parameters()
    ok = np.ones((1, 3, 40), dtype=bool)
    with pytest.raises(ValueError, match='shape'):
        g.heldout_batch([x], ok[:, :2])
    with pytest.raises(ValueError, match='shape'):
        g.heldout_batch([x, x], ok)
    bad = ok.copy(); bad[0, 1] = False
    with pytest.raises(ValueError, match=r'fit mask 0 leaves output\(s\) \[1\]'):
        g.heldout_batch([x], bad)
    bad = ok.copy(); bad[0, :, 7] = False
    with pytest.raises(ValueError, match=r'fit mask 0 leaves time index\(es\) \[7\]'):
        g.heldout_batch([x], bad)
    with pytest.raises(ValueError, match='committed sweep'):
        g.heldout_batch([x], ok, sweeps=0)
    with pytest.raises(ValueError, match='start'):
        g.heldout_batch([x], ok, start=(np.zeros(3), np.zeros(3)))
    with pytest.raises(ValueError, match='no parameter vector'):
        g.heldout_batch([], np.ones((0, 3, 40), dtype=bool))
    D = np.ones((3, 40), dtype=bool); D[0, :5] = False
    gm = _object(p=3, q=2, N=40, mask=D)
    with pytest.raises(ValueError, match='fit mask 1 fits an entry the data mask does not hold'):
        gm.heldout_batch([x, x], np.array([D, np.ones((3, 40), dtype=bool)]))
    with pytest.raises(ValueError, match='folds must have shape'):
        g.cross_validate(np.ones((2, 3, 39), dtype=bool))


def test_heldout_batch_names_why_the_side_by_side_form_does_not_apply():
    g = _object(p=2, q=1, N=40)
    x = g.get_parameters()
    ok = np.ones((1, 2, 40), dtype=bool); ok[0, 0, 3] = False
    gs = _object(p=2, q=1, N=40, sweep_order='sequential')
    with pytest.raises(NotImplementedError, match='sequential'):
        gs.heldout_batch([x], ok)
    g.batch_max_N = 39
    with pytest.raises(NotImplementedError, match='batch_max_N'):
        g.heldout_batch([x], ok)
    del g.batch_max_N

    class Mine(covfunc.covFunction):
        def __init__(self, a):
            super().__init__(a)

        def __call__(self, r):
            return self.pars[0] ** 2 * np.exp(-np.abs(r))

    gu = _object(p=2, q=1, N=40)
    gu.set_components([Mine(1.0)], [covfunc.SquaredExponential(1.0, 60.0), covfunc.SquaredExponential(0.7, 60.0)],
                      [meanfunc.Constant(0.0), meanfunc.Constant(0.0)], [0.1, 0.1])
    with pytest.raises(NotImplementedError, match='device program'):
        gu.heldout_batch([gu.get_parameters()], ok)
    g._comm = object()
    with pytest.raises(NotImplementedError, match='sharded'):
        g.heldout_batch([x], ok)


# ------------------------------------------------------------------ the restatement the GPU tests use
def test_the_restatement_is_the_gaussian_log_density():
    rng = np.random.RandomState(5)
    p, q, N = 3, 2, 17
    mu, var = rng.normal(size=(p + 1, q, N)), rng.uniform(0.05, 0.5, size=(p + 1, q, N))
    y = rng.normal(size=(p, N))
    jitt2, yerr2 = rng.uniform(0.01, 0.1, p), rng.uniform(0.01, 0.1, (p, N))
    held = rng.uniform(size=(p, N)) < 0.3
    y_g, e_g = np.where(held, y, np.nan), np.where(held, yerr2, np.inf)       # garbage outside: never read
    m, v, lpd, n = H.score(mu, var, y_g, jitt2, e_g, held)
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(v)) and np.all(np.isfinite(lpd))
    assert n.tolist() == held.sum(axis=1).tolist()
    for i in range(p):
        direct = 0.0
        for t in np.flatnonzero(held[i]):
            mean = sum(mu[0, j, t] * mu[1 + i, j, t] for j in range(q))
            vv = sum(mu[1 + i, j, t] ** 2 * var[0, j, t] + var[1 + i, j, t] * (var[0, j, t] + mu[0, j, t] ** 2) for j in range(q))
            vv += jitt2[i] + yerr2[i, t]
            assert m[i, t] == pytest.approx(mean, rel=1e-14) and v[i, t] == pytest.approx(vv, rel=1e-14)
            direct += stats.norm.logpdf(y[i, t], loc=mean, scale=np.sqrt(vv))
        assert lpd[i] == pytest.approx(direct, rel=1e-12)
    assert np.all(m[~held] == 0) and np.all(v[~held] == 0)
    # Monte Carlo: v is the variance of sum_j f_j w_ij + noise under the mean-field posterior
    i, t = np.argwhere(held)[0]
    f = mu[0, :, t] + np.sqrt(var[0, :, t]) * rng.normal(size=(400000, q))
    w = mu[1 + i, :, t] + np.sqrt(var[1 + i, :, t]) * rng.normal(size=(400000, q))
    draws = (f * w).sum(axis=1) + np.sqrt(jitt2[i] + yerr2[i, t]) * rng.normal(size=400000)
    assert draws.mean() == pytest.approx(m[i, t], abs=5 * np.sqrt(v[i, t] / 400000))
    assert draws.var() == pytest.approx(v[i, t], rel=0.02)
