"""Data masks without a GPU: the dense restatement against the reference's fixtures, validation before any device
call, from_series, _initMuVar on a masked y and the C ABI's new entry point."""
import os
import re

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip
from oracle import cpu_ref
from tests import _cases, _mask_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('tag', ['step_p1q1', 'step_p2q1', 'step_p3q2', 'step_p2q3', 'cfg1_N200'])
def test_dense_restatement_with_an_all_true_mask_is_the_reference(tag):
    pr = R.problem(tag)
    d, meta = pr['d'], pr['meta']
    mask = np.ones(pr['y_raw'].shape, dtype=bool)
    E, P, mu, var = R.sweeps(pr['Kf'], pr['Kw'], pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2'],
                             d['mu_init'], d['var_init'], mask, meta['nsweeps'])
    np.testing.assert_allclose(E, d['elbo_sweeps'], rtol=1e-9)
    np.testing.assert_allclose(P, d['parts_sweeps'], rtol=1e-9)
    _cases.assert_state('mask ref ' + tag, mu, d['mu_final'], var, d['var_final'])


@pytest.mark.parametrize('tag', ['step_p1q1', 'step_p2q1', 'cfg1_N200'])
def test_dense_restatement_with_inserted_all_masked_times(tag):
    pr, mask, pos = R.inserted(tag)
    d, meta = pr['d'], pr['meta']
    mu0, var0 = R.init_state(pr, mask)
    E, P, mu, var = R.sweeps(pr['Kf'], pr['Kw'], pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2'],
                             mu0, var0, mask, meta['nsweeps'])
    np.testing.assert_allclose(E, d['elbo_sweeps'], rtol=1e-9)
    np.testing.assert_allclose(P[:, 0], d['parts_sweeps'][:, 0], rtol=1e-9)
    np.testing.assert_allclose(P[:, 1] + P[:, 2], d['parts_sweeps'][:, 1] + d['parts_sweeps'][:, 2], rtol=1e-9)
    shape = (meta['p'] + 1, meta['q'], mask.shape[1])
    _cases.assert_state('mask ref inserted ' + tag, mu.reshape(shape)[..., pos], d['mu_final'],
                        var.reshape(shape)[..., pos], d['var_final'])


def _data(p=2, N=10, seed=0):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(N)) * 10
    return t, rng.randn(p, N), rng.rand(p, N) + 0.1


def _args(y, e):
    return [a for i in range(y.shape[0]) for a in (y[i], e[i])]


def test_validation_raises_before_any_device_call():
    t, y, e = _data()
    with pytest.raises(ValueError, match='shape'):
        gpyrn.inference(1, t, *_args(y, e), mask=np.ones((2, 9), dtype=bool))
    m = np.ones((2, 10), dtype=bool)
    m[1] = False
    with pytest.raises(ValueError, match='no observed entry'):
        gpyrn.inference(1, t, *_args(y, e), mask=m)
    m = np.ones((2, 10), dtype=bool)
    m[:, 4] = False
    with pytest.raises(ValueError, match='drop'):
        gpyrn.inference(2, t, *_args(y, e), mask=m)
    g = gpyrn.inference(1, t, *_args(y, e), mask=m)        # q = 1: allowed
    assert g.mask.dtype == bool and g._ctx is None
    assert gpyrn.inference(1, t, *_args(y, e)).mask is None


def test_masked_entries_never_reach_the_data():
    t, y, e = _data()
    m = np.ones((2, 10), dtype=bool)
    m[0, 3] = m[1, 7] = False
    y2, e2 = y.copy(), e.copy()
    y2[0, 3], e2[1, 7] = np.nan, np.inf
    g = gpyrn.inference(1, t, *_args(y2, e2), mask=m)
    assert np.all(np.isfinite(g.y)) and np.all(np.isfinite(g.yerr))
    assert g.y[0, 3] == 0 and g.yerr[1, 7] == 1


def test_init_mu_var_reads_a_masked_y_as_zero():
    t, y, e = _data(p=3, N=12, seed=3)
    m = R.partial_mask(3, 12, seed=1)
    g = gpyrn.inference(2, t, *_args(np.where(m, y, np.nan), e), mask=m)
    nodes = [gpyrn.SquaredExponential(1.3, 2.0), gpyrn.SquaredExponential(0.7, 3.0)]
    weights = [gpyrn.SquaredExponential(0.5 + 0.1 * k, 4.0) for k in range(6)]
    mu, var = g._initMuVar(nodes, weights, [0.1, 0.2, 0.3])
    mu_r, var_r = cpu_ref.init_mu_var(np.where(m, y, 0.0), [1.3, 0.7], [w.pars[0] for w in weights], [0.1, 0.2, 0.3])
    np.testing.assert_array_equal(mu, mu_r)
    np.testing.assert_array_equal(var, var_r)


def test_from_series_builds_the_union_grid_and_the_mask():
    t1, t2, t3 = np.array([3.0, 1.0, 2.0]), np.array([2.0, 5.0]), np.array([0.5, 5.0, 1.0])
    s = [(t1, t1 * 10, t1 + 0.1), (t2, t2 * 20, t2 + 0.2), (t3, t3 * 30, t3 + 0.3)]
    g = gpyrn.inference.from_series(1, s)
    np.testing.assert_array_equal(g.time, [0.5, 1.0, 2.0, 3.0, 5.0])
    assert g.p == 3 and g.N == 5
    np.testing.assert_array_equal(g.mask, [[0, 1, 1, 1, 0], [0, 0, 1, 0, 1], [1, 1, 0, 0, 1]])
    for i, (t, y, e) in enumerate(s):
        idx = np.searchsorted(g.time, t)
        np.testing.assert_array_equal(g.y[i, idx], y)
        np.testing.assert_array_equal(g.yerr[i, idx], e)
    assert np.all(g.y[~g.mask] == 0) and np.all(g.yerr[~g.mask] == 1)
    g2 = gpyrn.inference.from_series(2, s)             # every time of the union is observed by some series: q = 2 is fine
    assert g2.q == 2 and g2.mask.any(axis=0).all()
    with pytest.raises(ValueError):
        gpyrn.inference.from_series(1, [(np.array([1.0, 1.0]), np.ones(2), np.ones(2))])   # a repeated time in one series


def test_refusals_do_not_need_a_device():
    t, y, e = _data()
    m = np.ones((2, 10), dtype=bool)
    m[0, 2] = False
    g = gpyrn.inference(1, t, *_args(y, e), mask=m)
    g.set_components(gpyrn.SquaredExponential(1, 1), [gpyrn.SquaredExponential(1, 1)] * 2, [gpyrn.Constant(0), gpyrn.Constant(0)], [0.1, 0.1])
    assert not g._batchable()
    for call in (lambda: g.grad_ELBO(), lambda: g.nELBO_and_grad(g.get_parameters()),
                 lambda: g.optimize(jac=True), lambda: g.ELBOaux(*[None] * 8),
                 lambda: g._updateSigMu(*[None] * 10), lambda: g._entropy(None, None),
                 lambda: g._expectedLogPrior(*[None] * 8), lambda: g._expectedLogLike(*[None] * 6)):
        with pytest.raises(NotImplementedError):
            call()

    class FakeComm:
        world, rank, local_rank = 2, 0, 0
    with pytest.raises(NotImplementedError):
        gpyrn.inference(1, t, *_args(y, e), mask=m, comm=FakeComm())


def test_set_mask_is_in_the_header_and_the_binding():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gprn_hip.h')).read(), flags=re.S)
    assert re.search(r'int\s+gprn_set_mask\s*\(\s*gprn_ctx\*\s*\w+\s*,\s*const\s+uint8_t\*\s*\w+\s*\)', text)
    assert 'gprn_set_mask' in _hip.SIGNATURES
    if os.path.exists(_hip.LIB_PATH):
        assert hasattr(_hip.load_library(), 'gprn_set_mask')
