"""inference.predict_batch / posterior_predictive and Context.predict_batch without a GPU: the mixture's moments against a
direct NumPy mixture, the one-by-one fallback behind a stand-in context that has no side-by-side form, argument errors."""
import types

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc


class _NoBatchContext:
    """Stands in for _hip.Context: predict_batch has no side-by-side form (None, as for GPRN_E_UNSUPPORTED); predict returns
    rows that depend on the kernels, the state and the times it was given, so that a wrong pairing shows."""
    rank = 0

    def __init__(self, G):
        self.G = G
        self.kernels = {}
        self.batch_calls = 0
        self.predict_calls = 0

    def owner_of(self, gp):
        return 0

    def set_kernel(self, gp, ops, params, add_nugget):
        self.kernels[gp] = np.array(params, dtype=float)

    def set_muvar(self, mu, var):
        self.mu, self.var = np.array(mu, dtype=float), np.array(var, dtype=float)

    def predict_batch(self, *args, **kw):
        self.batch_calls += 1
        return None

    def predict(self, tstar):
        self.predict_calls += 1
        ts = np.asarray(tstar, dtype=float)
        amp = np.array([self.kernels[g][0] for g in range(self.G)])
        mean = amp[:, None] * np.sin(ts[None, :] / 7.0 + np.arange(self.G)[:, None]) + self.mu.mean()
        var = 0.1 + amp[:, None] ** 2 * np.cos(ts[None, :] / 5.0) ** 2 + self.var.mean()
        return mean, var, 0


def _object(p=2, q=2, N=20):
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0, 50, N))
    args = []
    for _ in range(p):
        args += [np.sin(t / 6) + 0.1 * rng.standard_normal(N), np.full(N, 0.2)]
    g = gpyrn.inference(q, t, *args)
    nodes = [covfunc.SquaredExponential(1.0 + 0.1 * j, 10.0) for j in range(q)]
    weights = [covfunc.SquaredExponential(0.8 + 0.05 * k, 20.0) for k in range(q * p)]
    g.set_components(nodes, weights, [meanfunc.Constant(0.1 * i) for i in range(p)], [0.3] * p)
    return g


def _sets_and_states(g, B, seed=0):
    rng = np.random.default_rng(seed)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * rng.uniform(0.9, 1.1, x0.size) for _ in range(B)]
    shape = (B, g.p + 1, g.q, g.N)
    return sets, rng.standard_normal(shape), rng.uniform(0.5, 1.5, shape)


def test_fallback_is_one_prediction_per_vector():
    B = 3
    g = _object()
    g._ctx = fake = _NoBatchContext(g.q * (g.p + 1))
    sets, mu, var = _sets_and_states(g, B)
    tstar = np.linspace(-5, 60, 17)
    mean, pvar, lat = g.predict_batch(sets, tstar=tstar, states=(mu, var), separate=True)
    assert fake.batch_calls == 1 and fake.predict_calls == B
    assert mean.shape == (B, tstar.size, g.p) and pvar.shape == mean.shape and lat.shape == (B, g.q * (g.p + 1), tstar.size)
    np.testing.assert_array_equal(g.get_parameters(), sets[-1])
    for b in range(B):
        g.set_parameters(sets[b])
        m1, v1, parts = g._Prediction(tstar=tstar, mu=mu[b], var=var[b], separate=True)
        assert np.array_equal(mean[b], m1) and np.array_equal(pvar[b], v1)
        assert np.array_equal(lat[b], np.concatenate([np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)]))
    assert not np.array_equal(mean[0], mean[1])
    two = g.predict_batch(sets, tstar=tstar, states=(mu.reshape(B, -1), var.reshape(B, -1)))
    assert len(two) == 2 and np.array_equal(two[0], mean) and np.array_equal(two[1], pvar)


def _with_stand_in(g, mean_b, var_b):
    seen = {}

    def stand_in(self, parameter_sets, tstar=None, states=None, max_iter=None, separate=False):
        seen.update(sets=parameter_sets, tstar=tstar, states=states, max_iter=max_iter, separate=separate)
        return mean_b, var_b
    g.predict_batch = types.MethodType(stand_in, g)
    return seen


@pytest.mark.parametrize('weights', [None, [3.0, 1.0, 0.0, 4.0, 2.0]])
def test_posterior_predictive_is_the_mixture(weights):
    B, ns, p = 5, 11, 2
    rng = np.random.default_rng(1)
    mean_b, var_b = rng.standard_normal((B, ns, p)), rng.uniform(0.1, 2.0, (B, ns, p))
    g = _object(p=p)
    seen = _with_stand_in(g, mean_b, var_b)
    ts = np.linspace(0, 1, ns)
    mean, var = g.posterior_predictive(list(range(B)), tstar=ts, weights=weights, states='s', max_iter=7)
    assert seen['tstar'] is ts and seen['states'] == 's' and seen['max_iter'] == 7 and not seen['separate']
    w = np.full(B, 1.0 / B) if weights is None else np.array(weights) / np.sum(weights)
    # the mixture directly: E[y] and E[y^2] - E[y]^2, component by component
    ref_mean = sum(w[b] * mean_b[b] for b in range(B))
    ref_second = sum(w[b] * (var_b[b] + mean_b[b] ** 2) for b in range(B))
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(var, ref_second - ref_mean ** 2, rtol=1e-12, atol=1e-14)
    assert (var > 0).all()
    if weights is not None:                                  # normalised: the scale of the weights does not matter
        m2, v2 = g.posterior_predictive(list(range(B)), tstar=ts, weights=10.0 * np.array(weights))
        np.testing.assert_allclose(m2, mean, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(v2, var, rtol=1e-12, atol=1e-14)


def test_posterior_predictive_of_one_vector_is_that_row():
    rng = np.random.default_rng(2)
    mean_b, var_b = rng.standard_normal((1, 9, 2)), rng.uniform(0.1, 2.0, (1, 9, 2))
    g = _object()
    _with_stand_in(g, mean_b, var_b)
    mean, var = g.posterior_predictive([0])
    assert np.array_equal(mean, mean_b[0])
    np.testing.assert_allclose(var, var_b[0], rtol=1e-12, atol=1e-14)      # ((v + m^2) - m^2: one rounding of m^2's size)


def test_posterior_predictive_rejects_bad_weights():
    g = _object()
    _with_stand_in(g, np.zeros((3, 4, 2)), np.ones((3, 4, 2)))
    for bad in ([1.0, 2.0], [1.0, -1.0, 1.0], [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError):
            g.posterior_predictive([0, 1, 2], weights=bad)


def test_predict_batch_argument_errors():
    B = 3
    g = _object()
    g._ctx = _NoBatchContext(g.q * (g.p + 1))
    sets, mu, var = _sets_and_states(g, B)
    with pytest.raises(ValueError):
        g.predict_batch([], states=(mu, var))
    with pytest.raises(ValueError):
        g.predict_batch(sets, states=(mu[:2], var[:2]))                    # fewer states than vectors
    with pytest.raises(ValueError):
        g.predict_batch(sets, states=(mu, var[..., :-1]))                  # a state of the wrong length
    with pytest.raises(ValueError):
        g.predict_batch(sets, states=mu)                                   # not a pair
    with pytest.raises(ValueError):
        g.predict_batch(sets, tstar=np.zeros((2, 2)), states=(mu, var))
    assert g._ctx.batch_calls == 0 and g._ctx.predict_calls == 0           # (refused before anything ran)


def test_context_predict_batch_argument_errors():
    """The binding's checks come before the library is touched: an object with the problem's sizes and no handle stands in."""
    ctx = types.SimpleNamespace(p=2, q=1, N=10, G=3, _lib=None, _h=None)
    call = lambda *a, **kw: _hip.Context.predict_batch(ctx, *a, **kw)
    B, d, n_k = 4, 3 * 10, 6
    kp, mu, var, jt, ts = np.ones((B, n_k)), np.zeros((B, d)), np.ones((B, d)), np.ones((B, 2)), np.linspace(0, 1, 5)
    with pytest.raises(ValueError, match='latent pair, the output pair or both'):
        call(kp, mu, var, ts, jitters=jt, latent=False, outputs=False)
    with pytest.raises(ValueError, match='kernel_params'):
        call(np.ones(n_k), mu, var, ts, jitters=jt)
    with pytest.raises(ValueError, match='mu and var'):
        call(kp, mu[:, :-1], var, ts, jitters=jt)
    with pytest.raises(ValueError, match='mu and var'):
        call(kp, mu, var[:2], ts, jitters=jt)
    with pytest.raises(ValueError, match='jitters'):
        call(kp, mu, var, ts)
    with pytest.raises(ValueError, match='jitters'):
        call(kp, mu, var, ts, jitters=np.ones((B, 3)))
    with pytest.raises(ValueError, match='tstar'):
        call(kp, mu, var, [], jitters=jt)
