"""Joint posterior draws for many vectors side by side (gprn_elbocalc_batch_draws, Context.elbocalc_batch_draws, inference.
sample_posterior_batch, posterior_predictive(draws=k)) without a GPU: the header and the binding agree on the new entry, the
argument checks come before anything touches the device, the one-by-one fallback behind a stand-in context consumes the same
normals, the restatement tests/_draw_batch_ref.py is consistent with itself -- chol(C* + nu I) reproduces C* -- and its own
draws under the GPU test's seed stay inside that test's bound."""
import ctypes
import inspect
import types

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip
from tests import _draw_batch_ref as D, _mask_ref as M, _varpred_ref as V
from tests.test_varpred_batch import _CTYPES, _OneByOneContext, _object, _prototype

SEED = 20240917     # tests/test_draw_batch_gpu.py's test 8


def test_header_declares_the_entry_and_the_binding_matches():
    args = _prototype('gprn_elbocalc_batch_draws')
    assert [a[1] for a in args] == ['ctx', 'n_eval', 'kernel_params', 'n_kernel_params', 'y_resid', 'jitters', 'mu', 'var',
                                    'max_iter', 'flags', 'ns', 'tstar', 'n_draws', 'z', 'elbo', 'iterations', 'converged', 'info',
                                    'mu_out', 'var_out', 'lat_draws', 'out_draws', 'nugget_out', 'draw_info']
    restype, argtypes = _hip.SIGNATURES['gprn_elbocalc_batch_draws']
    assert restype is ctypes.c_int
    assert argtypes == [_CTYPES[typ] for typ, _ in args]
    # it is gprn_elbocalc_batch_predict with the draws' arguments in place of the four prediction rows
    pred = _prototype('gprn_elbocalc_batch_predict')
    mine = ('n_draws', 'z', 'lat_draws', 'out_draws', 'nugget_out', 'draw_info')
    assert [a for a in args if a[1] not in mine] == [a for a in pred if a[1] not in ('lat_mean', 'lat_var', 'out_mean', 'out_var')]


def test_python_keywords():
    sig = inspect.signature(_hip.Context.elbocalc_batch_draws).parameters
    assert list(sig)[1:] == ['kernel_params', 'y_resid', 'jitters', 'mu', 'var', 'max_iter', 'tstar', 'z', 'forced', 'latent',
                             'outputs']
    assert sig['forced'].default is False and sig['latent'].default is True and sig['outputs'].default is True
    sig = inspect.signature(gpyrn.inference.sample_posterior_batch).parameters
    assert list(sig)[1:] == ['parameter_sets', 'tstar', 'n', 'noise', 'separate', 'rng', 'max_iter', 'sweeps', 'start']
    assert sig['n'].default == 1 and sig['noise'].default is False and sig['separate'].default is False
    assert all(sig[k].default is None for k in ('tstar', 'rng', 'max_iter', 'sweeps', 'start'))
    assert inspect.signature(gpyrn.inference.posterior_predictive).parameters['draws'].default is None


def test_argument_checks_come_before_the_device():
    g = _object()                                             # the reference form
    x = np.array(g.get_parameters(), dtype=float)
    state = (np.zeros((g.p + 1, g.q, g.N)), np.ones((g.p + 1, g.q, g.N)))
    with pytest.raises(ValueError, match="predict='variational'"):
        g.sample_posterior_batch([x, x])
    with pytest.raises(ValueError, match="predict='variational'"):
        g.posterior_predictive([x, x], draws=2)
    assert g._ctx is None
    g = _object(predict='variational')
    with pytest.raises(ValueError, match='start'):            # a start state belongs to the forced sweeps
        g.sample_posterior_batch([x, x], start=state)
    with pytest.raises(ValueError):
        g.sample_posterior_batch([x, x], sweeps=0, start=state)
    with pytest.raises(ValueError):
        g.sample_posterior_batch([x, x], max_iter=0)
    with pytest.raises(ValueError, match='n >= 1'):
        g.sample_posterior_batch([x, x], n=0)
    with pytest.raises(ValueError):
        g.sample_posterior_batch([])
    with pytest.raises(ValueError, match='tstar'):
        g.sample_posterior_batch([x, x], tstar=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='resample the chain'):
        g.posterior_predictive([x, x], draws=2, weights=[1.0, 3.0])
    with pytest.raises(ValueError, match='draws >= 1'):
        g.posterior_predictive([x, x], draws=0)
    with pytest.raises(ValueError, match='go with `draws`'):
        g.posterior_predictive([x, x], from_sweeps=True, noise=True)
    assert np.array_equal(g.get_parameters(), x)
    assert g._ctx is None
    g._comm = object()                                        # (what a sharded object holds: any communicator)
    with pytest.raises(NotImplementedError, match='sharded'):
        g.sample_posterior_batch([x, x])
    with pytest.raises(NotImplementedError, match='sharded'):
        g.posterior_predictive([x, x], draws=2, sweeps=2)
    assert g._ctx is None


class _DrawContext(_OneByOneContext):
    """... whose predict_draws returns rows that depend on the kernels, the state the loop left, the times and the normals."""
    def elbocalc_batch_draws(self, *a, **kw):
        self.calls.append('batch')
        return None

    def predict_draws(self, tstar, z, outputs=True):
        assert self.form == _hip.PREDICT_POSTERIOR
        self.calls.append('draws')
        ts = np.asarray(tstar, dtype=float)
        amp = np.array([self.kernels[g][0] for g in range(self.G)])
        lat = amp[:, None, None] * np.sin(ts[None, None, :] / 7.0) + self.mu.mean() + 0.5 * z
        p = self.shape[0] - 1
        q = self.G // (p + 1)
        out = np.array([sum(lat[q + j * p + i] * lat[j] for j in range(q)) for i in range(p)])
        return lat, out, np.full(self.G, 1.25e-12), 0


@pytest.mark.parametrize('forced', [True, False])
def test_one_by_one_fallback_consumes_the_same_normals(forced):
    B, n = 3, 2
    g = _object(predict='variational')
    g.batch_max_N = 0                                         # (N above batch_max_N: the side-by-side form does not apply)
    g._ctx = fake = _DrawContext(g)
    g._predict_sent = 'reference'
    rng = np.random.default_rng(0)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * rng.uniform(0.9, 1.1, x0.size) for _ in range(B)]
    tstar = np.linspace(-5, 60, 17)
    shape = (g.p + 1, g.q, g.N)
    start = (rng.standard_normal(shape), rng.uniform(0.5, 1.5, shape))
    if forced:
        kw = dict(sweeps=2, start=start)
    else:
        g._mu, g._var = start
        kw = dict(max_iter=30)
    G = g.q * (g.p + 1)
    draws, lat = g.sample_posterior_batch(sets, tstar=tstar, n=n, noise=True, separate=True, rng=9, **kw)
    loops = [c for c in fake.calls if isinstance(c, tuple)]
    assert loops == [('sweep', 2) if forced else ('elbocalc', 30)] * B
    assert fake.calls.count('draws') == B and 'batch' not in fake.calls
    assert draws.shape == (B, n, tstar.size, g.p) and lat.shape == (B, G, n, tstar.size)
    assert g.last_nuggets.shape == (B, G) and g.last_info == 0
    np.testing.assert_array_equal(g.get_parameters(), sets[-1])
    # the normals (B, G, n, N*) up front, the noise behind them from the same generator; the means and jitters per vector
    gen = np.random.default_rng(9)
    z = gen.standard_normal((B, G, n, tstar.size))
    eps = gen.standard_normal((B, n, tstar.size, g.p))
    state = start
    for b in range(B):
        g.set_parameters(sets[b])
        nodes, weights, means, jitters = g._get_components()
        ctx = g._setup_device(nodes, weights, means, jitters)
        ctx.option('predict_form', _hip.PREDICT_POSTERIOR)
        ctx.set_muvar(*state)
        if forced:
            ctx.sweep(2, commit=True)
        else:
            ctx.elbocalc(30)
        l_, o_, _, _ = ctx.predict_draws(tstar, z[b])
        assert np.array_equal(lat[b], l_)
        mv = np.array(np.array_split(g._mean(means, tstar), g.p))
        expect = np.transpose(o_, (1, 2, 0)) + mv.T[None] + eps[b] * np.abs(np.asarray(jitters, dtype=float))
        np.testing.assert_allclose(draws[b], expect, rtol=1e-14, atol=1e-14)
    assert not np.array_equal(draws[0], draws[1])


def test_posterior_predictive_with_draws_returns_k_curves_per_vector():
    B, ns, p, k = 4, 9, 2, 3
    rng = np.random.default_rng(1)
    mean_b, var_b = rng.standard_normal((B, ns, p)), rng.uniform(0.1, 2.0, (B, ns, p))
    curves_b = rng.standard_normal((B, k, ns, p))
    g = _object(p=p, predict='variational')
    seen, seen_d = {}, {}

    def stand_in(self, parameter_sets, tstar=None, **kw):
        seen.update(kw, tstar=tstar)
        return mean_b, var_b

    def stand_in_draws(self, parameter_sets, tstar=None, **kw):
        seen_d.update(kw, tstar=tstar)
        return curves_b
    g.predict_batch = types.MethodType(stand_in, g)
    g.sample_posterior_batch = types.MethodType(stand_in_draws, g)
    ts = np.linspace(0, 1, ns)
    mean, var, curves = g.posterior_predictive(list(range(B)), tstar=ts, draws=k, rng=4, noise=True, sweeps=3, start='s')
    assert seen == dict(from_sweeps=True, sweeps=3, start='s', tstar=ts)
    assert seen_d == dict(n=k, max_iter=None, sweeps=3, start='s', rng=4, noise=True, tstar=ts)
    assert curves.shape == (B * k, ns, p)
    assert np.array_equal(curves[k:2 * k], curves_b[1])       # (k per vector, vector-major)
    np.testing.assert_allclose(mean, mean_b.mean(axis=0), rtol=1e-14, atol=1e-15)
    assert len(g.posterior_predictive(list(range(B)), tstar=ts, from_sweeps=True)) == 2      # (without `draws`: unchanged)
    assert g._ctx is None


def test_binding_shape_checks_come_before_the_library():
    ctx = types.SimpleNamespace(p=2, q=1, N=10, G=3, _lib=None, _h=None)
    call = lambda *a, **kw: _hip.Context.elbocalc_batch_draws(ctx, *a, **kw)
    B, d, n_k = 4, 3 * 10, 6
    kp, yr, jt = np.ones((B, n_k)), np.zeros((B, 2, 10)), np.ones((B, 2))
    mu, var, ts = np.zeros((B, d)), np.ones((B, d)), np.linspace(0, 1, 5)
    z = np.zeros((B, 3, 2, 5))
    with pytest.raises(ValueError, match='latent draws, the output draws or both'):
        call(kp, yr, jt, mu, var, 3, ts, z, latent=False, outputs=False)
    with pytest.raises(ValueError, match='kernel_params'):
        call(np.ones(n_k), yr, jt, mu, var, 3, ts, z)
    with pytest.raises(ValueError, match='y_resid'):
        call(kp, yr[:, :1], jt, mu, var, 3, ts, z)
    with pytest.raises(ValueError, match='jitters'):
        call(kp, yr, jt[:, :1], mu, var, 3, ts, z)
    with pytest.raises(ValueError, match='mu and var'):
        call(kp, yr, jt, mu[:, :-1], var, 3, ts, z)
    with pytest.raises(ValueError, match='tstar is empty'):
        call(kp, yr, jt, mu, var, 3, np.zeros(0), z)
    for bad in (z[0], z[:, :2], z[:, :, :0], z[..., :4]):
        with pytest.raises(ValueError, match='z must be'):
            call(kp, yr, jt, mu, var, 3, ts, bad)
    with pytest.raises(ValueError, match='committed sweep'):
        call(kp, yr, jt, mu, var, 0, ts, z)


# ------------------------------------------------------------------ the restatement
def _case_a():
    pr = V.synthetic(45, 2, 2, seed=1, composite=True)
    mask = M.partial_mask(2, 45, 2)
    mu0, var0 = (np.asarray(a, dtype=float) for a in V.init_state(pr, mask))
    return pr, mask, mu0, var0


def test_the_restatement_is_consistent_with_itself():
    """chol(C* + nu I) reproduces C*; its draws are mean* + L z; the outputs' draws are sum_j w o f of the latent draws; at
    duplicated times C* is singular and the ladder still ends inside its range."""
    pr, mask, mu0, var0 = _case_a()
    comp = (pr['nodes'], pr['weights'], pr['means'], pr['jitters'])
    p, q = 2, 2
    for ts in (V.mixed_times(pr['time'], 129, seed=129), np.repeat(V.mixed_times(pr['time'], 43, seed=43), 3)):
        lat_mean, lat_cov, mu, var = D.posterior(pr, mask, 'reference', mu0, var0, comp, ts)
        assert lat_mean.shape == (6, ts.size) and lat_cov.shape == (6, ts.size, ts.size)
        z = np.random.default_rng(1).standard_normal((6, 3, ts.size))
        lat, nus = D.latent_draws(lat_mean, lat_cov, z)
        assert np.all(nus >= D.NU_MIN) and np.all(nus <= D.NU_MAX * 1.0001)
        for gi in range(6):
            nu, L = D.ladder(lat_cov[gi])
            assert nu == nus[gi] and np.all(L[np.triu_indices(ts.size, 1)] == 0.0)
            back = np.abs(L @ L.T - nu * np.eye(ts.size) - lat_cov[gi]).max() / np.abs(np.diag(lat_cov[gi])).max()
            assert back <= 1e-12, (gi, back)
            np.testing.assert_allclose(lat[gi], lat_mean[gi][None] + z[gi] @ L.T, rtol=0, atol=1e-13 * np.abs(lat[gi]).max())
        out = D.output_draws(lat, lat_cov, p, q, pr['jitters'])
        assert out.shape == (p, 3, ts.size)
        for i in range(p):
            s = sum(lat[q + j * p + i] * lat[j] for j in range(q))
            np.testing.assert_allclose(out[i], s, rtol=1e-13, atol=1e-13 * np.abs(s).max())
    # two sweeps are one sweep from the state the first one leaves
    _, _, mu1, var1 = D.posterior(pr, mask, 'reference', mu0, var0, comp, ts)
    a = D.posterior(pr, mask, 'reference', mu1, var1, comp, ts)
    b = D.posterior(pr, mask, 'reference', mu0, var0, comp, ts, sweeps=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_restatements_own_draws_stay_inside_the_moments_bound():
    """Test 8 of tests/test_draw_batch_gpu.py before the device: 20 000 draws of the restatement at 37 times under that test's
    seed, noise N(0, jitter^2) drawn behind the normals from the same generator, against the restatement's own mean and
    variance (the jitter once) -- inside 5 standard errors, the variance's from the draws' fourth moment."""
    pr, mask, mu0, var0 = _case_a()
    comp = (pr['nodes'], pr['weights'], pr['means'], pr['jitters'])
    p, q, n = 2, 2, 20000
    ts = V.mixed_times(pr['time'], 37, seed=37)
    gen = np.random.default_rng(SEED)
    z = gen.standard_normal((2, 6, n, ts.size))
    eps = gen.standard_normal((2, n, ts.size, p))
    for b in range(2):                                        # (the same posterior for both: what varies is the normals)
        lat_mean, lat_cov, _, _ = D.posterior(pr, mask, 'reference', mu0, var0, comp, ts, sweeps=2)
        lat, _ = D.latent_draws(lat_mean, lat_cov, z[b])
        f, w = lat[:q], lat[q:].reshape(q, p, n, ts.size)
        draws = np.transpose(np.array([sum(w[j, i] * f[j] for j in range(q)) for i in range(p)]), (1, 2, 0))
        draws = draws + eps[b] * np.abs(np.asarray(pr['jitters'], dtype=float))
        mean = V.combine(lat_mean, lat_cov, p, q, pr['jitters'])[0]
        var = V.variances(lat_mean, np.einsum('gnn->gn', lat_cov), p, q, pr['jitters'])
        m = draws.mean(axis=0)
        c = draws - m
        s2, m4 = (c ** 2).mean(axis=0), (c ** 4).mean(axis=0)
        zm = np.abs(m - mean) / np.sqrt(var / n)
        zv = np.abs(s2 * n / (n - 1) - var) / np.sqrt((m4 - s2 ** 2) / n)
        print('restatement moments, normals of vector %d: worst mean %.2f SE, worst variance %.2f SE' % (b, zm.max(), zv.max()))
        assert zm.max() < 5 and zv.max() < 5
