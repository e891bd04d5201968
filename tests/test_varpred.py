"""The variational form of prediction (inference(..., predict='variational'); option "predict_form") without a device: the
dense restatement tests/_varpred_ref.py against the sweep it restates and against the textbook form, and the plumbing.

* At the data times the predictive IS the state the sweep leaves (_mask_ref.sweep / _order_mask_ref.sweep), rows of zero
  precision included: 1e-9 norm-wise per latent GP, a tenth of the device bound of tests/test_varpred_gpu.py.
* Against K* K^-1 mu and K** - K* K^-1 K*^T + K* K^-1 Sigma K^-1 K*^T on a problem whose cond(K) <= 1e4 (short length
  scales), 1e-9: with eps cond(K)^2 ~ 2e-8 that form could not carry the bound on the fixtures' priors (cond ~ 1e8), where it
  is not used.
"""
import os
import re

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _cases, _mask_ref as M, _order_mask_ref as R, _varpred_ref as V

TOL = 1e-9


def _kernels(pr):
    return list(pr['nodes']) + list(pr['weights'])


def _at_data_times(pr, mask, order, mu0, var0):
    inputs, mu_n, var_n = V.latent_inputs(*V.args(pr), mu0, var0, mask, order)
    t = pr['time']
    lat_mean, lat_cov = V.predict_latent(_kernels(pr), t, t, inputs)
    lat_var = np.einsum('gnn->gn', lat_cov)
    return inputs, mu_n, var_n, lat_mean, lat_var, lat_cov


def _state_rows(mu, p, q):
    """The (p + 1, q, N) state as rows per latent GP index: node j at j, weight (j, i) at q + j p + i."""
    mu = np.asarray(mu)
    return np.array([mu[0, j] for j in range(q)] + [mu[1 + i, j] for j in range(q) for i in range(p)])


@pytest.mark.parametrize('tag,masked,order', [('step_p3q2', False, 'reference'), ('mid_N300_p3q2', False, 'reference'),
                                              ('step_p3q2', True, 'reference'), ('mid_N300_p3q2', True, 'reference'),
                                              ('step_p2q3', False, 'sequential'), ('step_p2q3', True, 'sequential')])
def test_data_times_give_the_state(tag, masked, order):
    pr = M.problem(tag)
    p, N = pr['y_raw'].shape
    q = pr['meta']['q']
    mask = M.partial_mask(p, N, 3) if masked else np.ones((p, N), dtype=bool)
    mu0, var0 = M.init_state(pr, mask)
    # the restatement's (K, d, pred) are the sweep's: its state is the sweep's, bit for bit
    for _ in range(2):                                       # (the second sweep starts from a state with structure)
        if order == 'reference':
            _, mu_s, var_s, _ = M.sweep(*R.args(pr), mu0, var0, mask)
        else:
            _, mu_s, var_s, _ = R.sweep(*R.args(pr), mu0, var0, mask, order)
        inputs, mu_n, var_n, lat_mean, lat_var, _ = _at_data_times(pr, mask, order, mu0, var0)
        np.testing.assert_array_equal(mu_n, mu_s.reshape(mu_n.shape))
        np.testing.assert_array_equal(var_n, var_s.reshape(var_n.shape))
        e_mu = _cases._rowwise(lat_mean, _state_rows(mu_n, p, q))
        e_var = _cases._rowwise(lat_var, _state_rows(var_n, p, q))
        print(tag, 'masked' if masked else 'full', order, 'mean', e_mu, 'variance', e_var)
        assert e_mu <= TOL and e_var <= TOL
        mu0, var0 = mu_n, var_n
    if masked:
        assert any(np.any(d == 0.0) for _, d, _ in inputs)   # (rows of zero precision were among them)


def test_explicit_sigma_at_the_data_times():
    """C* at the data times is the Sigma the sweep forms (return_sigma), to 1e-9 of its largest entry."""
    pr = M.problem('step_p2q3')
    p, N = pr['y_raw'].shape
    q = pr['meta']['q']
    mask = M.partial_mask(p, N, 3)
    mu0, var0 = M.init_state(pr, mask)
    *_, sig_f, sig_w = R.sweep(*R.args(pr), mu0, var0, mask, 'sequential', return_sigma=True)
    *_, lat_cov = _at_data_times(pr, mask, 'sequential', mu0, var0)
    for j in range(q):
        assert np.abs(lat_cov[j] - sig_f[j]).max() <= TOL * np.abs(sig_f[j]).max()
        for i in range(p):
            assert np.abs(lat_cov[q + j * p + i] - sig_w[j, i]).max() <= TOL * np.abs(sig_w[j, i]).max()


def test_against_the_textbook_form():
    """Short length scales: cond(K) <= 1e4, where K^-1 is harmless."""
    rng = np.random.RandomState(5)
    N, p, q = 45, 2, 2
    t = 1.4 * np.arange(N) + rng.uniform(-0.2, 0.2, N)      # (no two times close: that is what keeps cond(K) small)
    nodes = [covfunc.SquaredExponential(1.0, 0.8), covfunc.QuasiPeriodic(1.1, 1.5, 7.0, 0.9)]
    weights = [covfunc.SquaredExponential(0.9 + 0.05 * k, 1.0 + 0.2 * k) for k in range(q * p)]
    means = [meanfunc.Constant(0.2)] * p
    jit = [0.4, 0.6]
    y = np.array([np.sin(t / 3.0) + 0.1 * rng.standard_normal(N), np.cos(t / 4.0) + 0.1 * rng.standard_normal(N)])
    yerr = rng.uniform(0.05, 0.2, (p, N))
    from oracle import cpu_ref
    Kf, Kw, _, _, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, y)
    assert max(np.linalg.cond(K) for K in list(Kf) + list(Kw)) <= 1e4
    mask = M.partial_mask(p, N, 2)
    mu0, var0 = cpu_ref.init_mu_var(np.where(mask, y, 0.0), [n.pars[0] for n in nodes], [w.pars[0] for w in weights], jit)
    inputs, *_ = V.latent_inputs(Kf, Kw, yres, y, yerr ** 2, jitt2, mu0, var0, mask)
    ts = V.mixed_times(t, 40, seed=1)
    lat_mean, lat_cov = V.predict_latent(nodes + weights, t, ts, inputs)
    for kernel, (K, d, pred), m, C in zip(nodes + weights, inputs, lat_mean, lat_cov):
        sigma, mu, _ = M._gp(K, d, pred)
        Ks, Kss = V.kernel_blocks(kernel, t, ts)
        A = np.linalg.solve(K, Ks.T).T                        # K* K^-1
        m_ref = A @ mu
        C_ref = Kss - A @ Ks.T + A @ sigma @ A.T
        assert np.abs(m - m_ref).max() <= TOL * np.abs(m_ref).max()
        assert np.abs(C - C_ref).max() <= TOL * np.abs(C_ref).max()


def test_the_coincidence_rule_of_the_restatement():
    """A data time in tstar gives the row of the set-up's K; a duplicated time gets the delta terms off the diagonal of K**;
    WhiteNoise counts as a delta term; the two-argument kernels get none."""
    from oracle import cpu_ref
    t = np.array([0.0, 1.5, 2.0, 4.0])
    ts = np.array([1.5, 3.0, 1.5, -1.0])
    k = covfunc.Sum(covfunc.SquaredExponential(1.2, 2.0), covfunc.WhiteNoise(0.3))
    K = cpu_ref.kmatrix(k, t)
    Ks, Kss = V.kernel_blocks(k, t, ts)
    np.testing.assert_allclose(Ks[0], K[1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(Ks[2], K[1], rtol=0, atol=1e-15)
    se = covfunc.SquaredExponential(1.2, 2.0)
    np.testing.assert_allclose(Ks[1], se(ts[1] - t), rtol=0, atol=1e-15)       # no delta term anywhere in that row
    assert Kss[0, 2] == Kss[0, 0] == Kss[2, 0] and abs(Kss[0, 0] - (1.44 + 0.09 + 1e-6)) < 1e-15
    assert abs(Kss[0, 1] - float(se(np.array(ts[0] - ts[1])))) < 1e-15
    pol = covfunc.Polynomial(1.0, 0.5, 0.1, 2)
    Ks2, Kss2 = V.kernel_blocks(pol, t, ts)
    np.testing.assert_allclose(Ks2[0], np.asarray(pol(t[1:2, None], t[None, :]))[0], rtol=1e-15)
    assert Kss2[0, 0] == Kss2[0, 2]


def test_the_combination_carries_the_jitter_once():
    rng = np.random.RandomState(0)
    p, q, ns = 2, 3, 7
    G = q * (p + 1)
    lat_mean = rng.standard_normal((G, ns))
    A = rng.standard_normal((G, ns, ns))
    lat_cov = A @ np.transpose(A, (0, 2, 1))
    jit = [0.3, 0.7]
    mean, cov = V.combine(lat_mean, lat_cov, p, q, jit)
    var = V.variances(lat_mean, np.einsum('gnn->gn', lat_cov), p, q, jit)
    np.testing.assert_allclose(np.einsum('inn->ni', cov), var, rtol=1e-13)
    mean_j, joint = V.combine(lat_mean, lat_cov, p, q, jit, joint=True)
    np.testing.assert_array_equal(mean, mean_j)
    assert np.array_equal(joint, joint.T)
    for i in range(p):
        np.testing.assert_array_equal(joint[i * ns:(i + 1) * ns, i * ns:(i + 1) * ns], cov[i])
    _, cov0 = V.combine(lat_mean, lat_cov, p, q, [0.0, 0.0])
    np.testing.assert_allclose(cov[1] - cov0[1], 0.49 * np.eye(ns), atol=1e-12)


# ------------------------------------------------------------------ plumbing (no device)
def test_header_constants_equal_the_binding():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gprn_hip.h')
    text = open(header).read()
    vals = {name: int(v) for name, v in re.findall(r'#define\s+(GPRN_PREDICT_\w+)\s+(\d+)', text)}
    assert vals == {'GPRN_PREDICT_REFERENCE': _hip.PREDICT_REFERENCE, 'GPRN_PREDICT_POSTERIOR': _hip.PREDICT_POSTERIOR}
    assert (_hip.PREDICT_REFERENCE, _hip.PREDICT_POSTERIOR) == (0, 1)
    assert '"predict_form"' in text and '"state_ready"' in text
    assert gpyrn.inference._PREDICT_FORMS == {'reference': 0, 'variational': 1}


def _tiny(**kw):
    t = np.linspace(0.0, 9.0, 10)
    return gpyrn.inference(1, t, np.sin(t), np.full(10, 0.1), **kw)


def test_the_switch_is_validated_before_a_device_call():
    for bad in ('x', 'posterior', None, 1):
        with pytest.raises(ValueError):
            _tiny(predict=bad)
    g = _tiny()
    assert g.predict_form == 'reference' and g._ctx is None
    g.predict_form = 'variational'
    assert g.predict_form == 'variational' and g._ctx is None
    with pytest.raises(ValueError):
        g.predict_form = 'bound'
    assert g.predict_form == 'variational'
    assert callable(g.predict)                               # (the property does not shadow the method)


def test_from_series_passes_the_switch_on():
    t1, t2 = np.arange(6.0), np.arange(1.0, 9.0, 2.0) + 0.5
    g = gpyrn.inference.from_series(1, [(t1, np.sin(t1), np.full(6, 0.1)), (t2, np.cos(t2), np.full(4, 0.1))],
                                    predict='variational')
    assert g.predict_form == 'variational' and g.mask is not None and g._ctx is None
    with pytest.raises(ValueError):
        gpyrn.inference.from_series(1, [(t1, np.sin(t1), np.full(6, 0.1))], predict='x')


class _Comm:
    world, rank, local_rank = 2, 0, 0


def test_a_sharded_object_refuses_the_variational_form():
    with pytest.raises(NotImplementedError, match='sharded'):
        _tiny(comm=_Comm(), predict='variational')
    g = _tiny(comm=_Comm())
    with pytest.raises(NotImplementedError, match='sharded'):
        g.predict_form = 'variational'
    assert g.predict_form == 'reference' and g._ctx is None


def test_the_batched_predictions_refuse_the_variational_form():
    g = _tiny(predict='variational')
    g.set_components(covfunc.SquaredExponential(1.0, 2.0), covfunc.SquaredExponential(1.0, 5.0), meanfunc.Constant(0.0), 0.1)
    x = g.get_parameters()
    for call in (g.predict_batch, g.posterior_predictive):
        with pytest.raises(NotImplementedError, match='end of a batch chunk'):
            call([x, x])
    assert g._ctx is None


def test_user_defined_kernels_are_refused_before_a_device_call():
    class Mine(covfunc.SquaredExponential):
        pass
    g = _tiny(predict='variational')
    g.set_components(Mine(1.0, 2.0), covfunc.SquaredExponential(1.0, 5.0), meanfunc.Constant(0.0), 0.1)
    with pytest.raises(NotImplementedError, match='device program'):
        g.predict(np.array([0.5]))
    assert g._ctx is None
