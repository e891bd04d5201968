"""Full predictive covariances and joint posterior draws on the GPU (inference.predict_cov / sample_posterior over
gprn_predict_cov / gprn_predict_draws) against the library's own _Prediction, the reference's fixtures and the NumPy /
SciPy restatement of _gp.GP.prediction (_gp.py:125-137) with the covariance kept whole (tests/_predict_cov_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _cases
from tests import _predict_cov_ref as ref

pytestmark = pytest.mark.gpu

TAGS = ['step_p1q1', 'step_p3q2', 'step_p2q3', 'cfg1_N200', 'mid_N300_p3q2']
# |C_dev - C_numpy| <= COV_TOL sqrt(diag C (x) diag C), latent and output matrices, cross blocks included (worst cases are
# printed per fixture)
COV_TOL = 1e-8


def _model(tag, state=True):
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    g = gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d))
    g.set_components(nodes, weights, means, jit)
    if state:
        g._mu, g._var = np.asarray(d['mu_final'], dtype=float), np.asarray(d['var_final'], dtype=float)
    return meta, d, g


def _state(g):
    if g._mu is None:
        return g._initMuVar(g.nodes, g.weights, g.jitters)
    return g._mu, g._var


def _numpy_latents(g, tstar):
    mu, var = _state(g)
    ms, vs = ref.latent_state(mu, var, g.p, g.q, g.time.size)
    out = [ref.latent_posterior(k, g.time, m, v, tstar) for k, m, v in zip(list(g.nodes) + list(g.weights), ms, vs)]
    return [o[0] for o in out], [o[1] for o in out]


def _worst(a, b):
    d = np.sqrt(np.abs(np.outer(np.diag(b), np.diag(b))))
    return float((np.abs(a - b) / np.where(d > 0, d, 1e-300)).max())


def _tstar(g, ns):
    lo, hi = g.time.min(), g.time.max()
    span = hi - lo
    return np.linspace(lo - 0.3 * span, hi + 0.3 * span, ns)       # beyond the data span on both sides


@pytest.mark.parametrize('tag', TAGS)
def test_diagonal_is_the_prediction_variance(tag):
    meta, d, g = _model(tag)
    fx = np.load(os.path.join(_cases.GOLDEN, 'pred_' + tag + '.npz'))
    mean, var = g._Prediction(tstar=fx['tstar'], mu=d['mu_final'], var=d['var_final'])
    m2, cov = g.predict_cov(tstar=fx['tstar'])
    assert cov.shape == (g.p, fx['tstar'].size, fx['tstar'].size)
    diag = np.array([np.diag(c) for c in cov]).T
    np.testing.assert_allclose(diag, var, rtol=1e-9, atol=0)
    np.testing.assert_allclose(diag, fx['var'], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(m2, mean, rtol=1e-13, atol=0)
    np.testing.assert_allclose(m2, fx['mean'], rtol=1e-7, atol=1e-9)
    for c in cov:
        np.testing.assert_array_equal(c, c.T)


@pytest.mark.parametrize('ns', [1, 37, 128, 300, 1000])
@pytest.mark.parametrize('tag', TAGS)
def test_covariances_match_numpy(tag, ns):
    meta, d, g = _model(tag)
    ts = _tstar(g, ns)
    mean, joint, Cn, Cw = g.predict_cov(tstar=ts, joint=True, separate=True)
    nm, nc = _numpy_latents(g, ts)
    lat = list(Cn) + list(Cw)
    worst_lat = max(_worst(a, b) for a, b in zip(lat, nc))
    for C in lat:
        np.testing.assert_array_equal(C, C.T)
        ev = np.linalg.eigvalsh(C)
        assert ev.min() >= -1e-10 * np.abs(np.diag(C)).max(), ev.min()
    jn = ref.output_cov(nm, nc, g.jitters, g.p, g.q, joint=True)
    worst_out = _worst(joint, jn)
    np.testing.assert_array_equal(joint, joint.T)
    _, per = g.predict_cov(tstar=ts)
    for i in range(g.p):                                     # the per-output matrices are the joint one's diagonal blocks
        np.testing.assert_allclose(per[i], joint[i * ns:(i + 1) * ns, i * ns:(i + 1) * ns], rtol=0, atol=0)
    print(f'{tag} ns={ns}: worst |dC| / sqrt(d d) latent {worst_lat:.2e}, output (joint) {worst_out:.2e}')
    assert worst_lat <= COV_TOL and worst_out <= COV_TOL


@pytest.mark.parametrize('tag', ['step_p3q2', 'cfg1_N200', 'mid_N300_p3q2'])
def test_draws_with_fixed_normals(tag):
    """Latent draws are mean + L z with L L^T = C + nu I.  L is recovered column by column from unit vectors z = e_d; its
    product is checked against the device's own C (backward error), and the draws of random z against mean + L z.  (A
    forward comparison with NumPy's Cholesky factor is ill-posed here: C is singular to rounding, cond(C + nu I) ~ 1e12,
    and the trailing columns of two fp64 factors of matrices 1e-12 apart differ by ~1e-5.)  Output draws are sum_j w o f
    of the returned latent draws."""
    meta, d, g = _model(tag)
    ts = _tstar(g, 150)
    ns, G = ts.size, g.q * (g.p + 1)
    _, _, Cn, Cw = g.predict_cov(tstar=ts, separate=True)
    C = list(Cn) + list(Cw)
    ctx = g._stage_posterior(g.nodes, g.weights, g.means, g.jitters, ts)
    eye = np.broadcast_to(np.eye(ns), (G, ns, ns)).copy()
    lat0, _, nug0, info = ctx.predict_draws(ts, np.zeros((G, 1, ns)))
    assert info == 0
    latI, _, nug, info = ctx.predict_draws(ts, eye)
    assert info == 0 and np.array_equal(nug, nug0)
    assert np.all(nug >= 1.25e-12) and np.all(nug <= 1.25e-6 * 1.0001)
    Ls = []
    for gi in range(G):
        L = (latI[gi] - lat0[gi]).T                           # column d = L e_d
        assert np.all(L[np.triu_indices(ns, 1)] == 0.0)
        A = C[gi] + nug[gi] * np.eye(ns)
        back = np.abs(L @ L.T - A).max() / np.abs(np.diag(A)).max()
        assert back <= 1e-12, (gi, back)
        Ls.append(L)
    nm, _ = _numpy_latents(g, ts)
    z = np.random.default_rng(7).standard_normal((G, 5, ns))
    lat, out, nug2, info = ctx.predict_draws(ts, z)
    assert info == 0 and np.array_equal(nug2, nug)
    worst = 0.0
    for gi in range(G):
        expect = lat0[gi] + (Ls[gi] @ z[gi].T).T
        worst = max(worst, np.abs(lat[gi] - expect).max() / np.abs(expect).max())
        np.testing.assert_allclose(lat0[gi][0], nm[gi], rtol=0, atol=1e-8 * np.abs(nm[gi]).max())
    print(f'{tag}: worst draw vs mean + L z {worst:.2e}, nuggets {nug}')
    assert worst <= 1e-12
    q, p = g.q, g.p
    for i in range(p):
        s = sum(lat[q + j * p + i] * lat[j] for j in range(q))
        np.testing.assert_allclose(out[i], s, rtol=1e-13, atol=1e-13 * np.abs(s).max())


def test_draw_moments_match_the_prediction():
    meta, d, g = _model('mid_N300_p3q2')
    fx = np.load(os.path.join(_cases.GOLDEN, 'pred_mid_N300_p3q2.npz'))
    ts = fx['tstar']
    assert ts.size == 37
    mean, var = g._Prediction(tstar=ts, mu=d['mu_final'], var=d['var_final'])
    n = 20000
    draws = g.sample_posterior(tstar=ts, n=n, noise=True, rng=12345)
    assert draws.shape == (n, ts.size, g.p) and np.all(np.isfinite(draws))
    m = draws.mean(axis=0)
    c = draws - m
    s2 = (c ** 2).mean(axis=0)
    m4 = (c ** 4).mean(axis=0)
    se_mean = np.sqrt(var / n)
    se_var = np.sqrt((m4 - s2 ** 2) / n)                      # (the fourth moment of the draws, not the Gaussian 2 s^4)
    zm, zv = np.abs(m - mean) / se_mean, np.abs(s2 * n / (n - 1) - var) / se_var
    print(f'moments: worst mean {zm.max():.2f} SE, worst variance {zv.max():.2f} SE')
    assert zm.max() < 5 and zv.max() < 5


def test_duplicated_times_raise_the_nugget():
    # every time three times: C_g is singular but for K**'s 1.25e-12 nugget, which a node of amplitude 1e6 drowns in rounding
    g = _synthetic(2, 1, [covfunc.SquaredExponential(1e3, 10.0)],
                   [covfunc.SquaredExponential(1.0, 15.0), covfunc.SquaredExponential(1.1, 12.0)])
    ts = np.repeat(_tstar(g, 40), 3)
    draws, nd, wd = g.sample_posterior(tstar=ts, n=4, separate=True, rng=3)
    assert np.all(np.isfinite(draws)) and np.all(np.isfinite(nd)) and np.all(np.isfinite(wd))
    assert g.last_nuggets.max() > 1.25e-12 and g.last_nuggets.max() <= 1.25e-6 * 1.0001
    print('nuggets', g.last_nuggets)


class _UserKernel(covfunc.covFunction):
    def __init__(self, inner):
        super().__init__(*inner.pars)
        self._inner = inner
        self._param_names = inner._param_names

    def __call__(self, r):
        return self._inner(r)


def _check_against_numpy(g, ts, what):
    mean, joint, Cn, Cw = g.predict_cov(tstar=ts, joint=True, separate=True)
    nm, nc = _numpy_latents(g, ts)
    worst_lat = max(_worst(a, b) for a, b in zip(list(Cn) + list(Cw), nc))
    worst_out = _worst(joint, ref.output_cov(nm, nc, g.jitters, g.p, g.q, joint=True))
    print(f'{what}: worst latent {worst_lat:.2e}, output {worst_out:.2e}')
    assert worst_lat <= COV_TOL and worst_out <= COV_TOL
    draws = g.sample_posterior(tstar=ts, n=3, rng=1)
    assert np.all(np.isfinite(draws))


def test_user_defined_kernels():
    meta, d, g = _model('step_p3q2')
    g.set_components([_UserKernel(k) for k in g.nodes], [_UserKernel(k) for k in g.weights], g.means, g.jitters)
    assert g.nodes[0]._device_program() is None
    _check_against_numpy(g, _tstar(g, 70), 'user kernels')


def _synthetic(p, q, nodes, weights, N=90):
    rng = np.random.default_rng(5)
    t = np.sort(rng.uniform(0, 60, N))
    args = []
    for _ in range(p):
        args += [np.sin(t / 7) + 0.1 * rng.standard_normal(N), np.full(N, 0.2)]
    g = gpyrn.inference(q, t, *args)
    g.set_components(nodes, weights, [meanfunc.Constant(0.0)] * p, [0.3] * p)
    return g


def test_polynomial_weight():
    g = _synthetic(2, 1, [covfunc.SquaredExponential(1.0, 8.0)],
                   [covfunc.Polynomial(0.5, 1e-3, 0.2, 2.0), covfunc.SquaredExponential(1.2, 12.0)])
    assert isinstance(g.weights[0], covfunc.Polynomial)
    _check_against_numpy(g, _tstar(g, 50), 'polynomial')


def test_composite_kernel():
    comp = covfunc.SquaredExponential(1.0, 20.0) * covfunc.Periodic(1.0, 9.0, 0.8) + covfunc.Matern32(0.5, 5.0)
    g = _synthetic(1, 1, [comp], [covfunc.SquaredExponential(1.0, 15.0)])
    assert g.nodes[0]._device_program() is not None
    _check_against_numpy(g, _tstar(g, 60), 'SE * Periodic + Matern32')


def test_config3_size():
    meta, d, g = _model('cfg3_N4096')
    mu, var = g._mu, g._var
    ts = _tstar(g, 1024)
    mean, pvar = g._Prediction(tstar=ts, mu=mu, var=var)
    m2, cov = g.predict_cov(tstar=ts)
    diag = np.array([np.diag(c) for c in cov]).T
    np.testing.assert_allclose(diag, pvar, rtol=1e-9, atol=0)
    np.testing.assert_allclose(m2, mean, rtol=1e-13, atol=0)
    ctx = g._backend()
    assert ctx.option('flags') == 1 and ctx.option('fallbacks') == 0


def test_sharded_context_is_refused(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs, outs = [], []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), GPRN_COMM_TRANSPORT='shm',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(21000 + os.getpid() % 20000))
        out = str(tmp_path / f'rank{r}.npz')
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, '-m', 'tests._cov_shard_worker', 'step_p3q2', out,
                                       f'{os.getpid()}_cov_shard'], cwd=root, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q_ in procs:
                q_.kill()
            raise
        logs.append(o.decode(errors='replace'))
    assert all(pr.returncode == 0 for pr in procs), '\n'.join(logs)
    for o in outs:
        msgs = [str(m) for m in np.load(o)['messages']]
        assert len(msgs) == 2
        for m in msgs:
            assert 'sharded context' in m and f'code {_hip.GPRN_E_UNSUPPORTED}' in m, m
