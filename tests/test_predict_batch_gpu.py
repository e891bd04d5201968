"""Prediction for many parameter vectors side by side on the GPU (gprn_predict_batch, Context.predict_batch,
inference.predict_batch / posterior_predictive): every slot of a batch against the reference's prediction fixtures, perturbed
vectors with states of their own across chunk boundaries against the device one by one, the blocking of the prediction
times, the two batched fills bit for bit against the fills of gprn_predict, a failed pivot in the middle of a batch, the
caller's context left alone, the refusals and the Python fallbacks.  The bounds are the project's own for a prediction
(tests/test_parity_gpu.py): means rtol 1e-7 / atol 1e-9, variances rtol 1e-6 / atol 1e-9.  No call may fall back to the
event schedule."""
import os
from itertools import chain

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _cases, _mask_ref as MR

pytestmark = pytest.mark.gpu
MEAN_TOL = dict(rtol=1e-7, atol=1e-9)
VAR_TOL = dict(rtol=1e-6, atol=1e-9)
TAGS = ['step_p1q1', 'step_p3q2', 'step_p2q3', 'cfg1_N200', 'mid_N300_p3q2']


def _model(tag, **kw):
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    g = gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d), **kw)
    g.set_components(nodes, weights, means, jit)
    return meta, d, g


def _fixture(tag):
    return np.load(os.path.join(_cases.GOLDEN, 'pred_' + tag + '.npz'))


def _tstar(g, ns):
    lo, hi = g.time.min(), g.time.max()
    span = hi - lo
    return np.linspace(lo - 0.3 * span, hi + 0.3 * span, ns)       # beyond the data span on both sides


def _perturbed(g, d, B, seed):
    """B parameter vectors at +-1-3 % of the fixture's, each with a perturbed copy of the fixture's final state."""
    rng = np.random.RandomState(seed)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * (1.0 + rng.choice([-1.0, 1.0], x0.size) * rng.uniform(0.01, 0.03, x0.size)) for _ in range(B)]
    mu0, var0 = np.asarray(d['mu_final'], dtype=float), np.asarray(d['var_final'], dtype=float)
    mu = np.array([mu0 * (1.0 + 0.02 * rng.standard_normal(mu0.shape)) for _ in range(B)])
    var = np.array([var0 * rng.uniform(0.97, 1.03, var0.shape) for _ in range(B)])
    assert (var > 0).all()
    return sets, mu, var


def _one_by_one(g1, x, mu, var, tstar):
    """(mean, var, latent means (G, ns), latent variances (G, ns)) of _Prediction / gprn_predict for this vector and state"""
    g1.set_parameters(np.array(x, dtype=float))
    mean, pvar, parts = g1._Prediction(tstar=tstar, mu=mu, var=var, separate=True)
    assert g1.last_info == 0
    gm, gv, info = g1._backend().predict(tstar)              # (the kernels and the state _Prediction just sent)
    assert info == 0
    np.testing.assert_array_equal(gm, np.concatenate([np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)]))
    return mean, pvar, gm, gv


def _both_ways(g, sets, mu, var, tstar):
    """Context.predict_batch with both pairs, and inference.predict_batch(states=) over the same list: the latter's values
    are the former's with the mean functions added.  Returns (mean (B, ns, p), var, lat_mean (B, G, ns), lat_var)."""
    B = len(sets)
    staged = g._predict_stage([np.array(x, dtype=float) for x in sets], tstar)
    assert staged is not None
    ctx, kp, jt, meanvals = staged
    res = ctx.predict_batch(kp, mu.reshape(B, -1), var.reshape(B, -1), tstar, jitters=jt)
    assert res is not None, 'the library has no side-by-side form for this problem'
    lm, lv, om, ov, info = res
    assert not info.any()
    only = ctx.predict_batch(kp, mu.reshape(B, -1), var.reshape(B, -1), tstar, jitters=jt, latent=False)
    assert only[0] is None and only[1] is None
    np.testing.assert_array_equal(only[2], om)               # (the out_* pair alone: the same bits, a smaller read-back)
    np.testing.assert_array_equal(only[3], ov)
    mean, pvar, lat = g.predict_batch(sets, tstar=tstar, states=(mu, var), separate=True)
    assert g.last_info == 0
    np.testing.assert_array_equal(lat, lm)
    np.testing.assert_array_equal(mean, np.transpose(om + meanvals, (0, 2, 1)))
    np.testing.assert_array_equal(pvar, np.transpose(ov, (0, 2, 1)))
    assert ctx.option('fallbacks') == 0
    return mean, pvar, lm, lv


# ------------------------------------------------------------------ 1. every slot against the reference's fixtures
# step_*: one tile (T = 1, the same launches); cfg1_N200: two tiles; mid_N300_p3q2: three tiles
@pytest.mark.parametrize('tag', TAGS)
def test_every_slot_reproduces_the_reference(tag):
    B = 5
    meta, d, g = _model(tag)
    fx = _fixture(tag)
    x = np.array(g.get_parameters(), dtype=float)
    mu = np.tile(np.asarray(d['mu_final'], dtype=float), (B, 1, 1, 1))
    var = np.tile(np.asarray(d['var_final'], dtype=float), (B, 1, 1, 1))
    mean, pvar, lm, lv = _both_ways(g, [x] * B, mu, var, fx['tstar'])
    q = g.q
    assert mean.shape == (B,) + fx['mean'].shape and lm.shape == (B, g.q * (g.p + 1), fx['tstar'].size)
    for b in range(B):
        np.testing.assert_allclose(lm[b, :q], fx['node_means'], **MEAN_TOL)
        np.testing.assert_allclose(lm[b, q:], fx['weight_means'], **MEAN_TOL)
        np.testing.assert_allclose(mean[b], fx['mean'], **MEAN_TOL)
        np.testing.assert_allclose(pvar[b], fx['var'], **VAR_TOL)
        assert np.array_equal(mean[b], mean[0]) and np.array_equal(pvar[b], pvar[0]) and np.array_equal(lv[b], lv[0])


# ------------------------------------------------------------------ 2. perturbed vectors and states, chunk boundaries
# (per evaluation 4 G + q - 1 matrices of ld^2 doubles: 4.3 MB at step_p3q2, 4.2 MB at cfg1_N200, 39 MB at mid_N300_p3q2)
@pytest.mark.parametrize('tag,budget_mb', [('step_p3q2', 10), ('cfg1_N200', 10), ('mid_N300_p3q2', 100)])
def test_perturbed_vectors_against_one_by_one_across_chunks(tag, budget_mb):
    B = 7
    meta, d, g = _model(tag)
    _, _, g1 = _model(tag)                                   # the one-by-one side, a context of its own
    g._backend().option('batch_mem_mb', budget_mb)
    tstar = _fixture(tag)['tstar']
    sets, mu, var = _perturbed(g, d, B, 23)
    mean, pvar, lm, lv = _both_ways(g, sets, mu, var, tstar)
    chunk = g._backend().option('batch_chunk')
    assert chunk in (2, 3), chunk
    for b in range(B):
        m1, v1, gm, gv = _one_by_one(g1, sets[b], mu[b], var[b], tstar)
        np.testing.assert_allclose(lm[b], gm, **MEAN_TOL)
        np.testing.assert_allclose(lv[b], gv, **VAR_TOL)
        np.testing.assert_allclose(mean[b], m1, **MEAN_TOL)
        np.testing.assert_allclose(pvar[b], v1, **VAR_TOL)
    assert g1._backend().option('fallbacks') == 0


# ------------------------------------------------------------------ 3. blocks of prediction times and their padding
# cfg1_N200: ld = 256, so 300 times are two blocks, the second ragged (44 rows of a 128-row tile); step_p1q1: ld = 128
@pytest.mark.parametrize('tag,sizes', [('cfg1_N200', (1, 128, 129, 256, 300)), ('step_p1q1', (1, 129))])
def test_blocks_of_prediction_times(tag, sizes):
    B = 3
    meta, d, g = _model(tag)
    _, _, g1 = _model(tag)
    sets, mu, var = _perturbed(g, d, B, 5)
    ctx, kp, jt, _ = g._predict_stage(sets, _tstar(g, 2))
    flat = lambda a: a.reshape(B, -1)
    for ns in sizes:
        tstar = _tstar(g, ns) if ns > 1 else np.array([0.5 * (g.time.min() + g.time.max())])
        lm, lv, om, ov, info = ctx.predict_batch(kp, flat(mu), flat(var), tstar, jitters=jt)
        assert not info.any() and lm.shape == (B, g.q * (g.p + 1), ns) and om.shape == (B, g.p, ns)
        for b in range(B):
            _, _, gm, gv = _one_by_one(g1, sets[b], mu[b], var[b], tstar)
            np.testing.assert_allclose(lm[b], gm, **MEAN_TOL)
            np.testing.assert_allclose(lv[b], gv, **VAR_TOL)
        ld = 128 * ((g.N + 127) // 128)
        if ns > ld:                                          # block by block = call by call, row for row
            head = ctx.predict_batch(kp, flat(mu), flat(var), tstar[:ld], jitters=jt)
            tail = ctx.predict_batch(kp, flat(mu), flat(var), tstar[ld:], jitters=jt)
            for whole, a, b_ in zip((lm, lv, om, ov), head[:4], tail[:4]):
                assert np.array_equal(whole, np.concatenate([a, b_], axis=2))
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 4. the two batched fills, bit for bit
# a single SE (cfg1_N200's node), a single QP (step_p3q2's node), kmix_N200_p2q2's composites SE * Periodic and SE +
# Exponential, and its Matern52 (a single kernel without host-computed reciprocals: the postfix program's path)
@pytest.mark.parametrize('tag,gp,ns', [('cfg1_N200', 0, 130), ('step_p3q2', 0, 37), ('kmix_N200_p2q2', 1, 256),
                                       ('kmix_N200_p2q2', 4, 77), ('kmix_N200_p2q2', 2, 128)])
def test_batched_fills_have_the_bits_of_the_single_fills(tag, gp, ns):
    B = 2
    meta, d, g = _model(tag)
    sets, mu, var = _perturbed(g, d, B, 11)
    tstar = _tstar(g, ns)
    ctx, kp, jt, _ = g._predict_stage(sets, tstar)
    kinds = [type(k).__name__ for k in chain(g.nodes, g.weights)]
    for e in range(B):
        single = ctx.test_predict_fill(kp, var, e, gp, tstar, batched=False)
        batched = ctx.test_predict_fill(kp, var, e, gp, tstar, batched=True)
        for what, a, b in zip(('K + diag v', 'K*', 'k**'), batched, single):
            assert np.all(np.isfinite(b)), (kinds[gp], what)
            assert np.array_equal(a, b), '%s of %s (evaluation %d): %d entries differ, worst %.3g' % (
                what, kinds[gp], e, int((a != b).sum()), float(np.abs(a - b).max()))
        assert np.array_equal(single[0], single[0].T)


# ------------------------------------------------------------------ 5. a failed pivot in the middle
def test_a_failed_pivot_in_the_middle_of_a_batch():
    """Evaluation 2's node variances are -10: K + 1.25e-12 I + diag v has no positive pivot -- a numerical verdict, not a
    fault.  The call without the bad state has a good one in its place (the same launch shapes)."""
    B = 4
    meta, d, g = _model('step_p3q2')
    sets, mu, var = _perturbed(g, d, B, 3)
    tstar = _fixture('step_p3q2')['tstar']
    ctx, kp, jt, _ = g._predict_stage(sets, tstar)
    flat = lambda a: a.reshape(B, -1)
    good = ctx.predict_batch(kp, flat(mu), flat(var), tstar, jitters=jt)
    bad_var = var.copy()
    bad_var[2, 0] = -10.0                                    # (row 0 of (p + 1, q, N): the nodes)
    res = ctx.predict_batch(kp, flat(mu), flat(bad_var), tstar, jitters=jt)
    info = res[4]
    assert info[2] > 0 and not info[[0, 1, 3]].any() and not good[4].any()
    for a, b in zip(res[:4], good[:4]):
        assert np.array_equal(a[[0, 1, 3]], b[[0, 1, 3]])
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 6. the caller's context is left alone
@pytest.mark.parametrize('tag', ['step_p3q2', 'cfg1_N200'])
def test_the_caller_is_untouched(tag):
    meta, d, g = _model(tag)
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    assert g.last_info == 0
    ctx.set_muvar(np.asarray(d['mu_init'], dtype=float), np.asarray(d['var_init'], dtype=float))
    ctx.sweep(2, commit=True)
    before = ctx.sweep(1, commit=False)
    state = ctx.get_muvar()
    B = 3
    sets, mu, var = _perturbed(g, d, B, 9)
    kp = []
    for x in sets:                                           # (nothing is sent to the device: the kernels stay as set up)
        g.set_parameters(x)
        kp.append(np.concatenate([g._kernel_spec(k)[2] for k in chain(g.nodes, g.weights)]))
    res = ctx.predict_batch(np.array(kp), mu.reshape(B, -1), var.reshape(B, -1), _tstar(g, 300),
                            jitters=np.tile(np.asarray(meta['jitters'], dtype=float), (B, 1)))
    assert res is not None and not res[4].any()
    after = ctx.sweep(1, commit=False)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    for a, b in zip(state, ctx.get_muvar()):
        assert np.array_equal(a, b)
    meta, d, g = _model(tag)                                 # the fixture's own parameters again
    g._ctx = ctx
    E, _, _, _ = g.ELBOcalc()
    np.testing.assert_allclose(E, float(d['calc_elbo']), rtol=1e-8)
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 7. refusals and fallbacks
class _UserKernel(covfunc.covFunction):
    """A user-defined covFunction subclass around a built-in: no device program."""

    def __init__(self, inner):
        super().__init__(*inner.pars)
        self._inner = inner
        self._param_names = inner._param_names

    def __call__(self, r):
        return self._inner(r)


def test_user_defined_kernels_are_refused_and_fall_back():
    B = 3
    meta, d, g = _model('step_p3q2')
    g.set_components([_UserKernel(k) for k in g.nodes], [_UserKernel(k) for k in g.weights], g.means, g.jitters)
    x = np.array(g.get_parameters(), dtype=float)
    tstar = _fixture('step_p3q2')['tstar']
    mu = np.tile(np.asarray(d['mu_final'], dtype=float), (B, 1, 1, 1))
    var = np.tile(np.asarray(d['var_final'], dtype=float), (B, 1, 1, 1))
    assert g._predict_stage([x] * B, tstar) is None
    # the C call itself: uploaded matrices have no program to substitute parameters into
    ctx = g._backend()
    for gp, k in enumerate(chain(g.nodes, g.weights)):
        g._send_spec(ctx, gp, g._kernel_spec(k))
    g._prior_key = None
    n_k = sum(k.pars.size for k in chain(g.nodes, g.weights))
    assert ctx.predict_batch(np.ones((B, n_k)), mu.reshape(B, -1), var.reshape(B, -1), tstar,
                             jitters=np.ones((B, g.p))) is None          # (GPRN_E_UNSUPPORTED)
    mean, pvar, lat = g.predict_batch([x] * B, tstar=tstar, states=(mu, var), separate=True)
    m1, v1, parts = g._Prediction(tstar=tstar, mu=mu[0], var=var[0], separate=True)
    for b in range(B):
        assert np.array_equal(mean[b], m1) and np.array_equal(pvar[b], v1)
        assert np.array_equal(lat[b], np.concatenate([np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)]))
    fx = _fixture('step_p3q2')
    np.testing.assert_allclose(mean[0], fx['mean'], **MEAN_TOL)


def test_a_masked_object_predicts_side_by_side():
    B = 4
    meta, d = _cases.load('step_p2q1')
    mask = MR.partial_mask(meta['p'], meta['N'], 4)
    _, _, g = _model('step_p2q1', mask=mask)
    _, _, g1 = _model('step_p2q1', mask=mask)
    assert not g._batchable()                                # (its loops run one by one)
    sets, mu, var = _perturbed(g, d, B, 31)
    tstar = _tstar(g, 150)
    mean, pvar, lm, lv = _both_ways(g, sets, mu, var, tstar)
    for b in range(B):
        m1, v1, gm, gv = _one_by_one(g1, sets[b], mu[b], var[b], tstar)
        np.testing.assert_allclose(lm[b], gm, **MEAN_TOL)
        np.testing.assert_allclose(lv[b], gv, **VAR_TOL)
        np.testing.assert_allclose(mean[b], m1, **MEAN_TOL)
        np.testing.assert_allclose(pvar[b], v1, **VAR_TOL)


# ------------------------------------------------------------------ 8. states=None: the loops of nELBO_batch first
def test_states_none_runs_the_loops_of_nelbo_batch():
    B = 4
    tag = 'step_p3q2'
    meta, d, g = _model(tag)
    _, _, g2 = _model(tag)
    sets, _, _ = _perturbed(g, d, B, 41)
    start = (np.asarray(d['mu_final'], dtype=float), np.asarray(d['var_final'], dtype=float))
    tstar = _fixture(tag)['tstar']
    g._mu, g._var = start[0].copy(), start[1].copy()
    mean, pvar = g.predict_batch(sets, tstar=tstar, max_iter=200)
    # the same list from the same start through Context.elbocalc_batch, then predict_batch(states=)
    g2._mu, g2._var = start[0].copy(), start[1].copy()
    ctx, kp, yr, jt, m0, v0 = g2._batch_stage([np.array(x, dtype=float) for x in sets])
    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 200, want_state=True)
    assert res is not None and not res[3].any()
    mean2, pvar2 = g2.predict_batch(sets, tstar=tstar, states=(res[4], res[5]))
    assert np.array_equal(mean, mean2) and np.array_equal(pvar, pvar2)
    # what the object keeps: nELBO_batch's rule -- the state of the last evaluation whose loop converged, the last vector
    done = np.flatnonzero(res[2])
    assert done.size
    assert np.array_equal(g._mu, res[4][done[-1]]) and np.array_equal(g._var, res[5][done[-1]])
    assert g._batch_last_done == int(done[-1])
    np.testing.assert_array_equal(g.get_parameters(), sets[-1])
    m_pp, v_pp = g2.posterior_predictive(sets, tstar=tstar, states=(res[4], res[5]))
    np.testing.assert_allclose(m_pp, mean.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(v_pp, (pvar + mean ** 2).mean(axis=0) - mean.mean(axis=0) ** 2, rtol=1e-9, atol=1e-12)
    assert g._backend().option('fallbacks') == 0 and g2._backend().option('fallbacks') == 0
