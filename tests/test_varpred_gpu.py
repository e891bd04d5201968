"""The variational form of prediction on the GPU (option "predict_form" = GPRN_PREDICT_POSTERIOR, inference(...,
predict='variational')) against the dense restatement tests/_varpred_ref.py and against the state the sweeps leave.

Shapes: one ragged tile (N = 45, p = q = 2, composite kernels with a WhiteNoise term, the small path -- and the launch path
with the small path switched off), N = 128 (the last full one-tile size), N = 129 (two tiles, the launch path),
mid_N300_p3q2 (three tiles), step_p2q3 in the sequential order under a mask with "order_mask".  Every masked case has rows of
zero precision, and the masked y / yerr handed over are NaN / inf.  Prediction times: ns in {1, 129, 300} (ns_pad equal to,
different from and beyond ld), each set a mix of data times, times between them, times outside the span and one duplicate.

Tolerances: the project's 1e-8 norm-wise per latent GP (tests/_cases.assert_state) on latent means and variances; 1e-8
relative on the output variances (bounded below by jitter^2); the output means norm-wise per output AND element by element,
1e-8 relative with an absolute floor of a thousandth of the output's largest mean (_close_means: they pass through zero as
the latent means do, and a sum of q products w f rounds at eps of its terms' size, not of its own).  The restatement predicts from ONE sweep off the initial state, so both sides form
(K, d, pred) from identical numbers.  No call may fall back to the event schedule."""
import ctypes
import functools
import os

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _cases, _mask_ref as M, _order_mask_ref as R, _varpred_ref as V

pytestmark = pytest.mark.gpu
TOL = 1e-8
POST = _hip.PREDICT_POSTERIOR

# name -> (problem, mask seed or None, sweep order, option "small_path" or None)
CASES = {
    'n45': (lambda: V.synthetic(45, 2, 2, seed=1, composite=True), 2, 'reference', None),
    'n45_launch': (lambda: V.synthetic(45, 2, 2, seed=1, composite=True), 2, 'reference', 0),
    'n128': (lambda: V.synthetic(128, 1, 1, seed=2), None, 'reference', None),
    'n129': (lambda: V.synthetic(129, 2, 1, seed=3), 5, 'reference', None),
    'mid300': (lambda: M.problem('mid_N300_p3q2'), 4, 'reference', None),
    'seq_p2q3': (lambda: M.problem('step_p2q3'), 3, 'sequential', None),
}
NS = (1, 129, 300)


@functools.lru_cache(maxsize=None)
def _problem(name):
    make, seed, order, small_path = CASES[name]
    pr = make()
    p, N = pr['y_raw'].shape
    if name == 'seq_p2q3':
        mask = M.partial_mask(2, 40, seed=3)
    else:
        mask = M.partial_mask(p, N, seed) if seed is not None else None
    if mask is not None:
        assert not mask.all()
    mu0, var0 = V.init_state(pr, mask)
    return pr, mask, order, small_path, np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float)


def _model(name, **kw):
    pr, mask, order, small_path, _, _ = _problem(name)
    y, e = pr['y_raw'], np.sqrt(pr['yerr2'])
    if mask is not None:
        y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
    args = [a for i in range(y.shape[0]) for a in (y[i], e[i])]
    q = len(pr['nodes'])
    g = gpyrn.inference(q, pr['time'], *args, mask=mask, sweep_order=order, sequential_under_mask=True, **kw)
    g.set_components(list(pr['nodes']), list(pr['weights']), list(pr['means']), list(pr['jitters']))
    return g


def _device(g, small_path=None):
    ctx = g._backend()
    if small_path is not None:
        ctx.option('small_path', small_path)
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    assert g.last_info == 0
    return ctx


def _assert_default_schedule(ctx):
    assert ctx.option('fallbacks') == 0
    if os.environ.get('GPRN_FLAGS', '1') != '0' and not os.environ.get('ROCPROF_COUNTER_COLLECTION'):
        assert ctx.option('flags') == 1


def _close_means(mean, ref, what):
    """Element by element: |mean - ref| <= 1e-8 max(|ref|, 1e-3 max |ref| of that output); (ns, p) arrays."""
    floor = 1e-3 * np.abs(ref).max(axis=0, keepdims=True)
    rel = float((np.abs(mean - ref) / np.maximum(np.abs(ref), floor)).max())
    print(what, 'output means off by', rel, '(element-wise relative, floored)')
    assert rel <= TOL


def _rows(state, p, q):
    s = np.asarray(state)
    return np.array([s[0, j] for j in range(q)] + [s[1 + i, j] for j in range(q) for i in range(p)])


@functools.lru_cache(maxsize=None)
def _reference(name, ns):
    """The restatement after ONE sweep from the initial state: latent means / covariances at the mixed times (ns = 0: at the
    data times), the state that sweep leaves, and the prediction times.  Computed once, shared, never written."""
    pr, mask, order, _, mu0, var0 = _problem(name)
    inputs, mu1, var1 = V.latent_inputs(*V.args(pr), mu0, var0, mask, order)
    ts = np.array(pr['time']) if ns == 0 else V.mixed_times(pr['time'], ns, seed=ns)
    lat_mean, lat_cov = V.predict_latent(list(pr['nodes']) + list(pr['weights']), pr['time'], ts, inputs)
    for a in (lat_mean, lat_cov, mu1, var1, ts):
        a.setflags(write=False)
    return ts, lat_mean, lat_cov, mu1, var1


def _swept(name, n_sweeps=1, **kw):
    """The model on the device in the posterior form, n committed sweeps from the initial state behind it."""
    pr, mask, order, small_path, mu0, var0 = _problem(name)
    g = _model(name, **kw)
    ctx = _device(g, small_path)
    assert ctx.option('predict_form', POST) in (0, 1)
    assert ctx.option('state_ready') == 0
    ctx.set_muvar(mu0, var0)
    _, _, info = ctx.sweep(n_sweeps, commit=True)
    assert info == 0 and ctx.option('state_ready') == 1
    return g, ctx


# ------------------------------------------------------------------ 1. data times give the state
@pytest.mark.parametrize('name,elbo', [('n45', 'reference'), ('n45', 'bound'), ('n45_launch', 'reference'), ('n128', 'reference'),
                                       ('n129', 'reference'), ('n129', 'bound'), ('mid300', 'reference'),
                                       ('seq_p2q3', 'reference'), ('seq_p2q3', 'bound')])
def test_data_times_give_the_state_after_forced_sweeps(name, elbo):
    g, ctx = _swept(name, n_sweeps=2, elbo=elbo)
    mu, var = ctx.get_muvar()
    gm, gv, info = ctx.predict(g.time)
    assert info == 0 and np.all(np.isfinite(gm)) and np.all(np.isfinite(gv))
    if g.mask is not None:
        assert (~g.mask).sum() > 0                             # (rows of zero precision: mask.hip's rows on the device)
    _cases.assert_state('varpred at the data times, forced sweeps %s %s' % (name, elbo), gm, _rows(mu, g.p, g.q),
                        gv, _rows(var, g.p, g.q), tol=TOL)
    assert ctx.option('state_ready') == 1
    _assert_default_schedule(ctx)


@pytest.mark.parametrize('name,elbo', [('n45', 'reference'), ('n129', 'bound'), ('seq_p2q3', 'reference')])
def test_data_times_give_the_state_after_elbocalc(name, elbo):
    g = _model(name, elbo=elbo, predict='variational')
    small_path = _problem(name)[3]
    if small_path is not None:
        g._backend().option('small_path', small_path)
    _, mu, var, it = g.ELBOcalc(max_iter=40)
    assert g.last_info == 0 and it >= 1
    ctx = g._backend()
    assert ctx.option('state_ready') == 1
    ctx.option('predict_form', POST)
    gm, gv, info = ctx.predict(g.time)
    assert info == 0
    _cases.assert_state('varpred at the data times, ELBOcalc %s %s (%d trips)' % (name, elbo, it), gm, _rows(mu, g.p, g.q),
                        gv, _rows(var, g.p, g.q), tol=TOL)
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ 2. other times
@pytest.mark.parametrize('ns', NS)
@pytest.mark.parametrize('name', list(CASES))
def test_latent_prediction_matches_the_restatement(name, ns):
    ts, lat_mean, lat_cov, mu1, var1 = _reference(name, ns)
    g, ctx = _swept(name)
    mu, var = ctx.get_muvar()
    _cases.assert_state('varpred: the sweep behind it %s' % name, mu, mu1.reshape(mu.shape), var, var1.reshape(var.shape))
    gm, gv, info = ctx.predict(ts)
    assert info == 0 and gm.shape == (g.q * (g.p + 1), ns)
    ref_var = np.einsum('gnn->gn', lat_cov)
    if ns == 1:
        print(name, 'ns = 1: mean', gm[:, 0], 'against', lat_mean[:, 0], 'variance', gv[:, 0], 'against', ref_var[:, 0])
    _cases.assert_state('varpred at %d mixed times %s' % (ns, name), gm, lat_mean, gv, ref_var, tol=TOL)
    assert np.all(gv > -TOL)
    _assert_default_schedule(ctx)


@pytest.mark.parametrize('name,ns', [('n45', 129), ('n129', 300), ('mid300', 129), ('seq_p2q3', 300)])
def test_inference_predict_matches_the_restatement(name, ns):
    pr, mask, order, small_path, mu0, var0 = _problem(name)
    ts, lat_mean, lat_cov, mu1, var1 = _reference(name, ns)
    g = _model(name, predict='variational')
    if small_path is not None:
        g._backend().option('small_path', small_path)
    shape = (g.p + 1, g.q, g.N)
    g._mu, g._var = mu0.reshape(shape).copy(), var0.reshape(shape).copy()
    mean, var, parts = g._Prediction(tstar=ts, separate=True)           # (one committed sweep from the stored state)
    assert g.last_info == 0
    _cases.assert_state('varpred: the state predict() keeps %s' % name, g._mu, mu1.reshape(shape), g._var, var1.reshape(shape))
    mvals = np.array([np.full(ts.size, 0.0) if m is None else m(ts) for m in pr['means']])
    ref_mean, _ = V.combine(lat_mean, lat_cov, g.p, g.q, pr['jitters'], mean_values=mvals)
    ref_var = V.variances(lat_mean, np.einsum('gnn->gn', lat_cov), g.p, g.q, pr['jitters'])
    e_mean = _cases._rowwise(mean.T, ref_mean.T)
    e_var = float(np.abs(var / ref_var - 1).max())
    print(name, ns, 'output means off by', e_mean, '(norm-wise per output), variances by', e_var, '(relative)')
    assert e_mean <= TOL and e_var <= TOL
    _close_means(mean, ref_mean, '%s %d' % (name, ns))
    # the jitter is there once: the reference form's q times would be off by (q - 1) jitter^2
    assert np.all(var >= np.asarray(pr['jitters']) ** 2 * (1 - 1e-12))
    np.testing.assert_array_equal(np.asarray(parts[0], dtype=float), np.asarray(
        g._backend().predict(ts)[0][:g.q]))                              # (separate: the latent means of the same call)
    t2, m2, sd2, _ = g.predict(tstar=ts)
    np.testing.assert_array_equal(m2, mean)
    np.testing.assert_array_equal(sd2, np.sqrt(var))


# ------------------------------------------------------------------ 3. predict_cov
@pytest.mark.parametrize('name,ns', [('n45', 129), ('n45_launch', 129), ('n129', 129), ('seq_p2q3', 300)])
def test_covariances_match_the_restatement(name, ns):
    pr = _problem(name)[0]
    ts, lat_mean, lat_cov, _, _ = _reference(name, ns)
    g, ctx = _swept(name)
    gm, gv, _ = ctx.predict(ts)
    mean, lat, joint = ctx.predict_cov(ts, joint=True)
    _, _, per = ctx.predict_cov(ts, joint=False, latent=False)
    np.testing.assert_array_equal(mean, gm)
    G = g.q * (g.p + 1)
    kernels = list(g.nodes) + list(g.weights)
    ld = 128 * ((g.N + 127) // 128)
    worst = 0.0
    for gi in range(G):
        np.testing.assert_array_equal(lat[gi], lat[gi].T)
        # the diagonal IS gprn_predict's variance: both are k** - sum_a W_a^2 over ld terms, summed in the tile kernel's order
        # and in the row kernel's; each sum is off by at most ld eps sum W^2 <= ld eps k**
        kss = float(V.kernel_blocks(kernels[gi], pr['time'][:1], ts[:1])[1][0, 0])
        assert np.abs(np.diag(lat[gi]) - gv[gi]).max() <= 2 * ld * np.finfo(float).eps * kss
        worst = max(worst, np.abs(lat[gi] - lat_cov[gi]).max() / np.abs(lat_cov[gi]).max())
    np.testing.assert_array_equal(joint, joint.T)
    _, ref_joint = V.combine(lat_mean, lat_cov, g.p, g.q, pr['jitters'], joint=True)
    e_joint = np.abs(joint - ref_joint).max() / np.abs(ref_joint).max()
    for i in range(g.p):
        np.testing.assert_array_equal(per[i], per[i].T)
        np.testing.assert_array_equal(per[i], joint[i * ns:(i + 1) * ns, i * ns:(i + 1) * ns])
    # duplicates of tstar carry the delta terms of K** between them: the two rows of C are the same row
    dup = [(a, b) for a in range(ns) for b in range(a + 1, ns) if ts[a] == ts[b]]
    assert len(dup) == 1
    a, b = dup[0]
    for gi in range(G):
        assert abs(lat[gi][a, b] - lat[gi][a, a]) <= 1e-12 * abs(lat_cov[gi]).max()
    print(name, ns, 'latent covariances off by', worst, 'joint by', e_joint, '(of the largest entry)')
    assert worst <= TOL and e_joint <= TOL
    assert ctx.option('state_ready') == 1
    _assert_default_schedule(ctx)


@pytest.mark.parametrize('name', ['n45', 'n129', 'seq_p2q3'])
def test_latent_covariances_at_the_data_times_are_the_sweeps_sigma(name):
    pr, mask, order, _, mu0, var0 = _problem(name)
    m = np.ones(pr['y_raw'].shape, dtype=bool) if mask is None else mask
    *_, sig_f, sig_w = R.sweep(*R.args(pr), mu0, var0, m, order, return_sigma=True)
    g, ctx = _swept(name)
    _, lat, _ = ctx.predict_cov(g.time, outputs=False)
    q, p = g.q, g.p
    worst = 0.0
    for j in range(q):
        worst = max(worst, np.abs(lat[j] - sig_f[j]).max() / np.abs(sig_f[j]).max())
        for i in range(p):
            worst = max(worst, np.abs(lat[q + j * p + i] - sig_w[j, i]).max() / np.abs(sig_w[j, i]).max())
    print(name, 'Sigma at the data times off by', worst, '(of the largest entry)')
    assert worst <= TOL


def test_predict_cov_of_the_object_carries_the_jitter_once():
    name, ns = 'n45', 129
    pr, mask, order, small_path, mu0, var0 = _problem(name)
    ts, lat_mean, lat_cov, _, _ = _reference(name, ns)
    g = _model(name, predict='variational')
    shape = (g.p + 1, g.q, g.N)
    g._mu, g._var = mu0.reshape(shape).copy(), var0.reshape(shape).copy()
    mean, var = g._Prediction(tstar=ts)
    kept = g._mu
    m2, cov, Cn, Cw = g.predict_cov(tstar=ts, separate=True)             # (no second sweep: the marker holds)
    assert g._mu is kept
    np.testing.assert_array_equal(m2, mean)
    diag = np.array([np.diag(c) for c in cov]).T
    np.testing.assert_allclose(diag, var, rtol=1e-12)
    _, ref_cov = V.combine(lat_mean, lat_cov, g.p, g.q, pr['jitters'])
    assert np.abs(cov - ref_cov).max() <= TOL * np.abs(ref_cov).max()
    assert Cn.shape == (g.q, ns, ns) and Cw.shape == (g.q * g.p, ns, ns)


# ------------------------------------------------------------------ 4. predict_draws
@pytest.mark.parametrize('name,ns', [('n45', 129), ('mid300', 150)])
def test_draws_with_fixed_normals(name, ns):
    """tests/test_predict_cov_gpu.py's identities in this form: latent - mean = L z with L L^T = C + nu I (L recovered from
    unit vectors, checked backwards against the device's own C), the outputs' combination, the reported nuggets."""
    g, ctx = _swept(name)
    pr = _problem(name)[0]
    ts = V.mixed_times(pr['time'], ns, seed=7)
    G = g.q * (g.p + 1)
    mean, C, _ = ctx.predict_cov(ts, outputs=False)
    lat0, _, nug0, info = ctx.predict_draws(ts, np.zeros((G, 1, ns)))
    assert info == 0
    latI, _, nug, info = ctx.predict_draws(ts, np.broadcast_to(np.eye(ns), (G, ns, ns)).copy())
    assert info == 0 and np.array_equal(nug, nug0)
    assert np.all(nug >= 1.25e-12) and np.all(nug <= 1.25e-6 * 1.0001)
    Ls = []
    for gi in range(G):
        np.testing.assert_array_equal(lat0[gi][0], mean[gi])
        L = (latI[gi] - lat0[gi]).T
        assert np.all(L[np.triu_indices(ns, 1)] == 0.0)
        A = C[gi] + nug[gi] * np.eye(ns)
        back = np.abs(L @ L.T - A).max() / np.abs(np.diag(A)).max()
        assert back <= 1e-12, (gi, back)
        Ls.append(L)
    z = np.random.default_rng(7).standard_normal((G, 3, ns))
    lat, out, nug2, info = ctx.predict_draws(ts, z)
    assert info == 0 and np.array_equal(nug2, nug)
    worst = 0.0
    for gi in range(G):
        expect = lat0[gi] + (Ls[gi] @ z[gi].T).T
        worst = max(worst, np.abs(lat[gi] - expect).max() / np.abs(expect).max())
    print(name, 'worst draw vs mean + L z', worst, 'nuggets', nug)
    assert worst <= 1e-12
    for i in range(g.p):
        s = sum(lat[g.q + j * g.p + i] * lat[j] for j in range(g.q))
        np.testing.assert_allclose(out[i], s, rtol=1e-13, atol=1e-13 * np.abs(s).max())
    assert ctx.option('state_ready') == 1
    _assert_default_schedule(ctx)


def test_sample_posterior_draws_the_noise_once():
    g = _model('n128', predict='variational')
    g.ELBOcalc(max_iter=20)
    ts = V.mixed_times(g.time, 129, seed=2)
    a = g.sample_posterior(tstar=ts, n=4, rng=11)
    b = g.sample_posterior(tstar=ts, n=4, rng=11, noise=True)
    assert a.shape == (4, 129, 1) and np.all(np.isfinite(a))
    noise = np.random.default_rng(11)
    noise.standard_normal((g.q * (g.p + 1), 4, 129))             # (the latent normals come first)
    np.testing.assert_allclose(b - a, noise.standard_normal(a.shape) * abs(g.jitters[0]), rtol=0, atol=1e-12)


# ------------------------------------------------------------------ 5. nothing is disturbed
@pytest.mark.parametrize('name', ['n45', 'n129', 'seq_p2q3'])
def test_a_prediction_disturbs_neither_the_gradient_nor_the_next_sweep(name):
    pr = _problem(name)[0]
    ts = V.mixed_times(pr['time'], 129, seed=1)
    out = []
    for predict in (False, True):
        g, ctx = _swept(name)
        n_par = sum(k.pars.size for k in list(g.nodes) + list(g.weights))
        if predict:
            ctx.predict(ts)
            ctx.predict_cov(ts, joint=True)
            ctx.predict_draws(ts, np.zeros((g.q * (g.p + 1), 2, ts.size)))
            assert ctx.option('state_ready') == 1
        grad = ctx.grad_elbo(n_par)
        if predict:
            ctx.predict(g.time)
        elbo, parts, info = ctx.sweep(2, commit=True)
        assert info == 0
        out.append((grad, elbo, parts) + ctx.get_muvar())
        _assert_default_schedule(ctx)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_a_second_prediction_needs_no_sweep():
    name = 'n129'
    pr = _problem(name)[0]
    t1, t2 = V.mixed_times(pr['time'], 300, seed=1), V.mixed_times(pr['time'], 129, seed=2)
    g, ctx = _swept(name)
    first = ctx.predict(t1)
    second = ctx.predict(t2)
    again = ctx.predict(t1)
    assert ctx.option('state_ready') == 1
    g2, ctx2 = _swept(name)
    fresh = ctx2.predict(t2)
    for a, b in zip(second, fresh):
        assert np.array_equal(a, b)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def test_the_reference_form_keeps_its_bits_around_the_option():
    name = 'n129'
    pr, mask, order, small_path, mu0, var0 = _problem(name)
    ts = V.mixed_times(pr['time'], 129, seed=3)
    g = _model(name)
    ctx = _device(g)
    assert ctx.option('predict_form') == _hip.PREDICT_REFERENCE

    def reference():
        ctx.set_muvar(mu0, var0)
        return ctx.predict(ts) + ctx.predict_cov(ts, joint=True)
    before = reference()
    assert ctx.option('state_ready') == 0
    assert ctx.option('predict_form', POST) == _hip.PREDICT_REFERENCE
    ctx.set_muvar(mu0, var0)
    ctx.sweep(1, commit=True)
    post = ctx.predict(ts)
    assert ctx.option('predict_form', _hip.PREDICT_REFERENCE) == POST
    after = reference()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert not np.allclose(post[1], before[1], rtol=1e-3)       # (the two forms are different quantities)
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ 6. validity and refusals
def test_validity_and_refusals(monkeypatch):
    lib = _hip.load_library()
    name = 'n45'
    pr, mask, order, small_path, mu0, var0 = _problem(name)
    g = _model(name)
    ctx = _device(g)
    dp = ctypes.POINTER(ctypes.c_double)
    ts = np.array([1.0, 2.0])
    m, v = np.zeros((g.q * (g.p + 1), 2)), np.zeros((g.q * (g.p + 1), 2))

    def predict():
        return lib.gprn_predict(ctx._h, 2, ts.ctypes.data_as(dp), m.ctypes.data_as(dp), v.ctypes.data_as(dp))
    # any other value
    for bad in (2, 7, -2, -5):
        assert lib.gprn_set_option(ctx._h, b'predict_form', bad, None) == _hip.GPRN_E_ARG
        assert b'predict_form' in lib.gprn_last_error(ctx._h)
    assert ctx.option('predict_form') == _hip.PREDICT_REFERENCE
    assert lib.gprn_set_option(ctx._h, b'state_ready', 1, None) == 0 and ctx.option('state_ready') == 0   # (read-only)
    # no committed sweep
    ctx.option('predict_form', POST)
    ctx.set_muvar(mu0, var0)
    assert predict() == _hip.GPRN_E_ARG
    assert b'needs a committed sweep' in lib.gprn_last_error(ctx._h)
    with pytest.raises(_hip.BackendError, match='needs a committed sweep'):
        ctx.predict_cov(ts)
    with pytest.raises(_hip.BackendError, match='needs a committed sweep'):
        ctx.predict_draws(ts, np.zeros((g.q * (g.p + 1), 1, 2)))
    ctx.sweep(1, commit=False)                                   # (an uncommitted sweep is none)
    assert predict() == _hip.GPRN_E_ARG
    ctx.sweep(1, commit=True)
    assert predict() == 0
    ctx.set_muvar(mu0, var0)                                     # (another state is staged: the sweep is gone)
    assert ctx.option('state_ready') == 0 and predict() == _hip.GPRN_E_ARG
    # an uploaded kernel
    K = np.asarray(pr['Kf'][0], dtype=float)
    ctx.upload_K(0, K)
    ctx.factor_priors()
    ctx.set_muvar(mu0, var0)
    ctx.sweep(1, commit=True)
    assert predict() == _hip.GPRN_E_UNSUPPORTED
    assert b'gprn_upload_K' in lib.gprn_last_error(ctx._h)
    # the posterior form, then a communicator
    ctx = _hip.Context(0)
    ctx.option('predict_form', POST)
    buf = ctypes.create_string_buffer(128)
    assert lib.gprn_comm_init(ctx._h, 2, 0, buf) == _hip.GPRN_E_UNSUPPORTED
    assert b'predict_form' in lib.gprn_last_error(ctx._h)
    ctx.close()
    # a communicator (one rank, for real), then the posterior form
    monkeypatch.setenv('GPRN_FORCE_RCCL', '1')
    ctx = _hip.Context(0)
    ctx.comm_init(1, 0, _hip.comm_unique_id())
    assert lib.gprn_set_option(ctx._h, b'predict_form', POST, None) == _hip.GPRN_E_UNSUPPORTED
    assert b'communicator' in lib.gprn_last_error(ctx._h)
    assert lib.gprn_set_option(ctx._h, b'predict_form', _hip.PREDICT_REFERENCE, None) == 0
    ctx.close()


# ------------------------------------------------------------------ 7. Python
def _count_sweeps(ctx):
    calls = []
    real = ctx.sweep

    def sweep(*a, **kw):
        calls.append((a, kw))
        return real(*a, **kw)
    ctx.sweep = sweep
    return calls


@pytest.mark.parametrize('name', ['n45', 'n129'])
def test_predict_sweeps_only_when_it_has_to(name):
    g = _model(name, predict='variational')
    pr = _problem(name)[0]
    ts = V.mixed_times(pr['time'], 129, seed=4)
    _, mu, var, _ = g.ELBOcalc(max_iter=200)
    assert g._mu is mu                                           # (converged: the stored state)
    calls = _count_sweeps(g._backend())
    mu_bits, var_bits = mu.copy(), var.copy()
    _, mean, sd, _ = g.predict(tstar=ts)
    g.predict_cov(tstar=ts)
    g.sample_posterior(tstar=ts, n=2, rng=0)
    assert calls == [] and g._mu is mu and g._var is var
    assert np.array_equal(g._mu, mu_bits) and np.array_equal(g._var, var_bits)
    # at the data times: the stored state, the imputation at the masked entries included
    m_data, v_data, parts = g._Prediction(separate=True)
    assert calls == []
    _cases.assert_state('varpred: predict at the data times %s' % name, np.concatenate(
        [np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)]), _rows(mu, g.p, g.q), tol=TOL)
    # new parameters: exactly one sweep, and the state it leaves is kept
    x = g.get_parameters()
    g.set_parameters(x * (1 + 1e-3))
    g.predict(tstar=ts)
    assert len(calls) == 1 and calls[0][1].get('commit') is True
    assert g._mu is not mu and g.last_info == 0
    g.predict(tstar=ts[:5])
    assert len(calls) == 1
    # an explicit state: one sweep from it, the stored state stays, and the next plain call sweeps again
    kept = g._mu
    g._Prediction(tstar=ts, mu=mu_bits, var=var_bits)
    assert len(calls) == 2 and g._mu is kept
    g.predict(tstar=ts)
    assert len(calls) == 3
    # the reference form on the same object: its own path, and the variational form sweeps again behind it
    g.predict_form = 'reference'
    m_ref, v_ref = g._Prediction(tstar=ts)
    assert len(calls) == 3
    g.predict_form = 'variational'
    m_var, v_var = g._Prediction(tstar=ts)
    assert len(calls) == 4
    assert not np.allclose(v_ref, v_var, rtol=1e-3)


def test_from_series_imputes_with_the_state():
    rng = np.random.RandomState(3)
    t1 = np.sort(rng.uniform(0.0, 50.0, 40))
    t2 = np.sort(np.concatenate([t1[::3], rng.uniform(0.0, 50.0, 25)]))
    series = [(t1, np.sin(t1 / 6.0) + 0.05 * rng.standard_normal(t1.size), np.full(t1.size, 0.1)),
              (t2, np.cos(t2 / 5.0) + 0.05 * rng.standard_normal(t2.size), np.full(t2.size, 0.1))]
    g = gpyrn.inference.from_series(1, series, predict='variational')
    assert g.predict_form == 'variational' and not g.mask.all()
    g.set_components(covfunc.QuasiPeriodic(1.0, 30.0, 20.0, 0.8),
                     [covfunc.SquaredExponential(1.0, 40.0), covfunc.SquaredExponential(0.9, 35.0)],
                     [meanfunc.Constant(0.0)] * 2, [0.2, 0.2])
    _, mu, var, _ = g.ELBOcalc(max_iter=200)
    mean, variance, parts = g._Prediction(separate=True)
    lat = np.concatenate([np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)])
    _cases.assert_state('varpred: from_series at the data times', lat, _rows(mu, g.p, g.q), tol=TOL)
    fit = np.einsum('iqn,qn->ni', mu[1:], mu[0])
    assert np.abs(mean - fit).max() <= TOL * np.abs(fit).max()
    _close_means(mean, fit, 'from_series')


def test_elboaux_behind_elbocalc_costs_one_sweep_and_the_result_is_right():
    """ELBOaux uploads its own matrices, stages another state and commits a sweep of its own: "state_ready" reads 1 behind it,
    and the object must know that this sweep is not the stored state's."""
    name = 'n128'
    pr, mask, order, small_path, mu0, var0 = _problem(name)
    assert mask is None                                          # (ELBOaux refuses a data mask)
    ts = V.mixed_times(pr['time'], 129, seed=6)
    g = _model(name, predict='variational')
    _, mu, var, _ = g.ELBOcalc(max_iter=200)
    assert g._mu is mu
    first = g._Prediction(tstar=ts)
    ctx = g._backend()
    jitt2 = np.asarray(pr['jitters'], dtype=float) ** 2
    g.ELBOaux(pr['Kf'], pr['Kw'], None, None, pr['y_resid'], jitt2, mu0, var0)
    assert ctx.option('state_ready') == 1 and g._mu is mu        # (a committed sweep -- of another state, uploaded kernels)
    calls = _count_sweeps(ctx)
    mean, variance = g._Prediction(tstar=ts)
    assert len(calls) == 1 and calls[0][1].get('commit') is True and g.last_info == 0
    g.predict_cov(tstar=ts)
    g.sample_posterior(tstar=ts, n=1, rng=0)
    assert len(calls) == 1
    # right: what a fresh object predicts from the same stored state, and the state itself at the data times
    g2 = _model(name, predict='variational')
    g2._mu, g2._var = mu.copy(), var.copy()
    mean2, variance2 = g2._Prediction(tstar=ts)
    np.testing.assert_allclose(variance, variance2, rtol=1e-10)
    _close_means(mean, mean2, 'behind ELBOaux')
    _cases.assert_state('varpred behind ELBOaux: the state kept', g._mu, g2._mu, g._var, g2._var, tol=1e-10)
    _, _, parts = g._Prediction(separate=True)
    _cases.assert_state('varpred behind ELBOaux at the data times', np.concatenate(
        [np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)]), _rows(g._mu, g.p, g.q), tol=TOL)
    assert np.all(np.isfinite(first[0])) and first[0].shape == mean.shape


def test_a_new_context_is_told_the_form():
    name = 'n45'
    pr = _problem(name)[0]
    ts = V.mixed_times(pr['time'], 129, seed=8)
    g = _model(name, predict='variational')
    g.ELBOcalc(max_iter=200)
    first = g._Prediction(tstar=ts)
    kept, kept_var = g._mu, g._var
    g._backend().close()
    g._ctx = None
    again = g._Prediction(tstar=ts)                              # (a new context: the option again, a set-up and one sweep)
    assert g._backend().option('predict_form') == POST and g._mu is not kept
    ref = _model(name)                                           # the reference form from the same state is another quantity
    ref._mu, ref._var = g._mu, g._var
    m_ref, v_ref = ref._Prediction(tstar=ts)
    assert not np.allclose(again[1], v_ref, rtol=1e-3)
    g3 = _model(name, predict='variational')                     # ... and it is what a fresh object predicts from that state
    g3._mu, g3._var = np.array(kept), np.array(kept_var)
    m3, v3 = g3._Prediction(tstar=ts)
    _close_means(again[0], m3, 'a new context')
    np.testing.assert_allclose(again[1], v3, rtol=1e-10)
    assert first[0].shape == again[0].shape
