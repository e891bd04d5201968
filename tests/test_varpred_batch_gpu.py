"""Prediction from each vector's own posterior at the end of a batch chunk (gprn_elbocalc_batch_predict,
Context.elbocalc_batch_predict, inference.predict_batch(from_sweeps=True)) on the GPU: against the dense restatement
tests/_varpred_ref.py at every slot's own kernels, against each slot's returned state, against the device one by one, across
chunks, and the contract of the entry point.

Shapes, the smallest at which each path can go wrong: (a) N = 45, p = q = 2, composite kernels with a WhiteNoise term, masked:
one ragged tile; (b) N = 128, p = q = 1: the last full one-tile size; (c) N = 129, p = 2, q = 1, masked: two tiles, the
worker; (d) mid_N300_p3q2, masked: three tiles; (e) step_p2q3, masked, in the sequential order with sequential_under_mask and
batch_under_mask; (f) mid_N300_p3q2 again in the sequential order: the ct kept behind the refresh above one tile.  Masked y / yerr are handed over as NaN / inf.  B = 4 vectors (5 where compaction is asked for, 20 where
the one-tile chunk of at least 16 has to be smaller than the list), 1-10 % perturbations of the fixtures' parameters.
ns in {1, 129, 300} from V.mixed_times: with ld = 128 / 256 / 384 one block, a ragged last block and several blocks.

Tolerances are the project's own: latent means and variances 1e-8 norm-wise per latent GP (tests/_cases.assert_state), output
variances 1e-8 relative, output means tests/test_varpred_gpu.py's _close_means rule.  No call may fall back to the event
schedule."""
import copy
import ctypes
import functools
from itertools import chain

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from oracle import cpu_ref
from tests import _cases, _mask_ref as M, _varpred_ref as V

pytestmark = pytest.mark.gpu
TOL = 1e-8
POST = _hip.PREDICT_POSTERIOR
NS = (1, 129, 300)
MAX_ITER = 200
SCALES = (1.01, 0.99, 1.05, 0.93)
# the compaction recipe of tests/test_mask_batch_gpu.py: cold starts at these scales stop at different trips
STOP_SCALES = (1.0, 1.01, 0.99, 1.05, 0.95)

# name -> (problem, mask seed or None, sweep order)
CASES = {
    'a': (lambda: V.synthetic(45, 2, 2, seed=1, composite=True), 2, 'reference'),
    'b': (lambda: V.synthetic(128, 1, 1, seed=2), None, 'reference'),
    'c': (lambda: V.synthetic(129, 2, 1, seed=3), 5, 'reference'),
    'd': (lambda: M.problem('mid_N300_p3q2'), 4, 'reference'),
    'e': (lambda: M.problem('step_p2q3'), 3, 'sequential'),
    # (e) runs on one tile, where nothing is kept: the kept ct behind the sequential order's refresh needs the worker
    'f': (lambda: M.problem('mid_N300_p3q2'), 4, 'sequential'),
}
FORMS = [('a', 'reference'), ('a', 'bound'), ('b', 'reference'), ('c', 'reference'), ('c', 'bound'), ('d', 'reference'),
         ('e', 'reference'), ('e', 'bound'), ('f', 'reference')]
ABOVE_ONE_TILE = ('c', 'd', 'f')


@functools.lru_cache(maxsize=None)
def _problem(name):
    make, seed, order = CASES[name]
    pr = make()
    p, N = pr['y_raw'].shape
    mask = M.partial_mask(p, N, seed) if seed is not None else None
    if mask is not None:
        assert not mask.all()
    mu0, var0 = V.init_state(pr, mask)
    return pr, mask, order, np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float)


def _model(name, **kw):
    pr, mask, order, _, _ = _problem(name)
    y, e = pr['y_raw'], np.sqrt(pr['yerr2'])
    if mask is not None:
        y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
    args = [a for i in range(y.shape[0]) for a in (y[i], e[i])]
    g = gpyrn.inference(len(pr['nodes']), pr['time'], *args, mask=mask, sweep_order=order, sequential_under_mask=True,
                        batch_under_mask=True, **kw)
    # (copies: set_parameters writes into the kernels, and the problem is shared between the tests)
    g.set_components(*copy.deepcopy((list(pr['nodes']), list(pr['weights']), list(pr['means']), list(pr['jitters']))))
    return g


def _sets(g, scales=SCALES):
    x0 = np.array(g.get_parameters(), dtype=float)
    return [x0 * s for s in scales]


def _inputs(g, sets, start):
    """The arrays gprn_elbocalc_batch_predict takes, vector by vector, every evaluation from `start` = (mu, var); the kernel
    programs of the first vector go to the device and the context is told to run batches under its mask."""
    ctx = g._backend()
    ctx.option('batch_mask', 1 if g.mask is not None else 0)
    y_raw = np.concatenate(g.y)
    kp, yr, jt, m0, v0 = [], [], [], [], []
    for i, x in enumerate(sets):
        g.set_parameters(np.array(x, dtype=float))
        nodes, weights, means, jitters = g._get_components()
        specs = [g._kernel_spec(k) for k in chain(nodes, weights)]
        assert all(sp[0] == 'device' for sp in specs)
        if i == 0:
            for gp, sp in enumerate(specs):
                g._send_spec(ctx, gp, sp)
            g._prior_key = None
        kp.append(np.concatenate([sp[2] for sp in specs]))
        yr.append(y_raw - g._mean(means))
        jt.append(np.asarray(jitters, dtype=float))
        m0.append(np.ravel(start[0]))
        v0.append(np.ravel(start[1]))
    return ctx, np.array(kp), np.array(yr), np.array(jt), np.array(m0), np.array(v0)


def _rows(state, p, q):
    s = np.asarray(state)
    return np.array([s[0, j] for j in range(q)] + [s[1 + i, j] for j in range(q) for i in range(p)])


def _close_means(mean, ref, what):
    """tests/test_varpred_gpu.py's rule: |mean - ref| <= 1e-8 max(|ref|, 1e-3 max |ref| of that output); (ns, p) arrays."""
    floor = 1e-3 * np.abs(ref).max(axis=0, keepdims=True)
    rel = float((np.abs(mean - ref) / np.maximum(np.abs(ref), floor)).max())
    print(what, 'output means off by', rel, '(element-wise relative, floored)')
    assert rel <= TOL


def _mean_combination(lat_mean, p, q):
    """sum_j f_j w_ji from latent means (G, ns), without the mean functions: (ns, p) (V.combine's mean)."""
    f, w = lat_mean[:q], lat_mean[q:].reshape(q, p, lat_mean.shape[1])
    return np.array([sum(w[j, i] * f[j] for j in range(q)) for i in range(p)]).T


def _times(name, ns):
    return V.mixed_times(_problem(name)[0]['time'], ns, seed=ns)


@functools.lru_cache(maxsize=None)
def _restated(name, ns):
    """Per vector of _sets: the restatement's latent means and variances (G, ns) at the mixed times after ONE sweep from the
    initial state at THAT vector's kernels, means and jitters, and its jitters.  Computed once, shared, never written."""
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name)
    ts = _times(name, ns)
    out = []
    for x in _sets(g):
        g.set_parameters(x.copy())
        nodes, weights, means, jit = g._get_components()
        Kf, Kw, _, _, yres, jitt2 = cpu_ref.setup(np.asarray(pr['time']), nodes, weights, means, jit, pr['y_raw'])
        inputs, _, _ = V.latent_inputs(Kf, Kw, yres, pr['y_raw'], pr['yerr2'], jitt2, mu0, var0, mask, order)
        lat_mean, lat_cov = V.predict_latent(list(nodes) + list(weights), pr['time'], ts, inputs)
        lat_var = np.einsum('gnn->gn', lat_cov).copy()
        for a in (lat_mean, lat_var):
            a.setflags(write=False)
        out.append((lat_mean, lat_var, tuple(float(j) for j in jit)))
    return out


# ------------------------------------------------------------------ 1. every slot against the restatement
@pytest.mark.parametrize('name,elbo', FORMS)
def test_every_slot_of_a_forced_batch_matches_the_restatement(name, elbo):
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name, elbo=elbo)
    sets = _sets(g)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, (mu0, var0))
    for ns in NS:
        ts = _times(name, ns)
        res = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 1, ts, forced=True)
        assert res is not None, 'the library has no batched form for this problem'
        elbo_v, iters, conv, info, mu, var, lm, lv, om, ov = res
        assert not info.any() and (iters == 1).all() and not conv.any()
        assert lm.shape == (len(sets), g.q * (g.p + 1), ns) and om.shape == (len(sets), g.p, ns)
        for b, (ref_mean, ref_var, jit) in enumerate(_restated(name, ns)):
            what = 'varpred_batch %s %s ns = %d slot %d' % (name, elbo, ns, b)
            _cases.assert_state(what, lm[b], ref_mean, lv[b], ref_var, tol=TOL)
            out_mean = _mean_combination(ref_mean, g.p, g.q)
            out_var = V.variances(ref_mean, ref_var, g.p, g.q, jit)
            e_var = float(np.abs(ov[b].T / out_var - 1).max())
            print(what, 'latent', _cases.ACHIEVED[-1][1:], 'output variances off by', e_var, '(relative)')
            assert e_var <= TOL
            _close_means(om[b].T, out_mean, what)
            assert np.all(ov[b] >= np.asarray(jit)[:, None] ** 2 * (1 - 1e-12))     # (the jitter is there, once)
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 2. data times give each slot's state
@pytest.mark.parametrize('name,elbo', FORMS)
def test_data_times_give_each_slots_state(name, elbo):
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name, elbo=elbo)
    sets = _sets(g, STOP_SCALES)
    # (c has q = 1: from its own initial state every vector stops at the rule's minimum of 4 trips, so it starts from twice
    # the initial means, where the five vectors take 6 to 11 trips)
    start = (2.0 * mu0, var0) if name == 'c' else (mu0, var0)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, start)
    res = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, MAX_ITER, np.asarray(g.time, dtype=float), outputs=False)
    elbo_v, iters, conv, info, mu, var, lm, lv, om, ov = res
    assert not info.any() and om is None and ov is None
    print('varpred_batch data times %s %s: trips %s' % (name, elbo, iters.tolist()))
    if name in ABOVE_ONE_TILE:
        assert len(set(iters.tolist())) >= 2              # (evaluations leave the tables at different trips: compaction)
    if mask is not None:
        assert (~mask).sum() > 0                          # (rows of zero precision)
    for b in range(len(sets)):
        _cases.assert_state('varpred_batch at the data times %s %s slot %d (%d trips)' % (name, elbo, b, iters[b]),
                            lm[b], _rows(mu[b], g.p, g.q), lv[b], _rows(var[b], g.p, g.q), tol=TOL)
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 3. against the device one by one
@pytest.mark.parametrize('name', list(CASES))
def test_against_the_device_one_by_one(name):
    pr, mask, order, mu0, var0 = _problem(name)
    g, g1 = _model(name), _model(name)
    sets = _sets(g)
    ts = _times(name, 300)
    g1.set_parameters(np.array(g.get_parameters(), dtype=float))
    _, mu_w, var_w, _ = g1.ELBOcalc(mu=mu0.copy(), var=var0.copy(), max_iter=MAX_ITER)
    for what, start in (('cold', (mu0, var0)), ('warm', (np.asarray(mu_w), np.asarray(var_w)))):
        ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, start)
        elbo_v, iters, conv, info, mu, var, lm, lv, om, ov = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, MAX_ITER, ts)
        assert not info.any()
        for b, x in enumerate(sets):
            g1.set_parameters(x.copy())
            nodes, weights, means, jitters = g1._get_components()
            c1 = g1._setup_device(nodes, weights, means, jitters)
            assert g1.last_info == 0
            c1.option('predict_form', POST)
            c1.set_muvar(np.array(start[0], dtype=float), np.array(start[1], dtype=float))
            hist, it1, conv1, info1, mu1, var1 = c1.elbocalc(MAX_ITER)
            assert info1 == 0 and it1 == iters[b] and bool(conv1) == bool(conv[b])
            gm, gv, _ = c1.predict(ts)
            _cases.assert_state('varpred_batch against one by one %s %s slot %d' % (name, what, b), lm[b], gm, lv[b], gv, tol=TOL)
            out_var = V.variances(gm, gv, g.p, g.q, jitters)
            assert float(np.abs(ov[b].T / out_var - 1).max()) <= TOL
            out_mean = _mean_combination(gm, g.p, g.q)
            _close_means(om[b].T, out_mean, 'varpred_batch against one by one %s %s slot %d' % (name, what, b))
            assert c1.option('fallbacks') == 0
        print('varpred_batch_vs_one_by_one %s %s: trips %s, worst latent %s' % (
            name, what, iters.tolist(), max(a[1] for a in _cases.ACHIEVED[-len(sets):])))
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 4. chunks
# a: the one-tile chunk holds 16 at least, so 20 vectors; c: about 9 MB of slabs per evaluation; d: about 44 MB
@pytest.mark.parametrize('name,B,budget_mb', [('a', 20, 1), ('c', 5, 30), ('d', 5, 100)])
def test_chunks_give_the_unchunked_rows(name, B, budget_mb):
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * STOP_SCALES[k % 5] * (1.0 + 0.002 * (k // 5)) for k in range(B)]
    ts = _times(name, 129)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, (mu0, var0))
    whole = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 3, ts, forced=True)
    assert ctx.option('batch_chunk') == B
    ctx.option('batch_mem_mb', budget_mb)
    parts = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 3, ts, forced=True)
    chunk = ctx.option('batch_chunk')
    print('varpred_batch chunks %s: %d of %d per chunk' % (name, chunk, B))
    assert 1 <= chunk < B
    assert not whole[3].any() and not parts[3].any()
    for a, b in zip(whole[6:], parts[6:]):
        scale = np.abs(a).max(axis=-1, keepdims=True)
        assert float((np.abs(a - b) / scale).max()) <= 1e-12
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 5. bits
@pytest.mark.parametrize('name,elbo', [('a', 'reference'), ('c', 'bound'), ('e', 'reference')])
def test_the_loops_outputs_keep_their_bits(name, elbo):
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name, elbo=elbo)
    sets = _sets(g, STOP_SCALES)
    ts = _times(name, 129)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, (mu0, var0))
    for forced, trips in ((True, 2), (False, MAX_ITER)):
        plain = ctx.elbocalc_batch(kp, yr, jt, m0, v0, trips, want_state=True, forced=forced)
        res = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, trips, ts, forced=forced)
        for a, b in zip(plain, res[:6]):
            assert np.array_equal(a, b)
        again = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, trips, ts, forced=forced)
        for a, b in zip(res, again):
            assert np.array_equal(a, b)
        only = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, trips, ts, forced=forced, latent=False)
        assert only[6] is None and only[7] is None
        assert np.array_equal(only[8], res[8]) and np.array_equal(only[9], res[9])
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 6. a failed pivot in the middle
@pytest.mark.parametrize('name', ['a', 'd'])
def test_a_failed_pivot_in_the_middle_of_a_batch(name):
    """tests/test_grad_batch_gpu.py's construction: a NaN jitter, so no pivot of B is positive -- a numerical verdict, not a
    device fault.  The call without the bad vector has a good one in its place (the same launch shapes)."""
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name)
    sets = _sets(g, STOP_SCALES)
    bad = [x.copy() for x in sets]
    bad[2][-1] = np.nan
    ts = _times(name, 129)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, (mu0, var0))
    good = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 6, ts)
    assert not good[3].any()
    ctx, kp, yr, jt, m0, v0 = _inputs(g, bad, (mu0, var0))
    got = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 6, ts)
    assert got[3][2] > 0 and np.isnan(got[0][2])
    for rows in got[6:]:
        assert np.all(np.isnan(rows[2]))
    keep = [0, 1, 3, 4]
    assert not got[3][keep].any()
    for a, b in zip(good, got):
        assert np.array_equal(a[keep], b[keep])
    for rows in got[6:]:
        assert np.all(np.isfinite(rows[keep]))
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 7. the context is untouched
@pytest.mark.parametrize('name', ['a', 'c'])
def test_the_context_is_untouched(name):
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name)
    x = np.array(g.get_parameters(), dtype=float)
    _, kp, yr, jt, m0, v0 = _inputs(g, _sets(g), (mu0, var0))
    g.set_parameters(x.copy())
    ts = _times(name, 129)
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    ctx.option('predict_form', POST)

    def swept():
        ctx.set_muvar(mu0, var0)
        e, parts, info = ctx.sweep(1, commit=True)
        assert info == 0
        return [np.asarray(e), np.asarray(parts)] + list(ctx.get_muvar())

    before = swept()
    assert ctx.option('state_ready') == 1
    first = ctx.predict(ts)
    res = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 3, ts)
    assert not res[3].any()
    assert ctx.option('state_ready') == 1
    for a, b in zip(first, ctx.predict(ts)):                  # (the committed sweep's X, s and ct are where they were)
        assert np.array_equal(a, b)
    for a, b in zip(before, swept()):
        assert np.array_equal(a, b)
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 8. refusals and argument errors
def _raw_call(ctx, kp, yr, jt, m0, v0, max_iter, ts, flags=0, latent=True, outputs=True, ns=None):
    B, G, p = kp.shape[0], ctx.G, ctx.p
    dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    arrs = [np.ascontiguousarray(a, dtype=float) for a in (kp, yr, jt, m0, v0, ts)]
    elbo = np.zeros(B)
    it, cv, info = (np.zeros(B, dtype=np.int32) for _ in range(3))
    lm, lv = (np.zeros((B, G, ts.size)) if latent else None for _ in range(2))
    om, ov = (np.zeros((B, p, ts.size)) if outputs else None for _ in range(2))
    return ctx._lib.gprn_elbocalc_batch_predict(ctx._h, B, dp(arrs[0]), kp.shape[1], dp(arrs[1]), dp(arrs[2]), dp(arrs[3]),
                                                dp(arrs[4]), max_iter, flags, ts.size if ns is None else ns, dp(arrs[5]),
                                                dp(elbo), ip(it), ip(cv), ip(info), None, None, dp(lm), dp(lv), dp(om), dp(ov))


def test_refusals_and_argument_errors():
    name = 'a'
    pr, mask, order, mu0, var0 = _problem(name)
    g = _model(name)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, _sets(g), (mu0, var0))
    ts = _times(name, 129)
    lib = ctx._lib
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == 0
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 0, ts) == _hip.GPRN_E_ARG                  # no sweep is committed
    assert b'committed sweep' in lib.gprn_last_error(ctx._h)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, ns=0) == _hip.GPRN_E_ARG
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, latent=False, outputs=False) == _hip.GPRN_E_ARG
    assert b'neither' in lib.gprn_last_error(ctx._h)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, flags=2) == _hip.GPRN_E_ARG         # an unknown flag
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, flags=_hip.GPRN_BATCH_FORCED, outputs=False) == 0
    ctx.option('batch_mask', 0)                                                          # a mask without "batch_mask"
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == _hip.GPRN_E_UNSUPPORTED
    assert b'mask' in lib.gprn_last_error(ctx._h)
    ctx.option('batch_mask', 1)
    ctx.option('small_path', 0)                                                          # one tile, the small path off
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == _hip.GPRN_E_UNSUPPORTED
    assert b'small path' in lib.gprn_last_error(ctx._h)
    assert ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 2, ts) is None
    ctx.option('small_path', 1)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == 0
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 9. Python
def _series_model(**kw):
    rng = np.random.RandomState(3)
    t1 = np.sort(rng.uniform(0.0, 50.0, 40))
    t2 = np.sort(np.concatenate([t1[::3], rng.uniform(0.0, 50.0, 25)]))
    series = [(t1, np.sin(t1 / 6.0) + 0.05 * rng.standard_normal(t1.size), np.full(t1.size, 0.1)),
              (t2, np.cos(t2 / 5.0) + 0.05 * rng.standard_normal(t2.size), np.full(t2.size, 0.1))]
    g = gpyrn.inference.from_series(2, series, predict='variational', sweep_order='sequential', sequential_under_mask=True,
                                    batch_under_mask=True, **kw)
    g.set_components([covfunc.QuasiPeriodic(1.0, 30.0, 20.0, 0.8), covfunc.SquaredExponential(0.5, 25.0)],
                     [covfunc.SquaredExponential(1.0, 40.0), covfunc.SquaredExponential(0.9, 35.0),
                      covfunc.SquaredExponential(0.4, 45.0), covfunc.SquaredExponential(0.3, 30.0)],
                     [meanfunc.Constant(0.1), meanfunc.Constant(-0.2)], [0.2, 0.25])
    return g


def test_python_from_sweeps_on_series_with_their_own_grids():
    g = _series_model()
    assert g.predict_form == 'variational' and not g.mask.all() and g.q == 2
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * s for s in SCALES]
    ts = V.mixed_times(g.time, 129, seed=1)
    mean, var, lat = g.predict_batch(sets, tstar=ts, from_sweeps=True, separate=True, max_iter=60)
    assert mean.shape == (4, 129, g.p) and var.shape == mean.shape and lat.shape == (4, g.q * (g.p + 1), 129)
    assert g.last_info == 0 and np.all(np.isfinite(mean)) and np.all(var > 0)
    np.testing.assert_allclose(g.get_parameters(), sets[-1])
    w = np.array([1.0, 2.0, 3.0, 4.0])
    g3 = _series_model()                                      # (fresh objects: both start every vector cold)
    pm, pv = g3.posterior_predictive(sets, tstar=ts, weights=w, from_sweeps=True, max_iter=60)
    g2 = _series_model()
    m2, v2 = g2.predict_batch(sets, tstar=ts, from_sweeps=True, max_iter=60)
    np.testing.assert_array_equal(m2, mean)
    wn = (w / w.sum())[:, None, None]
    ref_m = np.sum(wn * m2, axis=0)
    np.testing.assert_allclose(pm, ref_m, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(pv, np.sum(wn * (v2 + m2 * m2), axis=0) - ref_m * ref_m, rtol=1e-7)
    assert g._backend().option('fallbacks') == 0


def test_python_side_by_side_and_one_by_one_agree():
    g, g1 = _series_model(), _series_model()
    g1.batch_max_N = 0                                        # (N above batch_max_N: the one-by-one branch)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * s for s in SCALES]
    ts = V.mixed_times(g.time, 129, seed=2)
    nodes, weights, means, jitters = g._get_components()
    start = g._initMuVar(nodes, weights, jitters)
    a = g.predict_batch(sets, tstar=ts, from_sweeps=True, sweeps=2, start=start, separate=True)
    b = g1.predict_batch(sets, tstar=ts, from_sweeps=True, sweeps=2, start=start, separate=True)
    assert g.last_info == 0 and g1.last_info == 0
    for k in range(len(sets)):
        _cases.assert_state('varpred_batch python, side by side against one by one, vector %d' % k, a[2][k], b[2][k], tol=TOL)
        assert float(np.abs(a[1][k] / b[1][k] - 1).max()) <= TOL
        _close_means(a[0][k], b[0][k], 'python vector %d' % k)
    np.testing.assert_allclose(g.get_parameters(), sets[-1])
    np.testing.assert_allclose(g1.get_parameters(), sets[-1])
    assert g._backend().option('fallbacks') == 0 and g1._backend().option('fallbacks') == 0


def test_python_adds_the_mean_functions_per_vector():
    """Two vectors that differ only in a Constant mean: what each output mean carries on top of sum_j f_j w_ji -- rebuilt here
    from the latent rows of the same call -- is exactly that vector's own constant."""
    g = _series_model()
    names = list(g.parameters_dict.keys())
    x0 = np.array(g.get_parameters(), dtype=float)
    n_k = sum(k.pars.size for k in chain(g.nodes, g.weights))
    x1 = x0.copy()
    x1[n_k] += 0.75                                           # (the Constant of output 0)
    assert len(names) == x0.size
    ts = V.mixed_times(g.time, 129, seed=3)
    nodes, weights, means, jitters = g._get_components()
    start = g._initMuVar(nodes, weights, jitters)
    mean, var, lat = g.predict_batch([x0, x1], tstar=ts, from_sweeps=True, sweeps=2, start=start, separate=True)
    q, p = g.q, g.p
    for b, x in enumerate((x0, x1)):
        for i in range(p):
            fit = sum(lat[b][j] * lat[b][q + j * p + i] for j in range(q))
            scale = max(1.0, np.abs(fit).max())
            assert np.abs(mean[b][:, i] - fit - x[n_k + i]).max() <= 1e-13 * scale
    assert x1[n_k] - x0[n_k] == 0.75
