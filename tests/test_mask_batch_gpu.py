"""Side-by-side ELBO batches under a data mask (option "batch_mask", inference(..., batch_under_mask=True)): every slot of a
forced batch against the dense restatement tests/_mask_ref.py on both paths, perturbed vectors under the stop rule across
chunks and through compaction against the device one by one, garbage in the masked entries, gradients, the switch itself
and an mcmc run on series with their own time grids.  No call may fall back to the event schedule."""
import ctypes
import os
from itertools import chain

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from oracle import cpu_ref
from tests import _cases, _grad_ref as GR, _mask_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-8                   # the project's plain bound
PAIR_RTOL = 1e-9              # two device results from the same start (test_nelbo_batch_side_by_side_above_one_tile's bound)
PAIR_BOUND = 2e-8             # gradient entries of two device results (tests/test_grad_batch_gpu.py)
SCALES = (1.0, 1.01, 0.99, 1.05, 0.95, 1.2, 0.8)
MAX_ITER = 200


def _model(tag, time, y, yerr, mask, **kw):
    meta, _ = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    args = [a for i in range(y.shape[0]) for a in (y[i], yerr[i])]
    g = gpyrn.inference(meta['q'], time, *args, mask=mask, **kw)
    g.set_components(nodes, weights, means, jit)
    return g


def _partial(tag, seed, mask=None, **kw):
    """The fixture under a partial mask, the masked y / yerr handed over as NaN / inf: (problem, mask, model)."""
    pr = R.problem(tag)
    p, N = pr['y_raw'].shape
    mask = R.partial_mask(p, N, seed) if mask is None else mask
    y = np.where(mask, pr['y_raw'], np.nan)
    e = np.where(mask, np.sqrt(pr['yerr2']), np.inf)
    return pr, mask, _model(tag, pr['time'], y, e, mask, **kw)


def _inputs(g, sets, start):
    """The arrays gprn_elbocalc_batch takes, vector by vector, every evaluation from `start` = (mu, var); the kernel programs
    of the first vector go to the device and the context is told to run batches under its mask."""
    ctx = g._backend()
    ctx.option('batch_mask', 1)
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


def _problem_at(g):
    """tests/_mask_ref.problem's dict for the model `g` at its CURRENT parameters."""
    t = np.asarray(g.time, dtype=float)
    nodes, weights, means, jit = g._get_components()
    Kf, Kw, _, _, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, g.y)
    return dict(nodes=nodes, weights=weights, means=means, jitters=jit, time=t, Kf=Kf, Kw=Kw, y_resid=yres, y_raw=g.y,
                yerr2=g.yerr2, jitt2=jitt2)


# ------------------------------------------------------------------ 1. every slot of a forced batch is the restatement
def _forced_batch(g, pr, mask, nsweeps, B=5):
    mu0, var0 = R.init_state(pr, mask)
    x = np.array(g.get_parameters(), dtype=float)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, [x] * B, (mu0, var0))
    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, nsweeps, want_state=True, forced=True)
    assert res is not None, 'the library has no batched form for this problem'
    elbo, iters, conv, info, mu, var = res
    assert not info.any() and (iters == nsweeps).all() and not conv.any()
    assert ctx.option('fallbacks') == 0
    E, P, mu_r, var_r = R.sweeps(pr['Kf'], pr['Kw'], pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2'], mu0, var0, mask,
                                 nsweeps)
    assert np.all(np.isfinite(E)) and np.all(var_r > 0)
    print('mask_batch forced: ELBO rel %.2e' % np.abs(elbo / E[-1] - 1).max())
    np.testing.assert_allclose(elbo, np.full(B, E[-1]), rtol=RTOL)
    shape = mu[0].shape
    for b in range(B):
        _cases.assert_state('masked batch slot %d of %d' % (b, B), mu[b], mu_r.reshape(shape), var[b], var_r.reshape(shape))
        assert np.array_equal(mu[b], mu[0]) and np.array_equal(var[b], var[0]) and elbo[b] == elbo[0]
    return elbo, mu, var


# (a) one tile, q = 1 and 2, 6-7 masked per output; (d) three tiles, masked counts 87 / 53 / 87
@pytest.mark.parametrize('tag,seed', [('step_p2q1', 1), ('step_p3q2', 2), ('mid_N300_p3q2', 4)])
def test_every_slot_of_a_forced_batch_under_a_partial_mask(tag, seed):
    pr, mask, g = _partial(tag, seed)
    if tag == 'mid_N300_p3q2':
        assert (~mask).sum(axis=1).tolist() == [87, 53, 87]
    _forced_batch(g, pr, mask, pr['meta']['nsweeps'])


# (b) N = 128, the last one-tile size, 96 all-masked times: the NODE has a U; (c) N = 129: two tiles, 97 all-masked times
@pytest.mark.parametrize('tag,kw,N', [('step_p1q1', dict(per_gap=3), 128), ('step_p2q1', dict(per_gap=3), 128),
                                      ('step_p1q1', dict(per_gap=3, n_after=2), 129),
                                      ('step_p2q1', dict(per_gap=3, n_after=2), 129)])
def test_every_slot_of_a_forced_batch_with_all_masked_times(tag, kw, N):
    pr, mask, pos = R.inserted(tag, **kw)
    meta, d = pr['meta'], pr['d']
    assert mask.shape[1] == N and (~mask.any(axis=0)).sum() == N - pos.size == N - 32
    g = _model(tag, pr['time'], pr['y_nan'], pr['yerr_inf'], mask)
    elbo, mu, var = _forced_batch(g, pr, mask, meta['nsweeps'])
    # at the original positions: the reference's own sweeps (test_inserted_all_masked_times_reproduce_the_reference)
    np.testing.assert_allclose(elbo, np.full(elbo.size, d['elbo_sweeps'][-1]), rtol=RTOL)
    for b in range(elbo.size):
        _cases.assert_state('masked batch, inserted ' + tag, mu[b][..., pos], d['mu_final'], var[b][..., pos], d['var_final'])


def test_every_slot_of_a_forced_batch_with_two_row_tiles_of_U():
    """(e) N = 512, masked counts 160 / 214 / 170: the rows U of a weight fill two row tiles.  Two forced sweeps; the
    restatement gives ELBO -2493.99 and -1879.18."""
    tag = 'mid_N512_p3q2'
    mask = R.partial_mask(3, 512, 5, lo=0.30, hi=0.45)
    assert (~mask).sum(axis=1).tolist() == [160, 214, 170] and (~mask).sum(axis=1).min() > 128
    pr, mask, g = _partial(tag, 5, mask=mask)
    _forced_batch(g, pr, mask, 2, B=5)


# ------------------------------------------------------------------ 2. perturbed vectors, stop rule, chunks, compaction
def _perturbed(x0, B):
    """x0 * s for the seven scales; beyond seven the scales again with a second perturbation of 0.2 % per round."""
    return [x0 * SCALES[k % len(SCALES)] * (1.0 + 0.002 * (k // len(SCALES))) for k in range(B)]


def _one_by_one(g1, sets, start):
    out = []
    for x in sets:
        g1.set_parameters(np.array(x, dtype=float))
        e, mu, var, it = g1.ELBOcalc(max_iter=MAX_ITER, mu=np.array(start[0], dtype=float), var=np.array(start[1], dtype=float))
        assert g1.last_info == 0
        out.append((float(e), np.asarray(mu), np.asarray(var), int(it)))
    assert g1._backend().option('fallbacks') == 0
    return out


def _side_by_side(g, sets, start, budget_mb):
    ctx = g._backend()
    ctx.option('batch_mem_mb', budget_mb)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, start)
    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True)
    assert res is not None
    assert 1 <= ctx.option('batch_chunk') < len(sets)
    assert not res[3].any() and ctx.option('fallbacks') == 0
    return res


# step_p3q2: a one-tile chunk holds 16 at least, so 20 vectors; mid_N300_p3q2: about 44 MB of slabs per evaluation, chunks of 2
CHUNKED = [('step_p3q2', 2, 20, 1), ('mid_N300_p3q2', 4, 7, 100)]


@pytest.mark.parametrize('tag,seed,B,budget_mb', CHUNKED)
def test_perturbed_vectors_under_the_stop_rule_across_chunks(tag, seed, B, budget_mb):
    """Cold from the restatement's start state at x0, then warm from the converged state at x0, against the same evaluations
    one by one on a second object under the same mask.  The restatement's cold trip counts of the seven scales: step_p3q2
    16, 16, 16, 16, 15, 15, 11; mid_N300_p3q2 19, 18, 19, 14, 20, 13, 26 -- evaluations leave the batch at different trips."""
    pr, mask, g = _partial(tag, seed)
    _, _, g1 = _partial(tag, seed)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = _perturbed(x0, B)
    cold = R.init_state(pr, mask)
    g1.set_parameters(x0.copy())
    _, mu_w, var_w, _ = g1.ELBOcalc(mu=np.array(cold[0]), var=np.array(cold[1]))
    for what, start in (('cold', cold), ('warm', (mu_w, var_w))):
        elbo, iters, conv, info, mu, var = _side_by_side(g, sets, start, budget_mb)
        ones = _one_by_one(g1, sets, start)
        worst = max(abs(elbo[b] / ones[b][0] - 1) for b in range(B))
        print('mask_batch_vs_one_by_one %s %s: worst value %.2e, trips %s' % (tag, what, worst, iters.tolist()))
        if what == 'cold':
            assert len(set(iters.tolist())) > 1
        for b in range(B):
            np.testing.assert_allclose(elbo[b], ones[b][0], rtol=PAIR_RTOL)
            assert iters[b] == ones[b][3]
            _cases.assert_state('masked batch %s %s, vector %d' % (tag, what, b), mu[b], ones[b][1], var[b], ones[b][2])


# ------------------------------------------------------------------ 3. garbage in masked entries
@pytest.mark.parametrize('tag,seed,B,budget_mb', CHUNKED)
def test_garbage_in_masked_entries_never_reaches_arithmetic(tag, seed, B, budget_mb):
    pr = R.problem(tag)
    p, N = pr['y_raw'].shape
    mask = R.partial_mask(p, N, seed)
    y, e = pr['y_raw'], np.sqrt(pr['yerr2'])
    start = R.init_state(pr, mask)
    got = []
    for fill_y, fill_e in ((0.0, 1.0), (np.nan, np.inf)):
        g = _model(tag, pr['time'], y, e, mask)
        # INTO the device's y, y - mean and variances at the masked entries (the host layer would have replaced them)
        g.y = np.where(mask, g.y, fill_y)
        g.yerr = np.where(mask, g.yerr, fill_e)
        sets = _perturbed(np.array(g.get_parameters(), dtype=float), B)
        got.append(_side_by_side(g, sets, start, budget_mb))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
        assert np.all(np.isfinite(a))


# ------------------------------------------------------------------ 4. gradients
@pytest.mark.parametrize('tag,seed,scales', [('step_p3q2', 2, SCALES[:5]), ('mid_N300_p3q2', 4, SCALES[:3])])
def test_gradients_side_by_side_under_a_mask(tag, seed, scales):
    """nELBO_and_grad_batch with batch_under_mask=True against the same method's one-by-one branch on an object without it:
    each vector's loop from the same state, then gprn_grad_elbo on what it left -- the gradient code of
    nELBO_and_grad(fused=True), whose own call takes one MORE sweep before the gradient and so is not the batch's row.  The
    first forced slot also against the dense restatement tests/_grad_ref.py under the mask."""
    pr, mask, g = _partial(tag, seed, batch_under_mask=True)
    _, _, g1 = _partial(tag, seed)
    assert g._batchable() and not g1._batchable()
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * s for s in scales]
    n_k = sum(k.pars.size for k in chain(g.nodes, g.weights))
    is_k = np.arange(x0.size) < n_k
    is_j = np.arange(x0.size) >= x0.size - g.p
    start = R.init_state(pr, mask)
    g1.set_parameters(x0.copy())
    _, mu_w, var_w, _ = g1.ELBOcalc(mu=np.array(start[0]), var=np.array(start[1]))
    for what in ('forced', 'stop rule'):
        if what == 'forced':
            vals, grads = g.nELBO_and_grad_batch(sets, sweeps=2, start=start)
            vals1, grads1 = g1.nELBO_and_grad_batch(sets, sweeps=2, start=start)
        else:
            g._mu, g._var = mu_w.copy(), var_w.copy()
            g1._mu, g1._var = mu_w.copy(), var_w.copy()
            vals, grads = g.nELBO_and_grad_batch(sets, max_iter=MAX_ITER)
            vals1, grads1 = g1.nELBO_and_grad_batch(sets, max_iter=MAX_ITER)
        assert g.last_info == 0 and g1.last_info == 0 and g._backend().option('batch_chunk') > 1
        assert np.all(np.isfinite(vals)) and np.all(np.isfinite(grads))
        np.testing.assert_allclose(vals, vals1, rtol=PAIR_RTOL)
        # the scale of a kernel entry: the restatement's sum |G| |dK/dtheta| (at x0, one sweep from the start; the vectors are
        # within 5 % of it) -- and for the forced mode the restatement's own gradient of the first vector
        g1.set_parameters(x0.copy())
        prx = _problem_at(g1)
        st = GR.sweep_state(prx, np.asarray(start[0]), np.asarray(start[1]), mask)
        if what == 'forced':
            st = GR.sweep_state(prx, st['mu'], st['var'], mask)
        ref, norm = GR.kernel_gradient(prx, st, 'chol')
        worst = float((np.abs(grads - grads1)[:, is_k] / norm[None]).max())
        print('mask_batch_grad %s %s: kernel entries differ by %.2e of their scale' % (tag, what, worst))
        assert worst <= PAIR_BOUND
        np.testing.assert_allclose(grads[:, is_j], grads1[:, is_j], rtol=1e-10)
        if what == 'forced':
            dense = float((np.abs(-grads[0][is_k] - ref) / norm).max())
            print('mask_batch_grad %s forced slot 0 against the restatement: %.2e' % (tag, dense))
            assert dense <= RTOL
            np.testing.assert_allclose(-vals[0], st['elbo'], rtol=RTOL)
    assert g._backend().option('fallbacks') == 0 and g1._backend().option('fallbacks') == 0


# ------------------------------------------------------------------ 5. the switch
def _raw_batch(ctx, kp, yr, jt, m0, v0, max_iter):
    B = kp.shape[0]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    arrs = [np.ascontiguousarray(a, dtype=float) for a in (kp, yr, jt, m0, v0)]
    elbo = np.zeros(B)
    it, cv, info = (np.zeros(B, dtype=np.int32) for _ in range(3))
    return ctx._lib.gprn_elbocalc_batch(ctx._h, B, dp(arrs[0]), kp.shape[1], dp(arrs[1]), dp(arrs[2]), dp(arrs[3]), dp(arrs[4]),
                                        max_iter, dp(elbo), ip(it), ip(cv), ip(info), None, None)


@pytest.mark.parametrize('tag,seed', [('step_p3q2', 2), ('mid_N300_p3q2', 4)])
def test_the_option_switches_the_refusal(tag, seed):
    pr, mask, g = _partial(tag, seed)
    x0 = np.array(g.get_parameters(), dtype=float)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, [x0, x0 * 1.01], R.init_state(pr, mask))
    lib = ctx._lib
    assert ctx.option('batch_mask', 0) == 1                 # (the old value comes back, as for the other options)
    assert ctx.option('batch_mask') == 0
    assert _raw_batch(ctx, kp, yr, jt, m0, v0, 3) == _hip.GPRN_E_UNSUPPORTED
    assert b'not supported under a data mask' in lib.gprn_last_error(ctx._h)
    ctx.option('batch_mask', 1)
    assert _raw_batch(ctx, kp, yr, jt, m0, v0, 3) == 0
    ctx.option('batch_mask', 0)
    assert _raw_batch(ctx, kp, yr, jt, m0, v0, 3) == _hip.GPRN_E_UNSUPPORTED
    # the sequential order still does not meet a mask, whatever the option says
    ctx.option('batch_mask', 1)
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_SEQUENTIAL) == _hip.GPRN_E_UNSUPPORTED
    assert _raw_batch(ctx, kp, yr, jt, m0, v0, 3) == 0
    assert ctx.option('fallbacks') == 0


def test_nelbo_batch_follows_the_keyword(capsys):
    tag = 'step_p2q1'
    pr = R.problem(tag)
    mask = R.partial_mask(*pr['y_raw'].shape, seed=11)
    g = _model(tag, pr['time'], pr['y_raw'], np.sqrt(pr['yerr2']), mask)
    x0 = g.get_parameters()
    sets = [x0, x0 * 1.01, x0 * 0.99]
    g.ELBOcalc()
    start = (g._mu, g._var)
    capsys.readouterr()
    batch = g.nELBO_batch(sets)                              # without the keyword: the chained loop, as before
    assert 'side by side' not in capsys.readouterr().out
    g._mu, g._var = start
    loop = [g.nELBO(x) for x in sets]
    np.testing.assert_allclose(batch, loop, rtol=1e-12)
    g._mu, g._var = start
    g.batch_under_mask = True                                # (an attribute: set after the context exists)
    side = g.nELBO_batch(sets)
    assert 'evaluations side by side' in capsys.readouterr().out
    assert g._backend().option('batch_chunk') == 3 and g.last_info == 0
    # every evaluation from the shared start: the first is the chained loop's first
    np.testing.assert_allclose(side[0], loop[0], rtol=PAIR_RTOL)
    assert np.all(np.isfinite(side))
    g._mu, g._var = start
    g.batch_under_mask = False
    np.testing.assert_allclose(g.nELBO_batch(sets), loop, rtol=1e-12)
    assert g._backend().option('fallbacks') == 0


@pytest.mark.parametrize('tag', ['step_p3q2', 'mid_N300_p3q2'])
def test_without_a_mask_the_option_changes_no_bit(tag):
    meta, d = _cases.load(tag)
    out = []
    for on in (False, True):
        nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
        g = gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d), batch_under_mask=on)
        g.set_components(nodes, weights, means, jit)
        x0 = np.array(g.get_parameters(), dtype=float)
        g._mu, g._var = np.array(d['mu_init'], dtype=float), np.array(d['var_init'], dtype=float)
        out.append(np.array(g.nELBO_batch([x0, x0 * 1.01, x0 * 0.99], max_iter=30)))
        assert g._backend().option('batch_mask') == int(on) and g._backend().option('batch_chunk') == 3
    assert np.array_equal(out[0], out[1]) and np.all(np.isfinite(out[0]))


# ------------------------------------------------------------------ 6. end to end
def test_mcmc_on_series_with_their_own_time_grids(monkeypatch, tmp_path, capsys):
    """mcmc(batch=True) on a from_series object: the walkers of every half-step go through the side-by-side call, its
    log-probabilities are -nELBO_batch of the same walkers from the same state, and the chain's vectors predict."""
    from scipy import stats
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fake_emcee'))
    monkeypatch.chdir(tmp_path)
    rng = np.random.RandomState(0)
    t1 = np.sort(rng.uniform(0.0, 100.0, 34))
    t2 = np.sort(rng.uniform(0.0, 100.0, 28))
    f = lambda t: np.sin(2 * np.pi * t / 37.0)
    series = [(t1, 1.0 * f(t1) + 0.1 * rng.normal(size=t1.size), np.full(t1.size, 0.1)),
              (t2, -0.6 * f(t2) + 0.1 * rng.normal(size=t2.size), np.full(t2.size, 0.1))]

    def fresh():
        g = gpyrn.inference.from_series(1, series, batch_under_mask=True)
        g.set_components([covfunc.SquaredExponential(1.0, 20.0)],
                         [covfunc.SquaredExponential(1.0, 60.0), covfunc.SquaredExponential(0.7, 60.0)],
                         [meanfunc.Constant(0.0), meanfunc.Constant(0.0)], [0.15, 0.15])
        return g

    g = fresh()
    assert g.p == 2 and g.N <= 64 and not g.mask.all() and g._batchable()
    g.ELBOcalc()
    priors = {'node1.theta': stats.uniform(0.5, 2.0), 'node1.ell': stats.uniform(10.0, 30.0),
              'jitter1': stats.uniform(0.05, 0.5)}
    calls = []
    inner = g.nELBO_batch

    def recording(sets, **kw):
        state = (np.array(g._mu), np.array(g._var))
        vals = inner(sets, **kw)
        calls.append(([np.array(x) for x in sets], state, np.array(vals)))
        return vals

    monkeypatch.setattr(g, 'nELBO_batch', recording)
    np.random.seed(3)
    capsys.readouterr()
    sampler = g.mcmc(priors, vars=list(priors), niter=2, batch=True)
    assert 'evaluations side by side' in capsys.readouterr().out
    assert g._backend().option('batch_chunk') > 1 and g._backend().option('fallbacks') == 0 and g.last_info == 0
    assert len(calls) >= 1 + 1 + 2 * 2                       # mcmc's own first evaluation, the sampler's, two half-steps per step
    lp, blobs = sampler.get_log_prob(), sampler.get_blobs()
    assert lp.shape == (2, 6) and np.all(np.isfinite(lp)) and np.all(np.isfinite(blobs))
    seen = np.concatenate([-c[2] for c in calls])
    assert all(np.any(b == seen) for b in blobs.ravel())     # every kept ELBO is one a side-by-side call returned
    g2 = fresh()
    g2._select_vars(list(priors))
    for sets, state, vals in calls:
        g2._mu, g2._var = state
        np.testing.assert_allclose(g2.nELBO_batch(sets, max_iter=100), vals, rtol=1e-12)
    mean, var = g.posterior_predictive(sampler.get_chain(flat=True), tstar=np.linspace(0.0, 100.0, 40))
    assert mean.shape == var.shape and np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(var > 0)
