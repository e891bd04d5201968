"""Side-by-side cross-validation on the GPU (gprn_elbocalc_batch_heldout, inference.heldout_batch / cross_validate): every
evaluation under its own fit mask against the dense restatement tests/_mask_ref.py on both paths and at the tile edge, the
held-out rows and log predictive densities against the NumPy combination of the restatement's state (tests/_heldout_ref.py), a
shared fit mask against today's masked batches bit for bit, the stop rule across chunks and through compaction against the
device one by one, the refusals, and the Python layer against four mask= objects.  No call may fall back to the event schedule."""
import ctypes
from itertools import chain

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _cases, _heldout_ref as H, _mask_ref as R
from tests.test_mask_batch_gpu import SCALES, _perturbed

pytestmark = pytest.mark.gpu
RTOL = 1e-8                   # the project's plain bound: against the restatement
PAIR_RTOL = 1e-9              # two device results from the same start, equal trip counts
MAX_ITER = 200
_REF = {}                     # restatement results, computed once per (tag, mask, sweeps) and shared


def _model(tag, time, y, yerr, mask=None, **kw):
    meta, _ = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    args = [a for i in range(y.shape[0]) for a in (y[i], yerr[i])]
    g = gpyrn.inference(meta['q'], time, *args, mask=mask, **kw)
    g.set_components(nodes, weights, means, jit)
    return g


def _plain(tag, mask=None, **kw):
    """The fixture's problem and a model of it (under `mask`, its masked y / yerr handed over as NaN / inf)."""
    pr = R.problem(tag)
    y, e = pr['y_raw'], np.sqrt(pr['yerr2'])
    if mask is not None:
        y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
    return pr, _model(tag, pr['time'], y, e, mask, **kw)


def _inputs(g, sets, starts):
    """The arrays gprn_elbocalc_batch_heldout takes, vector by vector, evaluation b from starts[b] = (mu, var); the kernel
    programs of the first vector go to the device.  Option "batch_mask" stays off: the new entry point does not need it."""
    ctx = g._backend()
    ctx.option('batch_mask', 0)
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
        m0.append(np.ravel(starts[i][0]))
        v0.append(np.ravel(starts[i][1]))
    return ctx, np.array(kp), np.array(yr), np.array(jt), np.array(m0), np.array(v0)


def _restated(tag, pr, mask, nsweeps):
    """R.sweeps under `mask` from its own start, once per case: (ELBO, mu, var, start)."""
    key = (tag, mask.tobytes(), nsweeps)
    if key not in _REF:
        mu0, var0 = R.init_state(pr, mask)
        E, _, mu, var = R.sweeps(pr['Kf'], pr['Kw'], pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2'], mu0, var0, mask, nsweeps)
        assert np.all(np.isfinite(E)) and np.all(var > 0)
        _REF[key] = (E[-1], mu, var, (mu0, var0))
    return _REF[key]


def _rows_close(what, a, ref):
    """norm-wise per output row, the bound of _cases.assert_state"""
    a, ref = np.asarray(a).reshape(-1, a.shape[-1]), np.asarray(ref).reshape(-1, a.shape[-1])
    scale = np.abs(ref).max(axis=1)
    err = (np.abs(a - ref).max(axis=1) / np.where(scale > 0, scale, 1.0)).max()
    assert err <= RTOL, '%s off by %.3g (norm-wise per output; bound %.1g)' % (what, err, RTOL)
    return err


def _check_slot(what, res, b, pr, D, fit, ref):
    """Slot b of a forced call against the restatement `ref` = (ELBO, mu, var, ...) under `fit` and the NumPy score of ITS state."""
    elbo, iters, conv, info, mu, var, hmean, hvar, lpd, n_held = res
    held = D & ~fit
    np.testing.assert_allclose(elbo[b], ref[0], rtol=RTOL)
    shape = mu[b].shape
    _cases.assert_state(what, mu[b], np.reshape(ref[1], shape), var[b], np.reshape(ref[2], shape))
    m_r, v_r, lpd_r, n_r = H.score(ref[1], ref[2], pr['y_resid'], pr['jitt2'], pr['yerr2'], held)
    t = H.terms(ref[1], ref[2], pr['y_resid'], pr['jitt2'], pr['yerr2'], held)
    assert np.all(t <= 0) or np.all(t >= 0), 'the terms of the log predictive density change sign: a relative bound needs one'
    assert n_held[b].tolist() == n_r.tolist() == held.sum(axis=1).tolist()
    assert np.all(hmean[b][~held] == 0) and np.all(hvar[b][~held] == 0)
    e1 = _rows_close(what + ', held means', hmean[b], m_r)
    e2 = _rows_close(what + ', held variances', hvar[b], v_r)
    print('%s: ELBO rel %.2e, held rows %.2e / %.2e, lpd rel %.2e' % (
        what, abs(elbo[b] / ref[0] - 1), e1, e2, np.abs(lpd[b][n_r > 0] / lpd_r[n_r > 0] - 1).max() if n_r.any() else 0.0))
    np.testing.assert_allclose(lpd[b], lpd_r, rtol=RTOL)


def _forced(tag, g, pr, D, fits, nsweeps, refs=None, pr_ref=None):
    """One forced call, evaluation b under fits[b] from its own start; every slot against its restatement."""
    x = np.array(g.get_parameters(), dtype=float)
    refs = [_restated(tag, pr, f, nsweeps) for f in fits] if refs is None else refs
    starts = [R.init_state(pr, f) for f in fits]
    ctx, kp, yr, jt, m0, v0 = _inputs(g, [x] * len(fits), starts)
    res = ctx.elbocalc_batch_heldout(kp, yr, jt, m0, v0, nsweeps, np.array(fits), forced=True)
    assert res is not None, 'the library has no side-by-side form for this problem'
    assert not res[3].any() and (res[1] == nsweeps).all() and not res[2].any()
    assert ctx.option('fallbacks') == 0 and ctx.option('batch_chunk') == len(fits)
    again = ctx.elbocalc_batch_heldout(kp, yr, jt, m0, v0, nsweeps, np.array(fits), forced=True)
    for a, b in zip(res, again):                                # every sum in a fixed order: the same bits
        assert np.array_equal(a, b)
    return res, refs


def _with_times_held(mask, times):
    m = mask.copy()
    m[:, times] = False
    return m


# ------------------------------------------------------------------ 1. forced, one tile
def test_forced_one_tile_p3q2():
    tag = 'step_p3q2'
    pr, g = _plain(tag)
    fits = [R.partial_mask(3, 32, seed) for seed in range(1, 6)]
    assert [(~f).sum(axis=1).tolist() for f in fits] == [[6, 8, 6], [7, 7, 7], [7, 9, 7], [9, 5, 9], [6, 6, 9]]
    D = np.ones((3, 32), dtype=bool)
    res, refs = _forced(tag, g, pr, D, fits, pr['meta']['nsweeps'])
    for b, f in enumerate(fits):
        _check_slot('heldout %s slot %d' % (tag, b), res, b, pr, D, f, refs[b])


def _p2q1_fits():
    fits = [R.partial_mask(2, 32, seed) for seed in range(1, 6)]
    return fits + [_with_times_held(fits[0], [5, 6, 20])]       # the node has a U in the sixth evaluation only


def test_forced_one_tile_p2q1_with_a_node_u_in_one_evaluation():
    tag = 'step_p2q1'
    pr, g = _plain(tag)
    fits = _p2q1_fits()
    assert [int((~f.any(axis=0)).sum()) for f in fits] == [0, 0, 0, 0, 0, 3]
    D = np.ones((2, 32), dtype=bool)
    res, refs = _forced(tag, g, pr, D, fits, pr['meta']['nsweeps'])
    for b, f in enumerate(fits):
        _check_slot('heldout %s slot %d' % (tag, b), res, b, pr, D, f, refs[b])


# ------------------------------------------------------------------ 2. under a data mask, at the tile edge
@pytest.mark.parametrize('kw,N', [(dict(per_gap=3), 128), (dict(per_gap=3, n_after=2), 129)])
def test_under_a_data_mask_at_the_tile_edge(kw, N):
    """96 (97) never-observed times with NaN / inf in them; the folds live at the 32 observed positions, so every slot is the
    N = 32 problem's: its ELBO, its state at those positions, its held rows and its log predictive density."""
    tag = 'step_p2q1'
    pr, D, pos = R.inserted(tag, **kw)
    assert D.shape == (2, N) and pos.size == 32
    small = R.problem(tag)
    nsweeps = small['meta']['nsweeps']
    fits32 = _p2q1_fits()[:3] + [_p2q1_fits()[5]]
    fits = []
    for f in fits32:
        full = np.zeros((2, N), dtype=bool)
        full[:, pos] = f
        fits.append(full)
    g = _model(tag, pr['time'], pr['y_nan'], pr['yerr_inf'], D)
    # INTO the device's y - mean and variances at the never-observed entries (the host layer would have replaced them)
    g.y = np.where(D, g.y, np.nan)
    g.yerr = np.where(D, g.yerr, np.inf)
    x = np.array(g.get_parameters(), dtype=float)
    starts = [R.init_state(pr, f) for f in fits]
    ctx, kp, yr, jt, m0, v0 = _inputs(g, [x] * len(fits), starts)
    assert not np.all(np.isfinite(yr))
    res = ctx.elbocalc_batch_heldout(kp, yr, jt, m0, v0, nsweeps, np.array(fits), forced=True)
    assert res is not None and not res[3].any() and ctx.option('fallbacks') == 0
    elbo, _, _, _, mu, var, hmean, hvar, lpd, n_held = res
    assert all(np.all(np.isfinite(a)) for a in (elbo, mu, var, hmean, hvar, lpd))
    D32 = np.ones((2, 32), dtype=bool)
    for b, f32 in enumerate(fits32):
        ref = _restated(tag, small, f32, nsweeps)
        print('heldout inserted N = %d slot %d: ELBO %.9f (N = 32: %.9f)' % (N, b, elbo[b], ref[0]))
        np.testing.assert_allclose(elbo[b], ref[0], rtol=RTOL)
        shape = (3, 1, 32)
        _cases.assert_state('heldout inserted N = %d slot %d' % (N, b), mu[b][..., pos], np.reshape(ref[1], shape),
                            var[b][..., pos], np.reshape(ref[2], shape))
        m_r, v_r, lpd_r, n_r = H.score(ref[1], ref[2], small['y_resid'], small['jitt2'], small['yerr2'], D32 & ~f32)
        assert n_held[b].tolist() == n_r.tolist()
        off = np.ones(N, dtype=bool); off[pos] = False
        assert np.all(hmean[b][:, off] == 0) and np.all(hvar[b][:, off] == 0)
        _rows_close('held means', hmean[b][:, pos], m_r)
        _rows_close('held variances', hvar[b][:, pos], v_r)
        np.testing.assert_allclose(lpd[b], lpd_r, rtol=RTOL)


# ------------------------------------------------------------------ 3. above one tile
def test_forced_above_one_tile_n300():
    tag = 'mid_N300_p3q2'
    pr, g = _plain(tag)
    fits = [R.partial_mask(3, 300, seed) for seed in range(1, 6)]
    counts = [(~f).sum(axis=1).tolist() for f in fits]
    assert [87, 53, 87] in counts and [53, 85, 83] in counts
    D = np.ones((3, 300), dtype=bool)
    res, refs = _forced(tag, g, pr, D, fits, pr['meta']['nsweeps'])
    for b, f in enumerate(fits):
        _check_slot('heldout %s slot %d' % (tag, b), res, b, pr, D, f, refs[b])


def test_forced_above_one_tile_n512_two_row_tiles_of_u_and_nothing_held():
    tag = 'mid_N512_p3q2'
    pr, g = _plain(tag)
    fits = [R.partial_mask(3, 512, 5, lo=0.30, hi=0.45), R.partial_mask(3, 512, 1), np.ones((3, 512), dtype=bool)]
    assert [(~f).sum(axis=1).tolist() for f in fits] == [[160, 214, 170], [106, 143, 129], [0, 0, 0]]
    D = np.ones((3, 512), dtype=bool)
    res, refs = _forced(tag, g, pr, D, fits, 2)
    for b, f in enumerate(fits):
        _check_slot('heldout %s slot %d' % (tag, b), res, b, pr, D, f, refs[b])
    assert np.all(res[8][2] == 0) and np.all(res[9][2] == 0) and np.all(res[6][2] == 0) and np.all(res[7][2] == 0)


# ------------------------------------------------------------------ 4. a shared fit mask is today's path
@pytest.mark.parametrize('tag,seed', [('step_p3q2', 2), ('mid_N300_p3q2', 4)])
def test_a_shared_fit_mask_returns_the_bits_of_the_masked_batch(tag, seed):
    pr = R.problem(tag)
    p, N = pr['y_raw'].shape
    M = R.partial_mask(p, N, seed)
    _, gm = _plain(tag, mask=M)
    x0 = np.array(gm.get_parameters(), dtype=float)
    sets = [x0 * s for s in SCALES[:4]]
    start = R.init_state(pr, M)
    starts = [start] * len(sets)
    fits = np.array([M] * len(sets))
    # today's path: gprn_elbocalc_batch under "batch_mask" on the context masked with M
    ctx, kp, yr, jt, m0, v0 = _inputs(gm, sets, starts)
    ctx.option('batch_mask', 1)
    today = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True)
    assert today is not None and not today[3].any()
    ctx.option('batch_mask', 0)
    same_ctx = ctx.elbocalc_batch_heldout(kp, yr, jt, m0, v0, MAX_ITER, fits)
    # ... and on a context without a mask
    _, g = _plain(tag)
    ctx2, kp2, yr2, jt2, m2, v2 = _inputs(g, sets, starts)
    other_ctx = ctx2.elbocalc_batch_heldout(kp2, yr2, jt2, m2, v2, MAX_ITER, fits)
    for what, got in (('the masked context', same_ctx), ('a context without a mask', other_ctx)):
        assert got is not None, what
        for k, name in enumerate(('elbo', 'iterations', 'converged', 'info', 'mu', 'var')):
            assert np.array_equal(got[k], today[k]), '%s: %s differs from the masked batch' % (what, name)
    assert np.all(same_ctx[9] == 0) and np.all(same_ctx[8] == 0)          # under D = M nothing is held out
    assert other_ctx[9].tolist() == [(~M).sum(axis=1).tolist()] * len(sets)
    assert ctx.option('fallbacks') == 0 and ctx2.option('fallbacks') == 0


# ------------------------------------------------------------------ 5. stop rule, chunks, compaction
@pytest.mark.parametrize('tag,B,budget_mb', [('step_p3q2', 20, 1), ('mid_N300_p3q2', 7, 100)])
def test_the_stop_rule_across_chunks_against_one_by_one(tag, B, budget_mb):
    """Evaluation b: scale b of tests/test_mask_batch_gpu.py under mask seed 1 + b mod 5; cold from each mask's own start,
    then warm from the state each mask converges to at x0, against ELBOcalc on a second object built with mask=fit_mask[b]."""
    pr, g = _plain(tag)
    p, N = pr['y_raw'].shape
    masks = [R.partial_mask(p, N, 1 + s) for s in range(5)]
    ones = [_plain(tag, mask=m)[1] for m in masks]
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = _perturbed(x0, B)
    fits = np.array([masks[b % 5] for b in range(B)])
    cold = [R.init_state(pr, m) for m in masks]
    warm = []
    for s, g1 in enumerate(ones):
        g1.set_parameters(x0.copy())
        _, mu_w, var_w, _ = g1.ELBOcalc(mu=np.array(cold[s][0]), var=np.array(cold[s][1]))
        warm.append((np.asarray(mu_w), np.asarray(var_w)))
    for what, per_mask in (('cold', cold), ('warm', warm)):
        starts = [per_mask[b % 5] for b in range(B)]
        ctx = g._backend()
        ctx.option('batch_mem_mb', budget_mb)
        ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, starts)
        res = ctx.elbocalc_batch_heldout(kp, yr, jt, m0, v0, MAX_ITER, fits)
        assert res is not None and not res[3].any()
        assert 1 <= ctx.option('batch_chunk') < B and ctx.option('fallbacks') == 0
        elbo, iters, conv, info, mu, var, hmean, hvar, lpd, n_held = res
        print('heldout_vs_one_by_one %s %s: trips %s' % (tag, what, iters.tolist()))
        if what == 'cold':
            assert len(set(iters.tolist())) > 1                  # evaluations leave the batch at different trips
        for b in range(B):
            g1 = ones[b % 5]
            g1.set_parameters(np.array(sets[b], dtype=float))
            e1, mu1, var1, it1 = g1.ELBOcalc(max_iter=MAX_ITER, mu=np.array(starts[b][0], dtype=float),
                                             var=np.array(starts[b][1], dtype=float))
            assert g1.last_info == 0 and g1._backend().option('fallbacks') == 0
            np.testing.assert_allclose(elbo[b], float(e1), rtol=PAIR_RTOL)
            assert iters[b] == int(it1)
            _cases.assert_state('heldout %s %s, vector %d' % (tag, what, b), mu[b], np.asarray(mu1), var[b], np.asarray(var1),
                                tol=PAIR_RTOL)
            # the rows and the score are the NumPy combination of the state that came back
            nodes, weights, means, jit = g1._get_components()
            resid = (np.concatenate(g.y) - g1._mean(means)).reshape(p, N)
            held = ~fits[b]
            m_r, v_r, lpd_r, n_r = H.score(mu[b], var[b], resid, np.asarray(jit, dtype=float) ** 2, pr['yerr2'], held)
            assert n_held[b].tolist() == n_r.tolist()
            _rows_close('held means', hmean[b], m_r)
            _rows_close('held variances', hvar[b], v_r)
            np.testing.assert_allclose(lpd[b], lpd_r, rtol=RTOL)


# ------------------------------------------------------------------ 6. refusals and errors
def _raw(ctx, kp, yr, jt, m0, v0, max_iter, fits):
    B = kp.shape[0]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    arrs = [np.ascontiguousarray(a, dtype=float) for a in (kp, yr, jt, m0, v0)]
    fm = np.ascontiguousarray(fits, dtype=np.uint8)
    elbo, lpd = np.zeros(B), np.zeros((B, ctx.p))
    it, cv, info = (np.zeros(B, dtype=np.int32) for _ in range(3))
    nh = np.zeros((B, ctx.p), dtype=np.int32)
    rc = ctx._lib.gprn_elbocalc_batch_heldout(ctx._h, B, dp(arrs[0]), kp.shape[1], dp(arrs[1]), dp(arrs[2]), dp(arrs[3]), dp(arrs[4]),
                                              max_iter, 0, fm.ctypes.data, dp(elbo), ip(it), ip(cv), ip(info), None, None, None, None,
                                              dp(lpd), ip(nh))
    return rc, ctx._lib.gprn_last_error(ctx._h) or b''


def _sweep_bits(g, start):
    ctx = g._backend()
    ctx.set_muvar(np.asarray(start[0], dtype=float), np.asarray(start[1], dtype=float))
    e, parts, info = ctx.sweep(2, commit=True)
    assert info == 0
    return np.concatenate([e, parts.ravel(), np.ravel(ctx.get_muvar())])


@pytest.mark.parametrize('tag', ['step_p3q2', 'mid_N300_p3q2'])
def test_refusals_name_their_reason_and_leave_the_context_alone(tag):
    pr = R.problem(tag)
    p, N = pr['y_raw'].shape
    D = np.ones((p, N), dtype=bool)
    D[0, 3] = False
    _, g = _plain(tag, mask=D)
    x0 = np.array(g.get_parameters(), dtype=float)
    start = R.init_state(pr, D)
    fit = R.partial_mask(p, N, 1) & D
    ctx, kp, yr, jt, m0, v0 = _inputs(g, [x0, x0 * 1.01], [start, start])
    g.set_parameters(x0.copy())
    g.ELBOcalc(max_iter=2, mu=np.array(start[0]), var=np.array(start[1]))     # (the context's own set-up and state)
    before = _sweep_bits(g, start)
    good = np.array([fit, fit])
    bad = good.copy(); bad[1, 0, 3] = True
    rc, msg = _raw(ctx, kp, yr, jt, m0, v0, 3, bad)
    assert rc == _hip.GPRN_E_ARG and b'evaluation 1' in msg and b'data mask does not hold' in msg
    bad = good.copy(); bad[0, 2, :] = False
    rc, msg = _raw(ctx, kp, yr, jt, m0, v0, 3, bad)
    assert rc == _hip.GPRN_E_ARG and b'evaluation 0' in msg and b'without a fitted entry' in msg
    bad = good.copy(); bad[1, :, 11] = False
    rc, msg = _raw(ctx, kp, yr, jt, m0, v0, 3, bad)
    assert rc == _hip.GPRN_E_ARG and b'evaluation 1' in msg and b'without a fitted output' in msg
    rc, msg = _raw(ctx, kp, yr, jt, m0, v0, 0, good)
    assert rc == _hip.GPRN_E_ARG and b'committed sweep' in msg
    assert np.array_equal(_sweep_bits(g, start), before)
    rc, msg = _raw(ctx, kp, yr, jt, m0, v0, 3, good)
    assert rc == 0, msg
    assert np.array_equal(_sweep_bits(g, start), before) and ctx.option('fallbacks') == 0


def test_refusals_of_the_sequential_order_and_of_uploaded_kernels():
    tag = 'step_p3q2'
    pr, g = _plain(tag)
    p, N = pr['y_raw'].shape
    x0 = np.array(g.get_parameters(), dtype=float)
    start = R.init_state(pr, np.ones((p, N), dtype=bool))
    good = np.array([R.partial_mask(p, N, 1), R.partial_mask(p, N, 2)])
    ctx, kp, yr, jt, m0, v0 = _inputs(g, [x0, x0 * 1.01], [start, start])
    g.set_parameters(x0.copy())
    g.ELBOcalc(max_iter=2, mu=np.array(start[0]), var=np.array(start[1]))
    before = _sweep_bits(g, start)
    ctx.set_sweep_order(_hip.ORDER_SEQUENTIAL)
    rc, msg = _raw(ctx, kp, yr, jt, m0, v0, 3, good)
    assert rc == _hip.GPRN_E_UNSUPPORTED and b'sequential sweep order' in msg
    ctx.set_sweep_order(_hip.ORDER_REFERENCE)
    assert np.array_equal(_sweep_bits(g, start), before)
    assert _raw(ctx, kp, yr, jt, m0, v0, 3, good)[0] == 0
    assert np.array_equal(_sweep_bits(g, start), before)
    # an uploaded kernel in place of latent GP 0's program
    K = g._host_K(g.nodes[0], np.asarray(g.time, dtype=float)) + 1e-6 * np.eye(N)
    ctx.upload_K(0, K)
    rc, msg = _raw(ctx, kp, yr, jt, m0, v0, 3, good)
    assert rc == _hip.GPRN_E_UNSUPPORTED and b'device kernel program' in msg
    for gp, k in enumerate(chain(g.nodes, g.weights)):
        g._send_spec(ctx, gp, g._kernel_spec(k))
    g._prior_key = None
    g.ELBOcalc(max_iter=2, mu=np.array(start[0]), var=np.array(start[1]))
    assert np.array_equal(_sweep_bits(g, start), before) and ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 7. the Python layer
def test_cross_validate_against_four_masked_objects():
    tag = 'step_p3q2'
    pr, g = _plain(tag)
    p, N = pr['y_raw'].shape
    folds = g.cv_folds(4, rng=0)
    assert folds.n_never_held == 0
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0, x0 * 1.02]
    cv = g.cross_validate(folds, sets, max_iter=MAX_ITER)
    assert g.last_info == 0 and g._backend().option('fallbacks') == 0 and g._backend().option('batch_chunk') == 8
    assert cv.lpd.shape == (2, 4, p) and cv.elpd.shape == (2,) and cv.mean.shape == (2, p, N)
    assert np.all(cv.n_held.sum(axis=1) == N) and np.all(np.isfinite(cv.mean)) and np.all(cv.var > 0)
    np.testing.assert_allclose(cv.elpd, cv.lpd.sum(axis=(1, 2)), rtol=1e-14)
    for s, x in enumerate(sets):
        for f in range(4):
            fit = np.asarray(folds[f])
            _, g1 = _plain(tag, mask=fit)
            g1.set_parameters(x.copy())
            e1, mu1, var1, it1 = g1.ELBOcalc(max_iter=MAX_ITER)      # (a fresh object's own start under its mask)
            np.testing.assert_allclose(cv.elbo[s, f], float(e1), rtol=PAIR_RTOL)
            assert cv.iterations[s, f] == int(it1) and cv.converged[s, f]
            nodes, weights, means, jit = g1._get_components()
            mean_f = g1._mean(means).reshape(p, N)
            m_r, v_r, lpd_r, n_r = H.score(mu1, var1, pr['y_raw'] - mean_f, np.asarray(jit, dtype=float) ** 2, pr['yerr2'], ~fit)
            assert cv.n_held[s, f].tolist() == n_r.tolist()
            np.testing.assert_allclose(cv.lpd[s, f], lpd_r, rtol=RTOL)
            held = ~fit
            scale = np.abs(m_r + mean_f).max()
            assert np.abs(cv.mean[s][held] - (m_r + mean_f)[held]).max() <= RTOL * scale
            np.testing.assert_allclose(cv.var[s][held], v_r[held], rtol=RTOL)
    # default vector: the object's own
    g.set_parameters(x0.copy())
    one = g.cross_validate(folds, max_iter=MAX_ITER)
    assert np.array_equal(one.lpd[0], cv.lpd[0]) and np.array_equal(one.elbo[0], cv.elbo[0])
