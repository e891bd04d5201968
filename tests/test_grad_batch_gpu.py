"""The ELBO gradient for many parameter vectors side by side on the GPU (gprn_elbocalc_batch_grad, Context.elbocalc_batch(
want_grad=, forced=), inference.nELBO_and_grad_batch): every slot of a batch against the dense restatement tests/_grad_ref.py,
perturbed vectors under the stop rule across chunk boundaries against the device one by one, a failed pivot in the middle of
a batch, the contract of the entry point, and the Python method against its own one-by-one branch.  The norm of a gradient
entry is tests/test_grad_fused_gpu.py's: |dev - ref| / sum |G| |dK/dtheta|.  No call may fall back to the event schedule."""
import ctypes
from itertools import chain

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from oracle import cpu_ref
from tests import _cases, _grad_ref as GR, _mask_ref as MR, _order_ref as OR

pytestmark = pytest.mark.gpu
RTOL = 1e-8
PROJECT_BOUND = 1e-8          # the project's tolerance; gprn_grad_elbo itself meets it against the same restatement
PAIR_BOUND = 2e-8             # two device results, each within PROJECT_BOUND of the same algebra


def _model(tag, order='reference'):
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    g = gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d), sweep_order=order)
    g.set_components(nodes, weights, means, jit)
    return meta, d, g


def _n_kernel(g):
    return sum(k.pars.size for k in chain(g.nodes, g.weights))


def _inputs(g, sets, start=None):
    """The arrays gprn_elbocalc_batch_grad takes, vector by vector; every evaluation from `start` = (mu, var), else from its
    own _initMuVar state.  The kernel programs of the first vector go to the device."""
    ctx = g._backend()
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
        mu, var = start if start is not None else g._initMuVar(nodes, weights, jitters)
        m0.append(np.ravel(mu))
        v0.append(np.ravel(var))
    return ctx, np.array(kp), np.array(yr), np.array(jt), np.array(m0), np.array(v0)


def _problem_at(g):
    """tests/_mask_ref.problem's dict for the model `g` at its CURRENT parameters."""
    t = np.asarray(g.time, dtype=float)
    nodes, weights, means, jit = g._get_components()
    Kf, Kw, _, _, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, g.y)
    return dict(nodes=nodes, weights=weights, means=means, jitters=jit, time=t, Kf=Kf, Kw=Kw, y_resid=yres, y_raw=g.y,
                yerr2=g.yerr2, jitt2=jitt2)


def _restated_sweep(pr, mu0, var0, order):
    """GR.sweep_state; under the sequential order the state, the ELBO and the weights' precisions are those of
    tests/_order_ref.py's sequential sweep (the nodes' precisions read the old state only: the same in both orders)."""
    st = GR.sweep_state(pr, mu0, var0)
    if order == 'sequential':
        Lf = np.array([np.linalg.cholesky(K) for K in pr['Kf']])
        Lw = np.array([np.linalg.cholesky(K) for K in pr['Kw']])
        E, mu, var, _ = OR.sweep(pr['Kf'], pr['Kw'], Lf, Lw, pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2'],
                                 np.asarray(mu0), np.asarray(var0), order='sequential')[:4]
        prec = 1.0 / st['variance']
        st['d_w'] = np.array([[(mu[0, j] ** 2 + var[0, j]) * prec[i] for i in range(st['p'])] for j in range(st['q'])])
        st['elbo'], st['mu'], st['var'] = E, mu, var
    return st


# ------------------------------------------------------------------ 1. every slot against the restatement
# step_p1q1: one tile, q = 1; step_p3q2: one tile, cross terms, Q2 scramble; step_p2q3: one tile, two cross terms (also under
# the sequential order); cfg1_N200: two tiles, ragged last tile; mid_N300_p3q2: three tiles, cross terms
@pytest.mark.parametrize('tag,order', [('step_p1q1', 'reference'), ('step_p3q2', 'reference'), ('step_p2q3', 'reference'),
                                       ('step_p2q3', 'sequential'), ('cfg1_N200', 'reference'),
                                       ('mid_N300_p3q2', 'reference')])
def test_every_slot_of_a_forced_batch_matches_the_restatement(tag, order):
    B = 5
    meta, d, g = _model(tag, order)
    pr = MR.problem(tag)
    mu0, var0 = np.array(d['mu_init'], dtype=float), np.array(d['var_init'], dtype=float)
    x = np.array(g.get_parameters(), dtype=float)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, [x] * B, (mu0, var0))
    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 1, want_state=True, want_grad=True, forced=True)
    assert res is not None, 'the library has no batched form for this problem'
    elbo, iters, conv, info, mu, var, grads = res
    assert not info.any() and (iters == 1).all() and not conv.any()
    st = _restated_sweep(pr, mu0, var0, order)
    ref, norm = GR.kernel_gradient(pr, st, 'chol')
    assert grads.shape == (B, ref.size) and np.all(np.isfinite(grads))
    dev = grads / g.q
    worst = float((np.abs(dev - ref[None]) / norm[None]).max())
    print('grad_batch_accuracy %s %s: worst slot %.2e; ELBO rel %.2e' % (tag, order, worst, np.abs(elbo / st['elbo'] - 1).max()))
    assert worst <= PROJECT_BOUND
    np.testing.assert_allclose(elbo, np.full(B, st['elbo']), rtol=RTOL)
    for b in range(B):
        _cases.assert_state('batch slot %d of %d, %s %s' % (b, B, tag, order), mu[b], st['mu'], var[b], st['var'])
        assert np.array_equal(grads[b], grads[0])
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 2. perturbed vectors, stop rule on, chunk boundaries
# step_p3q2: the one-tile chunk at its minimum of 16 (and the gradient pass in groups of a few evaluations: its scratch follows
# the same budget); mid_N300_p3q2: 39 MB of slabs per evaluation, chunks of 2
@pytest.mark.parametrize('tag,B,budget_mb,chunk', [('step_p3q2', 20, 1, 16), ('mid_N300_p3q2', 5, 100, 2)])
def test_perturbed_vectors_under_the_stop_rule_across_chunks(tag, B, budget_mb, chunk):
    MAX_ITER = 200
    meta, d, g = _model(tag)
    _, _, g1 = _model(tag)                                   # the one-by-one side, a context of its own
    ctx = g._backend()
    ctx.option('batch_mem_mb', budget_mb)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(17)
    sets = [x0 * rng.uniform(0.9, 1.1, x0.size) for _ in range(B)]
    n_k = _n_kernel(g)
    g1.set_parameters(x0.copy())
    _, mu_w, var_w, _ = g1.ELBOcalc()
    for what, start in (('cold', None), ('warm', (mu_w, var_w))):
        ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, start)
        plain = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True)
        assert ctx.option('batch_chunk') == chunk
        res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True, want_grad=True)
        assert ctx.option('batch_chunk') == chunk
        for a, b in zip(plain, res[:6]):                     # ELBO, trips, verdicts and states: the same bits without grad_out
            assert np.array_equal(a, b)
        again = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True, want_grad=True)
        for a, b in zip(res, again):
            assert np.array_equal(a, b)
        elbo, iters, conv, info, mu, var, grads = res
        assert not info.any() and np.all(np.isfinite(grads))
        worst = 0.0
        for b, x in enumerate(sets):
            g1.set_parameters(x.copy())
            nodes, weights, means, jitters = g1._get_components()
            c1 = g1._setup_device(nodes, weights, means, jitters)
            assert g1.last_info == 0
            s_mu, s_var = start if start is not None else g1._initMuVar(nodes, weights, jitters)
            c1.set_muvar(np.asarray(s_mu, dtype=float), np.asarray(s_var, dtype=float))
            hist, it1, conv1, info1, mu1, var1 = c1.elbocalc(MAX_ITER)
            one = c1.grad_elbo(n_k)
            assert info1 == 0 and it1 == iters[b] and bool(conv1) == bool(conv[b])
            np.testing.assert_allclose(elbo[b], hist[-1], rtol=1e-9)
            # the scale of an entry: the restatement's sum |G| |dK/dtheta| at this vector, one sweep from the returned state
            pr = _problem_at(g1)
            _, norm = GR.kernel_gradient(pr, GR.sweep_state(pr, mu[b], var[b]), 'chol')
            worst = max(worst, float((np.abs(grads[b] - one) / g.q / norm).max()))
            assert c1.option('fallbacks') == 0
        print('grad_batch_vs_one_by_one %s %s: worst entry %.2e, trips %d..%d' % (tag, what, worst, iters.min(), iters.max()))
        assert worst <= PAIR_BOUND
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 3. a failed pivot in the middle
@pytest.mark.parametrize('tag', ['step_p3q2', 'mid_N300_p3q2'])
def test_a_failed_pivot_in_the_middle_of_a_batch(tag):
    """tests/test_parity_gpu.py::test_a_failed_evaluation_leaves_a_batch_at_once's way: a NaN jitter, so no pivot of B is
    positive -- a numerical verdict.  The call without the bad vector has a good one in its place (the same launch shapes)."""
    meta, d, g = _model(tag)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(23)
    sets = [x0 * rng.uniform(0.98, 1.02, x0.size) for _ in range(5)]
    bad = [x.copy() for x in sets]
    bad[2][-1] = np.nan
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets)
    good = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 6, want_state=True, want_grad=True)
    assert not good[3].any()
    ctx, kp, yr, jt, m0, v0 = _inputs(g, bad)
    got = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 6, want_state=True, want_grad=True)
    elbo, iters, conv, info, mu, var, grads = got
    assert info[2] > 0 and np.isnan(elbo[2]) and not conv[2]
    assert np.array_equal(grads[2], np.zeros(grads.shape[1]))
    keep = [0, 1, 3, 4]
    assert not info[keep].any() and np.all(np.isfinite(grads[keep]))
    for a, b in zip(good, got):
        assert np.array_equal(a[keep], b[keep])
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 4. contract
def _raw_call(ctx, kp, yr, jt, m0, v0, max_iter, flags=0, want_grad=True):
    B = kp.shape[0]
    dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    arrs = [np.ascontiguousarray(a, dtype=float) for a in (kp, yr, jt, m0, v0)]
    elbo, grad = np.zeros(B), (np.zeros((B, kp.shape[1])) if want_grad else None)
    it, cv, info = (np.zeros(B, dtype=np.int32) for _ in range(3))
    return ctx._lib.gprn_elbocalc_batch_grad(ctx._h, B, dp(arrs[0]), kp.shape[1], dp(arrs[1]), dp(arrs[2]), dp(arrs[3]),
                                             dp(arrs[4]), max_iter, flags, dp(elbo), ip(it), ip(cv), ip(info), None, None,
                                             dp(grad))


@pytest.mark.parametrize('tag', ['step_p3q2', 'cfg1_N200'])
def test_contract_of_the_entry_point(tag):
    meta, d, g = _model(tag)
    x = np.array(g.get_parameters(), dtype=float)
    n_k = _n_kernel(g)
    _, kp, yr, jt, m0, v0 = _inputs(g, [x * 1.01, x * 0.99, x])
    # the context's own problem (at x): a committed sweep, then what it holds
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    ctx.set_muvar(np.array(d['mu_init'], dtype=float), np.array(d['var_init'], dtype=float))
    _, _, info = ctx.sweep(1, commit=True)
    assert info == 0

    def held():
        out = list(ctx.get_muvar())
        sc = ctx.get_scalars()
        out += [np.ravel(sc[k]) for k in sorted(sc)]
        for gp in range(g.q * (g.p + 1)):
            out += [ctx.get_matrix(_hip.M_K, gp), ctx.get_matrix(_hip.M_KLINV, gp)]
        return out

    before = held()
    assert np.all(np.isfinite(ctx.grad_elbo(n_k)))
    lib = ctx._lib
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 0) == _hip.GPRN_E_ARG              # no sweep is committed
    assert b'committed sweep' in lib.gprn_last_error(ctx._h)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 0, want_grad=False) == 0
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, flags=2) == _hip.GPRN_E_ARG     # an unknown flag
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, flags=_hip.GPRN_BATCH_FORCED) == 0
    for a, b in zip(before, held()):
        assert np.array_equal(a, b)
    out = np.zeros(n_k)
    assert lib.gprn_grad_elbo(ctx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n_k) == _hip.GPRN_E_ARG
    assert b'committed sweep' in lib.gprn_last_error(ctx._h)
    # refusals: an uploaded kernel, a data mask
    ctx.upload_K(0, ctx.get_matrix(_hip.M_K, 0))
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2) == _hip.GPRN_E_UNSUPPORTED
    g._prior_key = None
    _inputs(g, [x])                                           # (the programs again)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2) == 0
    mask = np.ones((g.p, g.N), dtype=bool)
    mask[0, 3] = False
    ctx.set_mask(mask)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2) == _hip.GPRN_E_UNSUPPORTED
    assert b'mask' in lib.gprn_last_error(ctx._h)
    ctx.set_mask(None)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2) == 0
    assert ctx.option('fallbacks') == 0


def test_refused_on_a_context_with_a_communicator(monkeypatch):
    """The one-rank RCCL communicator of tests/test_order_gpu.py (a second rank cannot attach on one GPU)."""
    meta, d, g = _model('step_p1q1')
    x = np.array(g.get_parameters(), dtype=float)
    _, kp, yr, jt, m0, v0 = _inputs(g, [x, x])
    monkeypatch.setenv('GPRN_FORCE_RCCL', '1')
    ctx = _hip.Context(0)
    ctx.comm_init(1, 0, _hip.comm_unique_id())
    ctx.set_data(np.asarray(g.time, dtype=float), g.y, g.yerr, g.q)
    for gp, k in enumerate(chain(g.nodes, g.weights)):
        g._send_spec(ctx, gp, g._kernel_spec(k))
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2) == _hip.GPRN_E_UNSUPPORTED
    assert b'one rank' in ctx._lib.gprn_last_error(ctx._h)
    ctx.close()


# ------------------------------------------------------------------ 5. Python
def test_the_python_method_against_its_one_by_one_branch():
    tag = 'step_p3q2'
    meta, d, g = _model(tag)
    _, _, g1 = _model(tag)
    g1.batch_max_N = 0                                        # (N above batch_max_N: the one-by-one branch)
    x0 = np.array(g.get_parameters(), dtype=float)
    names = list(g.parameters_dict.keys())
    frozen = names[1]
    for m in (g, g1):
        m.freeze_parameter(name=frozen)
    free = ~g.frozen_mask
    assert free.sum() == x0.size - 1
    rng = np.random.RandomState(29)
    sets = [x0[free] * rng.uniform(0.95, 1.05, int(free.sum())) for _ in range(4)]
    start = (np.array(d['mu_init'], dtype=float), np.array(d['var_init'], dtype=float))
    vals, grads = g.nELBO_and_grad_batch(sets, sweeps=3, start=start)
    vals1, grads1 = g1.nELBO_and_grad_batch(sets, sweeps=3, start=start)
    assert g.last_info == 0 and g1.last_info == 0
    assert len(vals) == 4 and grads.shape == (4, int(free.sum())) and grads1.shape == grads.shape
    np.testing.assert_allclose(vals, vals1, rtol=1e-9)
    n_k = _n_kernel(g)
    n_m = x0.size - n_k - g.p
    pos = np.flatnonzero(free)                                # position of every free entry in the full vector
    is_k, is_m, is_j = pos < n_k, (pos >= n_k) & (pos < n_k + n_m), pos >= n_k + n_m
    assert is_k.sum() == n_k - 1 and is_j.sum() == g.p
    worst = 0.0
    for b, x in enumerate(sets):
        g1.set_parameters(x.copy())
        pr = _problem_at(g1)
        st = GR.sweep_state(pr, *start)
        for _ in range(2):
            st = GR.sweep_state(pr, st['mu'], st['var'])
        _, norm = GR.kernel_gradient(pr, st, 'chol')
        worst = max(worst, float((np.abs(grads[b] - grads1[b])[is_k] / norm[pos[is_k]]).max()))
    print('grad_batch_python: kernel entries differ by %.2e of their scale' % worst)
    assert worst <= PAIR_BOUND
    np.testing.assert_allclose(grads[:, is_j], grads1[:, is_j], rtol=1e-10)
    assert not grads[:, is_m].any() and not grads1[:, is_m].any()
    np.testing.assert_allclose(g.get_parameters(), sets[-1])
    # the stop rule's mode: values and gradients of the warm-started loops, as nELBO_batch's values
    g._mu, g._var = start
    vals_w, grads_w = g.nELBO_and_grad_batch(sets, max_iter=50)
    g._mu, g._var = start
    np.testing.assert_array_equal(vals_w, g.nELBO_batch(sets, max_iter=50))
    assert np.all(np.isfinite(grads_w))
    assert g._backend().option('fallbacks') == 0


def test_a_list_whose_kernel_expression_changes_shape_falls_back():
    """A kernel whose device program has another shape on either side of l = 25 (one squared exponential, or the sum of two
    equal ones): the list cannot be laid out side by side, every vector goes one by one -- the forced sweeps, then
    gprn_grad_elbo on what they left -- and the shapes are those of the side-by-side form."""
    class Switching(covfunc.covFunction):
        _param_names = ('a', 'l')
        _tag = 'SW'

        def _double(self):
            return self.pars[1] > 25.0

        def __call__(self, r):
            return (2.0 if self._double() else 1.0) * self.pars[0] ** 2 * np.exp(-0.5 * r ** 2 / self.pars[1] ** 2)

        def _device_program(self):
            push = (covfunc.OP_PUSH, covfunc.KID['SE'], 0)
            ops = [push, push, (covfunc.OP_ADD, 0, 0)] if self._double() else [push]
            return ops, np.asarray(self.pars, dtype=float).ravel()

    rng = np.random.RandomState(1)
    t = np.sort(rng.rand(40)) * 50
    y, e = rng.randn(2, 40), 0.1 + 0.1 * rng.rand(2, 40)

    def fresh():
        g = gpyrn.inference(1, t, y[0], e[0], y[1], e[1])
        g.set_components(Switching(1.0, 24.0), [covfunc.SquaredExponential(1.0, 20.0), covfunc.SquaredExponential(0.8, 30.0)],
                         [meanfunc.Constant(0.0), meanfunc.Constant(0.1)], [0.3, 0.4])
        return g

    g = fresh()
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0.copy(), x0.copy(), x0.copy()]
    sets[1][1] = 26.0                                         # the node's length scale: the other program
    sets[2][0] = 1.1
    assert g._batch_stage([x.copy() for x in sets]) is None
    vals, grads = g.nELBO_and_grad_batch(sets, sweeps=2)
    assert len(vals) == 3 and grads.shape == (3, x0.size) and np.all(np.isfinite(vals)) and np.all(np.isfinite(grads))
    g2 = fresh()
    n_k = _n_kernel(g2)
    for b, x in enumerate(sets):
        g2.set_parameters(x.copy())
        ctx = g2._setup_device(g2.nodes, g2.weights, g2.means, g2.jitters)
        ctx.set_muvar(*[np.asarray(a, dtype=float) for a in g2._initMuVar(g2.nodes, g2.weights, g2.jitters)])
        elbo, _, info = ctx.sweep(2, commit=True)
        assert info == 0
        np.testing.assert_allclose(vals[b], -elbo[-1], rtol=1e-12)
        assert np.array_equal(grads[b, :n_k], -ctx.grad_elbo(n_k) / g2.q)
