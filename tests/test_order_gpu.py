"""The sequential sweep order on the GPU (inference(..., sweep_order='sequential'), gprn_set_sweep_order) against the NumPy
restatement tests/_order_ref.py: forced sweeps on both paths, what the two orders share bit for bit, ELBOcalc with its trip
count, nELBO_batch slot by slot, grad_ELBO, and the refusals of the C ABI.  Tolerances: the project's own (1e-8 on the ELBO
and its parts, _cases.assert_state on the state).  No call may fall back to the event schedule."""
import ctypes
import os

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from oracle import cpu_ref
from tests import _cases, _order_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-8


def _model(tag, order='sequential'):
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    g = gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d), sweep_order=order)
    g.set_components(nodes, weights, means, jit)
    return meta, d, g


def _assert_default_schedule(ctx):
    assert ctx.option('fallbacks') == 0
    if os.environ.get('GPRN_FLAGS', '1') != '0' and not os.environ.get('ROCPROF_COUNTER_COLLECTION'):
        assert ctx.option('flags') == 1


def _device(g, small_path=None):
    ctx = g._backend()
    if small_path is not None:
        ctx.option('small_path', small_path)
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    assert g.last_info == 0
    return ctx


# ------------------------------------------------------------------ forced sweeps
@pytest.mark.parametrize('tag,small_path', [('step_p3q2', None), ('step_p2q3', None), ('kmix_N200_p2q2', None),
                                            ('mid_N300_p3q2', None), ('mid_N512_p3q2', None), ('cfg5shape_N1024', None),
                                            ('step_p3q2', 0), ('step_p2q3', 0)])
def test_forced_sweeps_match_the_restatement(tag, small_path):
    """The fixture's number of sweeps (at least 2) from _initMuVar: ELBO and parts of every sweep, the final state.  The
    one-tile fixtures run on the one-tile kernels and, with option small_path = 0, on the launch schedule."""
    meta, d, g = _model(tag)
    pr = R.problem(tag)
    n = max(2, int(meta['nsweeps']))
    E, P, mu_r, var_r = R.sweeps(*pr['args'], pr['mu0'], pr['var0'], n, order='sequential')
    ctx = _device(g, small_path)
    mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
    ctx.set_muvar(mu0, var0)
    elbo, parts, info = ctx.sweep(n, commit=True)
    assert info == 0
    print(tag, 'ELBO', elbo, 'rel', np.abs(elbo / E - 1).max(), 'parts rel', np.abs(parts / P - 1).max())
    np.testing.assert_allclose(elbo, E, rtol=RTOL)
    np.testing.assert_allclose(parts, P, rtol=RTOL)
    mu, var = ctx.get_muvar()
    _cases.assert_state('sequential forced sweeps %s (small_path %s)' % (tag, small_path), mu, mu_r, var, var_r)
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ what the orders share
@pytest.mark.parametrize('tag,small_path', [('step_p3q2', None), ('step_p2q3', None), ('step_p2q3', 0), ('mid_N300_p3q2', None)])
def test_first_sweep_shares_variances_and_group_zero_with_the_reference_order(tag, small_path):
    out = {}
    for order in ('reference', 'sequential'):
        meta, d, g = _model(tag, order)
        ctx = _device(g, small_path)
        ctx.set_muvar(d['mu_init'], d['var_init'])
        _, _, info = ctx.sweep(1, commit=True)
        assert info == 0
        out[order] = ctx.get_muvar()
        _assert_default_schedule(ctx)
    (mu_r, var_r), (mu_s, var_s) = out['reference'], out['sequential']
    assert np.array_equal(var_s[0], var_r[0])                  # every node variance
    assert np.array_equal(mu_s[0, 0], mu_r[0, 0])              # mu_f0
    assert np.array_equal(var_s[1:, 0], var_r[1:, 0])          # the variances of node 0's weights
    assert not np.allclose(mu_s[0, 1], mu_r[0, 1], rtol=1e-6, atol=0)


@pytest.mark.parametrize('tag', ['step_p1q1', 'step_p2q1', 'cfg1_N200'])
def test_with_one_node_the_orders_are_bit_identical(tag):
    out = {}
    for order in ('reference', 'sequential'):
        meta, d, g = _model(tag, order)
        assert meta['q'] == 1
        ctx = _device(g)
        ctx.set_muvar(d['mu_init'], d['var_init'])
        elbo, parts, _ = ctx.sweep(3, commit=True)
        out[order] = (elbo, parts) + ctx.get_muvar() + g.ELBOcalc()[:3]
        _assert_default_schedule(ctx)
    for a, b in zip(out['reference'], out['sequential']):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('tag', ['step_p2q3', 'mid_N300_p3q2'])
def test_back_to_the_reference_order_is_a_context_that_never_left_it(tag):
    meta, d, g0 = _model(tag, 'reference')
    c0 = _device(g0)
    c0.set_muvar(d['mu_init'], d['var_init'])
    want = c0.sweep(2, commit=True)[:2] + c0.get_muvar()
    meta, d, g = _model(tag, 'reference')
    ctx = _device(g)
    g.sweep_order = 'sequential'
    ctx.set_muvar(d['mu_init'], d['var_init'])
    ctx.sweep(2, commit=True)
    g.sweep_order = 'reference'
    ctx.set_muvar(d['mu_init'], d['var_init'])
    got = ctx.sweep(2, commit=True)[:2] + ctx.get_muvar()
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(got[0], d['elbo_sweeps'][:2], rtol=RTOL)
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ ELBOcalc
@pytest.mark.parametrize('tag', ['step_p3q2', 'step_p2q3', 'mid_N300_p3q2', 'cfg5shape_N1024'])
def test_elbocalc_history_state_and_trip_count(tag):
    """The trip count is comparable because the rule's criterion is away from its threshold on these fixtures: asserted
    here, on the restatement alone (1e-6 relative at the firing trip and the one before)."""
    meta, d, g = _model(tag)
    pr = R.problem(tag)
    e_r, mu_r, var_r, it_r, hist_r, crit = R.elbo_calc(*pr['args'], pr['mu0'], pr['var0'], order='sequential')
    print(tag, 'restatement: trips', it_r, 'ELBO', hist_r[1], '->', e_r, 'criterion', crit[-2:])
    assert it_r > 3 and crit[-1] < 1e-3
    for c in crit[-2:]:
        assert abs(c - 1e-3) > 1e-6 * 1e-3
    E, mu, var, it = g.ELBOcalc()
    print(tag, 'device: trips', it, 'ELBO', E)
    assert g.last_info == 0
    assert it == it_r
    np.testing.assert_allclose(g._elbo_history, hist_r, rtol=RTOL)
    np.testing.assert_allclose(E, e_r, rtol=RTOL)
    _cases.assert_state('sequential ELBOcalc ' + tag, mu, mu_r, var, var_r)
    _assert_default_schedule(g._backend())


# ------------------------------------------------------------------ nELBO_batch
@pytest.mark.parametrize('tag,B,budget_mb', [('step_p2q3', 5, 0), ('mid_N300_p3q2', 7, 0), ('mid_N300_p3q2', 9, 100)])
def test_nelbo_batch_slots_equal_one_by_one_evaluation(tag, B, budget_mb, capsys):
    """B perturbed parameter vectors side by side against the same evaluations one by one from the same starting state,
    cold (each from its own _initMuVar state) and warm (all from one converged state): one tile, above it, and a list
    longer than one chunk (batch_mem_mb)."""
    _, _, g = _model(tag)
    if budget_mb:
        g._backend().option('batch_mem_mb', budget_mb)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(11)
    sets = [x0 * (1.0 + 0.05 * rng.standard_normal(x0.size)) + 0.01 * rng.standard_normal(x0.size) * (x0 == 0)
            for _ in range(B)]
    capsys.readouterr()
    got = np.array(g.nELBO_batch(sets))
    assert 'evaluations side by side' in capsys.readouterr().out, 'the list was evaluated one by one: no batched form?'
    assert g.last_info == 0 and np.all(np.isfinite(got))
    if budget_mb:
        assert 0 < g._backend().option('batch_chunk') < B
    _, _, gs = _model(tag)
    want, trips = [], []
    for x in sets:
        gs.set_parameters(x)
        e, _, _, it = gs.ELBOcalc()
        want.append(-e)
        trips.append(it)
    print(tag, 'cold trips', trips, 'rel', np.abs(got / np.array(want) - 1).max())
    np.testing.assert_allclose(got, want, rtol=1e-9)
    gs.set_parameters(x0)
    _, mu_w, var_w, _ = gs.ELBOcalc()
    g._mu, g._var = mu_w.copy(), var_w.copy()
    got = np.array(g.nELBO_batch(sets))
    want = []
    for x in sets:
        gs.set_parameters(x)
        e, _, _, it = gs.ELBOcalc(mu=mu_w, var=var_w)
        want.append(-e)
    print(tag, 'warm rel', np.abs(got / np.array(want) - 1).max())
    np.testing.assert_allclose(got, want, rtol=1e-9)
    _assert_default_schedule(g._backend())
    _assert_default_schedule(gs._backend())


# ------------------------------------------------------------------ grad_ELBO
@pytest.mark.parametrize('tag', ['step_p3q2', 'mid_N300_p3q2'])
def test_grad_elbo_under_the_sequential_order(tag):
    """As tests/test_parity_gpu.py::test_grad_elbo_against_finite_differences and with its tolerances: the returned ELBO is
    the restatement's one further sequential sweep, the gradient the central differences of cpu_ref.fixed_state_elbo at that
    sweep's state.  The covariances are those of that sequential sweep (tests/_order_ref.py, return_sigma): a weight's
    precision reads the NEW mean of its node, so from node 1 on they are not the reference order's."""
    meta, d, g = _model(tag)
    g.ELBOcalc()
    mu_prev, var_prev = g._mu.copy(), g._var.copy()
    E, grad = g.grad_ELBO(mean_sweeps=0)
    assert grad.shape == (len(g.get_parameters(include_frozen=True)),)
    t = np.asarray(g.time, dtype=float)
    nodes, weights, means, jit = g.nodes, g.weights, g.means, list(g.jitters)
    Kf, Kw, Lf, Lw, yres, j2 = cpu_ref.setup(t, nodes, weights, means, jit, g.y)
    E_ref, mu_n, var_n, parts, sig_f, sig_w = R.sweep(Kf, Kw, Lf, Lw, yres, g.y, g.yerr2, j2, mu_prev, var_prev,
                                                      order='sequential', return_sigma=True)
    print(tag, 'ELBO', E, 'restatement', E_ref)
    np.testing.assert_allclose(E, E_ref, rtol=RTOL)
    _cases.assert_state('sequential grad_ELBO sweep ' + tag, g._mu, mu_n, g._var, var_n)
    mu_f, mu_w = mu_n[0], mu_n[1:]

    def F():
        Kf_, Kw_, _, _, _, j2_ = cpu_ref.setup(t, nodes, weights, means, jit, g.y)
        return cpu_ref.fixed_state_elbo(Kf_, Kw_, g.y, g.yerr2, j2_, mu_f, mu_w, sig_f, sig_w)

    fd = []
    for k in list(nodes) + list(weights):
        for i in range(k.pars.size):
            v = k.pars[i]
            h = 1e-5 * max(1.0, abs(v))
            k.pars[i] = v + h; up = F()
            k.pars[i] = v - h; dn = F()
            k.pars[i] = v
            fd.append((up - dn) / (2 * h))
    fd += [0.0] * sum(0 if m is None else int(m._parsize) for m in means)
    for i in range(len(jit)):
        v = jit[i]
        h = 1e-5 * max(1.0, abs(v))
        jit[i] = v + h; up = F()
        jit[i] = v - h; dn = F()
        jit[i] = v
        fd.append((up - dn) / (2 * h))
    fd = np.array(fd)
    scale = np.abs(fd).max()
    print(tag, 'gradient off by', np.abs(grad - fd).max() / scale, 'of its largest entry')
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-6 * scale)
    _assert_default_schedule(g._backend())


def test_elboaux_keeps_the_reference_order():
    """ELBOaux restates a reference function: its sweep runs in the reference's order whatever the object's, and the
    object's order is back afterwards."""
    tag = 'step_p3q2'
    pr = R.problem(tag)
    Kf, Kw, Lf, Lw, yres, y, yerr2, j2 = pr['args']
    out = {}
    for order in ('reference', 'sequential'):
        meta, d, g = _model(tag, order)
        out[order] = g.ELBOaux(Kf, Kw, Lf, Lw, yres, j2, d['mu_init'], d['var_init'])[:3]
        assert g.sweep_order == order
    for a, b in zip(out['reference'], out['sequential']):
        assert np.array_equal(a, b)
    E_s, _, _, _ = R.sweeps(*pr['args'], pr['mu0'], pr['var0'], 1, order='sequential')
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    ctx.set_muvar(d['mu_init'], d['var_init'])
    np.testing.assert_allclose(ctx.sweep(1)[0], E_s, rtol=RTOL)       # (the context is sequential again)
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ the C ABI's refusals
def test_refusals_through_the_c_abi(monkeypatch):
    lib = _hip.load_library()
    rng = np.random.RandomState(0)
    t, y, e = np.sort(rng.rand(20)) * 10, rng.randn(2, 20), rng.rand(2, 20) + 0.1
    mask = np.ones((2, 20), dtype=bool)
    mask[0, 3] = False
    # a value that is no order
    ctx = _hip.Context(0)
    ctx.set_data(t, y, e, 2)
    assert lib.gprn_set_sweep_order(ctx._h, 2) == _hip.GPRN_E_ARG
    assert lib.gprn_set_sweep_order(ctx._h, -1) == _hip.GPRN_E_ARG
    # mask, then order
    ctx.set_mask(mask)
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_SEQUENTIAL) == _hip.GPRN_E_UNSUPPORTED
    assert b'mask' in lib.gprn_last_error(ctx._h)
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_REFERENCE) == 0
    ctx.set_mask(None)
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_SEQUENTIAL) == 0
    # order, then mask
    assert lib.gprn_set_mask(ctx._h, np.ascontiguousarray(mask, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p)) == _hip.GPRN_E_UNSUPPORTED
    assert b'order' in lib.gprn_last_error(ctx._h)
    ctx.close()
    # order, then a communicator
    ctx = _hip.Context(0)
    ctx.set_sweep_order(_hip.ORDER_SEQUENTIAL)
    buf = ctypes.create_string_buffer(128)
    assert lib.gprn_comm_init(ctx._h, 2, 0, buf) == _hip.GPRN_E_UNSUPPORTED
    assert b'order' in lib.gprn_last_error(ctx._h)
    ctx.close()
    # a communicator (one rank, for real), then the order
    monkeypatch.setenv('GPRN_FORCE_RCCL', '1')
    ctx = _hip.Context(0)
    ctx.comm_init(1, 0, _hip.comm_unique_id())
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_SEQUENTIAL) == _hip.GPRN_E_UNSUPPORTED
    assert b'communicator' in lib.gprn_last_error(ctx._h)
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_REFERENCE) == 0
    ctx.close()
