"""The sequential sweep order under a data mask on the GPU (option "order_mask", inference(..., mask=,
sweep_order='sequential', sequential_under_mask=True)) against the dense restatement tests/_order_mask_ref.py: forced sweeps
on every path, what the two orders share bit for bit, the masked instantiations where nothing is selected away, q = 1,
ELBOcalc with its trip count, nELBO_batch slot by slot, grad_ELBO(fused=True) and the option through the C ABI.
Tolerances: the project's own (1e-8 on the ELBO and its parts, _cases.assert_state on the state, rows of zero precision
included).  No call may fall back to the event schedule."""
import ctypes
import os

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _cases, _grad_ref as GR, _mask_ref as M, _order_mask_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-8


def _model(tag, pr, mask, order='sequential', **kw):
    """The fixture's model on the problem `pr` (tests/_mask_ref.problem / inserted) under `mask` (None: no mask); the masked
    y / yerr handed over are NaN / inf."""
    meta, _ = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    if 'y_nan' in pr:
        y, e = pr['y_nan'], pr['yerr_inf']
    else:
        y, e = pr['y_raw'], np.sqrt(pr['yerr2'])
        if mask is not None:
            y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
    args = [a for i in range(y.shape[0]) for a in (y[i], e[i])]
    g = gpyrn.inference(meta['q'], pr['time'], *args, mask=mask, sweep_order=order, sequential_under_mask=True, **kw)
    g.set_components(nodes, weights, means, jit)
    return g


def _partial(tag, seed, order='sequential', **kw):
    pr = M.problem(tag)
    p, N = pr['y_raw'].shape
    mask = M.partial_mask(p, N, seed)
    assert not mask.all()
    return pr, mask, _model(tag, pr, mask, order, **kw)


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
# step_p3q2: one tile, the weights' refresh across p = 3 workgroups; step_p2q3: one tile, two later groups; kmix_N200_p2q2:
# T = 2 on the small path (option small_path = 2), ragged last tile, and the launch path (small_path = 0); mid_N300_p3q2:
# three tiles, |U| = 87 / 53 / 87, below one 128-row tile of U
@pytest.mark.parametrize('tag,seed,small_path', [('step_p3q2', 2, None), ('step_p2q3', 3, None), ('kmix_N200_p2q2', 3, 2),
                                                 ('kmix_N200_p2q2', 3, 0), ('mid_N300_p3q2', 4, None)])
def test_forced_sweeps_match_the_restatement(tag, seed, small_path):
    pr, mask, g = _partial(tag, seed)
    mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
    np.testing.assert_array_equal(mu0, M.init_state(pr, mask)[0])
    E, P, mu_r, var_r = R.sweeps(*R.args(pr), mu0, var0, mask, 3, order='sequential')
    ctx = _device(g, small_path)
    if tag == 'kmix_N200_p2q2':
        assert g.N == 200                                      # (two tiles, the second 72 rows)
    ctx.set_muvar(mu0, var0)
    elbo, parts, info = ctx.sweep(3, commit=True)
    assert info == 0
    print(tag, 'masked', (~mask).sum(axis=1), 'ELBO', elbo, 'rel', np.abs(elbo / E - 1).max(), 'parts rel', np.abs(parts / P - 1).max())
    np.testing.assert_allclose(elbo, E, rtol=RTOL)
    np.testing.assert_allclose(parts, P, rtol=RTOL)
    mu, var = ctx.get_muvar()
    _cases.assert_state('sequential under a mask, forced sweeps %s (small_path %s)' % (tag, small_path), mu,
                        mu_r.reshape(mu.shape), var, var_r.reshape(var.shape))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ what the orders share
@pytest.mark.parametrize('tag,seed,small_path', [('step_p3q2', 2, None), ('step_p2q3', 3, None), ('step_p2q3', 3, 0),
                                                 ('mid_N300_p3q2', 4, None)])
def test_first_sweep_shares_variances_and_group_zero_with_the_reference_order(tag, seed, small_path):
    """As tests/test_order_gpu.py compares them, rows of zero precision included (they take their variance from X, which no
    refresh touches)."""
    out = {}
    for order in ('reference', 'sequential'):
        pr, mask, g = _partial(tag, seed, order)
        ctx = _device(g, small_path)
        mu0, var0 = M.init_state(pr, mask)
        ctx.set_muvar(mu0, var0)
        _, _, info = ctx.sweep(1, commit=True)
        assert info == 0
        out[order] = ctx.get_muvar()
        _assert_default_schedule(ctx)
    (mu_r, var_r), (mu_s, var_s) = out['reference'], out['sequential']
    assert not mask[0].all()                                   # (output 0 has rows of zero precision)
    assert np.array_equal(var_s[0], var_r[0])                  # every node variance
    assert np.array_equal(mu_s[0, 0], mu_r[0, 0])              # mu_f0
    assert np.array_equal(var_s[1:, 0], var_r[1:, 0])          # the variances of node 0's weights
    assert not np.allclose(mu_s[0, 1], mu_r[0, 1], rtol=1e-6, atol=0)


# ------------------------------------------------------------------ the masked instantiations where nothing is selected away
@pytest.mark.parametrize('tag', ['step_p2q3', 'mid_N300_p3q2'])
def test_an_all_true_mask_on_the_context_is_bit_identical_to_no_mask(tag):
    """inference hands an all-True mask to nobody; Context.set_mask takes it, and every masked kernel runs -- order.hip's
    refresh among them."""
    pr = M.problem(tag)
    out = []
    for masked in (False, True):
        g = _model(tag, pr, None)
        ctx = g._backend()
        if masked:
            ctx.set_mask(np.ones(pr['y_raw'].shape, dtype=bool))
        ctx = _device(g)
        mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
        ctx.set_muvar(mu0, var0)
        elbo, parts, info = ctx.sweep(3, commit=True)
        assert info == 0
        out.append((elbo, parts) + ctx.get_muvar())
        _assert_default_schedule(ctx)
    for a, b in zip(*out):
        assert np.array_equal(a, b)
        assert np.all(np.isfinite(a))


# ------------------------------------------------------------------ q = 1
def test_with_one_node_and_all_masked_times_the_orders_are_bit_identical():
    tag = 'step_p2q1'
    pr, mask, pos = M.inserted(tag)
    assert pr['meta']['q'] == 1 and (~mask.any(axis=0)).sum() > 0
    out = {}
    for order in ('reference', 'sequential'):
        g = _model(tag, pr, mask, order)
        ctx = _device(g)
        mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
        ctx.set_muvar(mu0, var0)
        elbo, parts, _ = ctx.sweep(3, commit=True)
        out[order] = (elbo, parts) + ctx.get_muvar() + g.ELBOcalc()[:3]
        _assert_default_schedule(ctx)
    for a, b in zip(out['reference'], out['sequential']):
        assert np.array_equal(a, b)
        assert np.all(np.isfinite(a))


# ------------------------------------------------------------------ ELBOcalc
# step_p2q3, seed 3: the problem the reference's order diverges on (17 trips); mid_N300_p3q2: seed 4, the first tried (the
# restatement's criterion there: 1.50e-3 before the firing trip, 3.3e-4 at it)
@pytest.mark.parametrize('tag,seed,trips', [('step_p2q3', 3, 17), ('mid_N300_p3q2', 4, 7)])
def test_elbocalc_history_state_and_trip_count(tag, seed, trips):
    """The trip count is comparable because the rule's criterion is away from its threshold: asserted here, on the
    restatement alone (1e-6 relative at the firing trip and the one before)."""
    pr, mask, g = _partial(tag, seed)
    mu0, var0 = M.init_state(pr, mask)
    e_r, mu_r, var_r, it_r, hist_r, crit = R.elbo_calc(*R.args(pr), mu0, var0, mask, order='sequential')
    print(tag, 'restatement: trips', it_r, 'ELBO', hist_r[1], '->', e_r, 'criterion', crit[-2:])
    assert it_r == trips and crit[-1] < 1e-3
    for c in crit[-2:]:
        assert abs(c - 1e-3) > 1e-6 * 1e-3
    E, mu, var, it = g.ELBOcalc()
    print(tag, 'device: trips', it, 'ELBO', E)
    assert g.last_info == 0
    assert it == it_r
    np.testing.assert_allclose(g._elbo_history, hist_r, rtol=RTOL)
    np.testing.assert_allclose(E, e_r, rtol=RTOL)
    _cases.assert_state('sequential under a mask, ELBOcalc ' + tag, mu, mu_r.reshape(mu.shape), var, var_r.reshape(var.shape))
    _assert_default_schedule(g._backend())


# ------------------------------------------------------------------ nELBO_batch
@pytest.mark.parametrize('tag,seed,B', [('step_p2q3', 3, 5), ('mid_N300_p3q2', 4, 7)])
def test_nelbo_batch_slots_equal_one_by_one_evaluation(tag, seed, B, capsys):
    """tests/test_order_gpu.py's comparison with batch_under_mask = True: B perturbed parameter vectors side by side against
    the same evaluations one by one from the same starting state, cold (each from its own _initMuVar state) and warm (all
    from one converged state): the one-tile batch and midn.hip's worker."""
    _, _, g = _partial(tag, seed, batch_under_mask=True)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(11)
    sets = [x0 * (1.0 + 0.05 * rng.standard_normal(x0.size)) + 0.01 * rng.standard_normal(x0.size) * (x0 == 0)
            for _ in range(B)]
    capsys.readouterr()
    got = np.array(g.nELBO_batch(sets))
    assert 'evaluations side by side' in capsys.readouterr().out, 'the list was evaluated one by one: no batched form?'
    assert g.last_info == 0 and np.all(np.isfinite(got))
    _, _, gs = _partial(tag, seed)
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
@pytest.mark.parametrize('tag,seed', [('step_p3q2', 2), ('mid_N300_p3q2', 4)])
def test_fused_grad_elbo_under_the_sequential_order_and_a_mask(tag, seed):
    """tests/test_order_gpu.py::test_grad_elbo_under_the_sequential_order's procedure and tolerances: the returned ELBO is the
    restatement's one further sequential sweep under the mask, the gradient the central differences of the masked fixed-state
    ELBO (tests/_grad_ref.py) at that sweep's state, with that sweep's explicit covariances."""
    pr, mask, g = _partial(tag, seed)
    g.ELBOcalc()
    mu_prev, var_prev = g._mu.copy(), g._var.copy()
    E, grad = g.grad_ELBO(mean_sweeps=0, fused=True)
    assert grad.shape == (len(g.get_parameters(include_frozen=True)),) and np.all(np.isfinite(grad))
    E_ref, mu_n, var_n, parts, sig_f, sig_w = R.sweep(*R.args(pr), mu_prev, var_prev, mask, order='sequential', return_sigma=True)
    print(tag, 'ELBO', E, 'restatement', E_ref)
    np.testing.assert_allclose(E, E_ref, rtol=RTOL)
    _cases.assert_state('sequential under a mask, grad_ELBO sweep ' + tag, g._mu, mu_n.reshape(g._mu.shape), g._var,
                        var_n.reshape(g._var.shape))
    p, N = mask.shape
    st = dict(elbo=E_ref, mu=mu_n, var=var_n, sig_f=sig_f, sig_w=sig_w, mask=mask, y_raw=np.where(mask, pr['y_raw'], 0.0),
              p=p, q=pr['meta']['q'], N=N)
    fd = GR.finite_differences(pr, st)
    scale = np.abs(fd).max()
    print(tag, 'gradient off by', np.abs(grad - fd).max() / scale, 'of its largest entry')
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-6 * scale)
    _assert_default_schedule(g._backend())


# ------------------------------------------------------------------ the option through the C ABI
def test_the_option_through_the_c_abi():
    lib = _hip.load_library()
    rng = np.random.RandomState(0)
    t, y, e = np.sort(rng.rand(20)) * 10, rng.randn(2, 20), rng.rand(2, 20) + 0.1
    mask = np.ones((2, 20), dtype=bool)
    mask[0, 3] = False
    pm = np.ascontiguousarray(mask, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p)

    def set_option(ctx, value):
        return lib.gprn_set_option(ctx._h, b'order_mask', value, None)

    ctx = _hip.Context(0)
    ctx.set_data(t, y, e, 2)
    assert ctx.option('order_mask') == 0                       # the default: each refuses the other
    assert set_option(ctx, 2) == _hip.GPRN_E_ARG
    assert ctx.option('order_mask', 1) == 0
    # mask, then order
    assert lib.gprn_set_mask(ctx._h, pm) == 0
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_SEQUENTIAL) == 0
    # not switched off while both are in force
    assert set_option(ctx, 0) == _hip.GPRN_E_UNSUPPORTED
    msg = lib.gprn_last_error(ctx._h)
    assert b'mask' in msg and b'order' in msg
    assert ctx.option('order_mask') == 1
    # after dropping the mask it can be
    assert lib.gprn_set_mask(ctx._h, None) == 0
    assert set_option(ctx, 0) == 0
    # ... and the mask is refused again (the order is still the sequential one)
    assert lib.gprn_set_mask(ctx._h, pm) == _hip.GPRN_E_UNSUPPORTED
    assert b'order' in lib.gprn_last_error(ctx._h)
    # order, then mask
    assert set_option(ctx, 1) == 0
    assert lib.gprn_set_mask(ctx._h, pm) == 0
    assert set_option(ctx, 0) == _hip.GPRN_E_UNSUPPORTED
    # after going back to the reference's order it can be switched off as well
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_REFERENCE) == 0
    assert set_option(ctx, 0) == 0
    assert lib.gprn_set_sweep_order(ctx._h, _hip.ORDER_SEQUENTIAL) == _hip.GPRN_E_UNSUPPORTED
    assert b'mask' in lib.gprn_last_error(ctx._h)
    # gprn_keep_sigma stays refused under a mask whatever the option says
    assert set_option(ctx, 1) == 0
    assert lib.gprn_keep_sigma(ctx._h, 1) == _hip.GPRN_E_UNSUPPORTED
    assert ctx.option('fallbacks') == 0
    ctx.close()
