"""The bound form of the ELBO on the GPU (inference(..., elbo='bound'), option "elbo_form") against its NumPy restatement
tests/_bound_ref.py: forced sweeps and ELBOcalc on every path (one tile, two tiles on the one-launch kernels, the launch
schedule, both sweep orders, data masks), that the form changes the reported value and nothing else, nELBO_batch slot by
slot, the gradient of every parameter class, and the refusals.  Tolerances: the project's own (1e-8 on the ELBO and its
parts, _cases.assert_state on the state).  No call may fall back to the event schedule."""
import ctypes
import functools
import os

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _bound_ref as BR, _cases, _grad_ref as GR, _mask_ref as MR

pytestmark = pytest.mark.gpu
RTOL = 1e-8
PROJECT_BOUND = 1e-8


def _mask(tag, seed):
    meta, _ = _cases.load(tag)
    return None if seed is None else MR.partial_mask(meta['p'], meta['N'], seed=seed)


def _model(tag, order='reference', seed=None, elbo='bound', **kw):
    """The fixture's model; under a mask the masked y / yerr of the host object are NaN / inf."""
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    y, e = np.array(d['y']), np.array(d['yerr'])
    mask = _mask(tag, seed)
    if mask is not None:
        y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
        kw = dict(kw, mask=mask, sequential_under_mask=order != 'reference')
    args = [a for i in range(y.shape[0]) for a in (y[i], e[i])]
    g = gpyrn.inference(meta['q'], np.array(d['time']), *args, sweep_order=order, elbo=elbo, **kw)
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


@functools.lru_cache(maxsize=None)
def _reference(tag, order, seed):
    """The restatement's ELBOcalc loop from _initMuVar, computed once per case and left alone: trips 1 .. 3 are the three
    forced sweeps (their values, parts and the state after them), the rest is the loop."""
    pr = BR.problem(tag)
    mask = _mask(tag, seed)
    mu0, var0 = (pr['mu0'], pr['var0']) if mask is None else MR.init_state(pr, mask)
    e, mu, var, it, hist, crit, parts, snap = BR.elbo_calc(*pr['args'], mu0, var0, mask=mask, order=order, snapshot=3)
    for a in (hist, crit, parts, mu, var) + snap:
        a.setflags(write=False)
    return dict(pr=pr, mask=mask, mu0=mu0, var0=var0, e=e, mu=mu, var=var, it=it, hist=hist, crit=crit, parts=parts, snap=snap)


# step_p3q2: N = 32, one tile; step_p2q3: N = 40, q = 3, sequential order; kmix_N200_p2q2: two tiles on the one-launch
# kernels (option small_path = 2); mid_N300_p3q2: three tiles, the launch schedule, both orders; and the two masked cases
CASES = [('step_p3q2', 'reference', None, None), ('step_p2q3', 'sequential', None, None),
         ('kmix_N200_p2q2', 'reference', None, 2), ('mid_N300_p3q2', 'reference', None, None),
         ('mid_N300_p3q2', 'sequential', None, None), ('step_p2q3', 'sequential', 3, None),
         ('mid_N300_p3q2', 'reference', 3, None)]


@pytest.mark.parametrize('tag,order,seed,small_path', CASES)
def test_forced_sweeps_match_the_restatement(tag, order, seed, small_path):
    """Three forced sweeps from _initMuVar: the bound and its parts of every sweep, the final state."""
    ref = _reference(tag, order, seed)
    meta, d, g = _model(tag, order, seed)
    ctx = _device(g, small_path)
    mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
    np.testing.assert_allclose(np.ravel(mu0), np.ravel(ref['mu0']), rtol=1e-13)
    ctx.set_muvar(mu0, var0)
    elbo, parts, info = ctx.sweep(3, commit=True)
    assert info == 0
    E, P = ref['hist'][1:4], ref['parts'][:3]
    print(tag, order, seed, 'bound', elbo, 'rel %.2e, parts rel %.2e' % (np.abs(elbo / E - 1).max(), np.abs(parts / P - 1).max()))
    np.testing.assert_allclose(elbo, E, rtol=RTOL)
    np.testing.assert_allclose(parts, P, rtol=RTOL)
    np.testing.assert_allclose(elbo, parts.sum(axis=1), rtol=1e-14)         # (not divided by q)
    mu, var = ctx.get_muvar()
    _cases.assert_state('bound, forced sweeps %s %s mask %s' % (tag, order, seed), mu, ref['snap'][0], var, ref['snap'][1])
    assert not np.any(ctx.get_scalars()['q1'])
    _assert_default_schedule(ctx)


@pytest.mark.parametrize('tag,order,seed,small_path', CASES)
def test_elbocalc_history_state_and_trip_count(tag, order, seed, small_path):
    """The stop rule is applied to the bound's values.  The trip count is comparable because the rule's criterion is away
    from its threshold on these cases: asserted here, on the restatement alone."""
    ref = _reference(tag, order, seed)
    assert ref['it'] > 3 and ref['crit'][-1] < 1e-3
    for c in ref['crit'][-2:]:
        assert abs(c - 1e-3) > 1e-6 * 1e-3
    meta, d, g = _model(tag, order, seed)
    if small_path is not None:
        g._backend().option('small_path', small_path)
    E, mu, var, it = g.ELBOcalc()
    print(tag, order, seed, 'trips', it, '(restatement %d)' % ref['it'], 'bound', E)
    assert g.last_info == 0
    assert it == ref['it']
    np.testing.assert_allclose(g._elbo_history, ref['hist'], rtol=RTOL)
    np.testing.assert_allclose(E, ref['e'], rtol=RTOL)
    _cases.assert_state('bound, ELBOcalc %s %s mask %s' % (tag, order, seed), mu, ref['mu'], var, ref['var'])
    _assert_default_schedule(g._backend())


# ------------------------------------------------------------------ the form changes only the value
# the four paths: one tile on the one-launch kernels, one tile on the launch schedule, two tiles on the one-launch kernels,
# three tiles on the launch schedule
@pytest.mark.parametrize('tag,order,small_path', [('step_p2q3', 'sequential', None), ('step_p3q2', 'reference', 0),
                                                  ('kmix_N200_p2q2', 'reference', 2), ('mid_N300_p3q2', 'reference', None)])
def test_the_form_changes_the_value_and_nothing_else(tag, order, small_path):
    out = {}
    for form in ('reference', 'bound'):
        meta, d, g = _model(tag, order, elbo=form)
        ctx = _device(g, small_path)
        ctx.set_muvar(d['mu_init'], d['var_init'])
        elbo, parts, info = ctx.sweep(3, commit=True)
        assert info == 0
        out[form] = (elbo, parts) + ctx.get_muvar() + (ctx.get_scalars(),)
        _assert_default_schedule(ctx)
    off, on = out['reference'], out['bound']
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])          # mu, var: the same bits
    np.testing.assert_allclose(on[1][:, 2], off[1][:, 2], rtol=1e-12)               # Ent
    assert not np.allclose(on[0], off[0], rtol=1e-3)
    for k in ('logdetB', 'trBinv'):
        assert np.array_equal(on[4][k], off[4][k])
    assert not np.any(on[4]['q1']) and np.any(off[4]['q1'])
    if order == 'reference':
        np.testing.assert_allclose(off[0], d['elbo_sweeps'][:3], rtol=RTOL)
    # back to the reference form on the context that was in the bound form: a new set-up is asked for, then the same bits
    ctx.set_muvar(d['mu_init'], d['var_init'])
    assert ctx.option('elbo_form', _hip.ELBO_REFERENCE) == _hip.ELBO_BOUND
    lib = _hip.load_library()
    one = np.zeros(1)
    assert lib.gprn_sweep(ctx._h, 1, 1, one.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None) == _hip.GPRN_E_ARG
    g.elbo = 'reference'
    ctx = _device(g, small_path)
    ctx.set_muvar(d['mu_init'], d['var_init'])
    elbo, parts, info = ctx.sweep(3, commit=True)
    back = (elbo, parts) + ctx.get_muvar()
    for a, b in zip(off[:4], back):
        assert np.array_equal(a, b)
    assert np.array_equal(ctx.get_scalars()['q1'], off[4]['q1'])
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ batches
def _perturbed(g, B, rel, seed=11):
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(seed)
    return x0, [x0 * (1.0 + rel * rng.standard_normal(x0.size)) for _ in range(B)]


def _set_vector(pr, x):
    """The full parameter vector x (nodes, weights, means, jitters) into the restatement's own components."""
    k = 0
    for o in list(pr['nodes']) + list(pr['weights']) + [m for m in pr['means'] if m is not None]:
        o.pars[:] = x[k:k + o.pars.size]
        k += o.pars.size
    pr['jitters'] = [float(v) for v in x[k:]]
    assert k + len(pr['jitters']) == len(x)


@pytest.mark.parametrize('seed,kw', [(None, {}), (2, {'batch_under_mask': True})])
def test_nelbo_batch_on_one_tile(seed, kw, capsys):
    """B = 5 vectors 1 % around the fixture's (kernel, mean-function and jitter parameters all move) side by side against
    the same evaluations one by one on the device, each from its own _initMuVar state; slot 0 against the restatement."""
    tag = 'step_p3q2'
    _, _, g = _model(tag, seed=seed, **kw)
    x0, sets = _perturbed(g, 5, 0.01)
    capsys.readouterr()
    got = np.array(g.nELBO_batch(sets))
    assert 'evaluations side by side' in capsys.readouterr().out, 'the list was evaluated one by one: no batched form?'
    assert g.last_info == 0 and np.all(np.isfinite(got))
    _, _, gs = _model(tag, seed=seed, **kw)
    want = []
    for x in sets:
        gs.set_parameters(x)
        want.append(-gs.ELBOcalc()[0])
    print(tag, seed, 'rel', np.abs(got / np.array(want) - 1).max())
    np.testing.assert_allclose(got, want, rtol=1e-9)
    pr = BR.problem(tag)
    _set_vector(pr, sets[0])
    mask = _mask(tag, seed)
    gs.set_parameters(sets[0])
    mu0, var0 = gs._initMuVar(gs.nodes, gs.weights, gs.jitters)
    e0 = BR.elbo_calc(*BR.setup_args(pr), mu0, var0, mask=mask)[0]
    np.testing.assert_allclose(got[0], -e0, rtol=RTOL)
    _assert_default_schedule(g._backend())
    _assert_default_schedule(gs._backend())


@pytest.mark.parametrize('seed,kw', [(None, {}), (3, {'batch_under_mask': True})])
def test_forced_batch_above_one_tile(seed, kw):
    """B = 3 on the launch schedule, GPRN_BATCH_FORCED with three trips, every vector from the fixture's start: slot by slot
    against three forced sweeps of that vector alone, slot 0 against the restatement."""
    tag = 'mid_N300_p3q2'
    meta, d, g = _model(tag, seed=seed, **kw)
    x0, sets = _perturbed(g, 3, 0.01)
    mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
    staged = g._batch_stage(sets, start=(mu0, var0))
    assert staged is not None
    ctx, kp, yr, jt, m0, v0 = staged
    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 3, want_state=True, forced=True)
    assert res is not None, 'no batched form?'
    elbo, it, conv, info, mu_b, var_b = res
    assert not np.any(info) and np.all(it == 3) and not np.any(conv)
    _, _, gs = _model(tag, seed=seed, **kw)
    for b, x in enumerate(sets):
        gs.set_parameters(x)
        c1 = _device(gs)
        c1.set_muvar(mu0, var0)
        e1, _, i1 = c1.sweep(3, commit=True)
        assert i1 == 0
        np.testing.assert_allclose(elbo[b], e1[-1], rtol=1e-9)
        mu1, var1 = c1.get_muvar()
        _cases.assert_state('bound, forced batch slot %d mask %s' % (b, seed), mu_b[b], mu1, var_b[b], var1)
    pr = BR.problem(tag)
    _set_vector(pr, sets[0])
    E, _, _, _ = BR.sweeps(*BR.setup_args(pr), mu0, var0, 3, mask=_mask(tag, seed))
    np.testing.assert_allclose(elbo[0], E[-1], rtol=RTOL)
    _assert_default_schedule(g._backend())
    _assert_default_schedule(gs._backend())


@pytest.mark.parametrize('tag', ['step_p3q2', 'mid_N300_p3q2'])
def test_a_batch_whose_vectors_differ_in_their_mean_functions_only(tag):
    """Per-vector residuals: the likelihood term of slot b must read y - mean of vector b (a read through the wrong stride,
    or of the shared raw y, fails here by orders of magnitude)."""
    meta, d, g = _model(tag)
    n_k = sum(k.pars.size for k in list(g.nodes) + list(g.weights))
    n_m = sum(m.pars.size for m in g.means if m is not None)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = []
    for b in range(4):
        x = x0.copy()
        x[n_k:n_k + n_m] = x0[n_k:n_k + n_m] * (1.0 + 0.5 * b) + 0.3 * b
        sets.append(x)
    mu0, var0 = np.array(d['mu_init'], dtype=float), np.array(d['var_init'], dtype=float)
    ctx, kp, yr, jt, m0, v0 = g._batch_stage(sets, start=(mu0, var0))
    assert np.ptp(yr, axis=0).max() > 0.1 and not np.ptp(kp, axis=0).any()
    elbo, it, conv, info = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 2, forced=True)
    assert not np.any(info)
    pr = BR.problem(tag)
    want = []
    for x in sets:
        _set_vector(pr, x)
        want.append(BR.sweeps(*BR.setup_args(pr), mu0, var0, 2)[0][-1])
    print(tag, 'bounds', elbo, 'rel', np.abs(elbo / np.array(want) - 1).max())
    assert np.ptp(want) > 1e-3 * abs(want[0])
    np.testing.assert_allclose(elbo, want, rtol=RTOL)
    _assert_default_schedule(ctx)


# ------------------------------------------------------------------ gradients
def _kernel_norm_bound(tag, exact):
    """The bound on the kernel entries in the norm |dev - ref| / sum |G| |dK/dtheta|, by the rule of
    tests/test_grad_fused_gpu.py: 100 x the spread of the restatement's two LAPACK routes, or the deviation of the
    REFERENCE form's one-call gradient from its own restatement (tests/_grad_ref.py) on the same fixture from the same
    state, whichever is larger -- never anything the bound form returned."""
    meta, d, g = _model(tag, elbo='reference', exact_derivatives=exact)
    pr = MR.problem(tag)
    st = GR.sweep_state(pr, np.array(d['mu_init']), np.array(d['var_init']), None)
    ref, norm = GR.kernel_gradient(pr, st, 'chol')
    ctx = _device(g)
    ctx.set_muvar(d['mu_init'], d['var_init'])
    _, _, info = ctx.sweep(1, commit=True)
    assert info == 0
    dev = ctx.grad_elbo(ref.size) / g.q
    return float((np.abs(dev - ref) / norm).max())


# kmix_N200_p2q2: composite kernels -- with exact_derivatives (by default they are differenced on the device, whose error is
# the differences', tests/test_grad_exact_gpu.py); the others: closed forms
@pytest.mark.parametrize('tag,exact', [('step_p3q2', False), ('kmix_N200_p2q2', True), ('mid_N300_p3q2', False)])
def test_gradient_of_every_parameter_class(tag, exact):
    """grad_ELBO() -- one committed sweep from the fixture's start, then the fixed-state gradient of THAT sweep's bound --
    and nELBO_and_grad_batch (two forced sweeps, two vectors) against the restatement."""
    meta, d, g = _model(tag, exact_derivatives=exact)
    shape = (meta['p'] + 1, meta['q'], meta['N'])
    mu0, var0 = np.array(d['mu_init'], dtype=float).reshape(shape), np.array(d['var_init'], dtype=float).reshape(shape)
    g._mu, g._var = mu0.copy(), var0.copy()
    E, grad = g.grad_ELBO()
    assert g.last_info == 0
    pr = BR.problem(tag)
    e1, mu1, var1, _ = BR.sweep(*pr['args'], mu0, var0)
    want, norm = BR.gradient(pr, pr['args'], mu0, var0, mu1, var1)
    want_inv, _ = BR.gradient(pr, pr['args'], mu0, var0, mu1, var1, route='inv')
    n_k = int(np.sum(np.isfinite(norm)))
    spread = float((np.abs(want - want_inv)[:n_k] / norm[:n_k]).max())
    parent = _kernel_norm_bound(tag, exact)
    off = float((np.abs(grad - want)[:n_k] / norm[:n_k]).max())
    rest = float(np.abs(grad[n_k:] / want[n_k:] - 1).max())
    print('%s: kernel entries %.2e (spread of the two routes %.2e, reference form on the same fixture %.2e); mean and '
          'jitter entries rel %.2e' % (tag, off, spread, parent, rest))
    np.testing.assert_allclose(E, e1, rtol=RTOL)
    assert grad.shape == want.shape == (len(g.get_parameters(include_frozen=True)),)
    assert off <= max(100.0 * spread, parent) and off <= PROJECT_BOUND
    np.testing.assert_allclose(grad[n_k:], want[n_k:], rtol=1e-8)
    assert np.all(grad[n_k:] != 0.0)
    # total=True and mean_sweeps change nothing: same sweep, same numbers
    g._mu, g._var = mu0.copy(), var0.copy()
    E2, grad2 = g.grad_ELBO(mean_sweeps=3, total=True)
    assert E2 == E and np.array_equal(grad2, grad)
    # ---- side by side
    x0, sets = _perturbed(g, 2, 0.01, seed=5)
    sets[0] = x0
    values, grads = g.nELBO_and_grad_batch(sets, sweeps=2, start=(mu0, var0))
    for b, x in enumerate(sets):
        _set_vector(pr, x)
        args = BR.setup_args(pr)
        _, mu_a, var_a, _ = BR.sweep(*args, mu0, var0)
        e_b, mu_b, var_b, _ = BR.sweep(*args, mu_a, var_a)
        want_b, norm_b = BR.gradient(pr, args, mu_a, var_a, mu_b, var_b)
        np.testing.assert_allclose(values[b], -e_b, rtol=RTOL)
        off_b = float((np.abs(-grads[b] - want_b)[:n_k] / norm_b[:n_k]).max())
        print('%s slot %d: kernel entries %.2e, the others rel %.2e' % (tag, b, off_b, np.abs(-grads[b, n_k:] / want_b[n_k:] - 1).max()))
        assert off_b <= max(100.0 * spread, parent) and off_b <= PROJECT_BOUND
        np.testing.assert_allclose(-grads[b, n_k:], want_b[n_k:], rtol=1e-8)
    _assert_default_schedule(g._backend())


def test_with_one_node_the_kernel_entries_are_the_reference_form_s():
    """q = 1: no cross term, the raw reshape is the identity, nothing to divide by -- the same launches on the same data."""
    out = {}
    for form in ('reference', 'bound'):
        meta, d, g = _model('step_p2q1', elbo=form)
        shape = (meta['p'] + 1, meta['q'], meta['N'])
        g._mu, g._var = np.array(d['mu_init'], dtype=float).reshape(shape), np.array(d['var_init'], dtype=float).reshape(shape)
        out[form] = g.grad_ELBO(mean_sweeps=0, fused=True)[1]
        _assert_default_schedule(g._backend())
    n_k = sum(k.pars.size for k in list(g.nodes) + list(g.weights))
    np.testing.assert_allclose(out['bound'][:n_k], out['reference'][:n_k], rtol=1e-12)
    assert not np.allclose(out['bound'][n_k:], out['reference'][n_k:], rtol=1e-3)      # (the means are not zero here)


def test_optimize_with_the_analytic_gradient_raises_the_bound():
    """optimize(jac=True) needs neither fused= nor a start state in the bound form; a few L-BFGS-B steps must not lower the
    bound they differentiate."""
    meta, d, g = _model('step_p3q2', order='sequential')
    e0 = g.ELBOcalc()[0]
    res = g.optimize(method='L-BFGS-B', jac=True, sweeps=30, options={'maxiter': 3})
    assert np.isfinite(res.fun) and 'forced sweeps' in res.objective
    g.set_parameters(res.x)
    g._mu = g._var = None
    e1 = g.ELBOcalc()[0]
    print('bound at the start %.6f, after three L-BFGS-B steps %.6f' % (e0, e1))
    assert e1 > e0
    _assert_default_schedule(g._backend())


# ------------------------------------------------------------------ refusals
def test_refusals_through_the_c_abi(monkeypatch):
    lib = _hip.load_library()
    rng = np.random.RandomState(0)
    t, y, e = np.sort(rng.rand(20)) * 10, rng.randn(2, 20), rng.rand(2, 20) + 0.1
    ctx = _hip.Context(0)
    ctx.set_data(t, y, e, 2)
    old = ctypes.c_int(-5)
    for bad in (2, 7):
        assert lib.gprn_set_option(ctx._h, b'elbo_form', bad, ctypes.byref(old)) == _hip.GPRN_E_ARG
    assert ctx.option('elbo_form') == _hip.ELBO_REFERENCE
    assert ctx.option('elbo_form', _hip.ELBO_BOUND) == _hip.ELBO_REFERENCE and ctx.option('elbo_form') == _hip.ELBO_BOUND
    # what needs the reference's pairing is refused while the bound form is on
    assert lib.gprn_keep_sigma(ctx._h, 1) == _hip.GPRN_E_UNSUPPORTED
    assert b'elbo_form' in lib.gprn_last_error(ctx._h)
    A = np.zeros((20, 20))
    pd = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.gprn_grad_matrices(ctx._h, 0, pd(A), pd(A.copy())) == _hip.GPRN_E_UNSUPPORTED
    assert b'elbo_form' in lib.gprn_last_error(ctx._h)
    assert lib.gprn_grad_kernel(ctx._h, 0, pd(np.zeros(20)), pd(np.zeros(8))) == _hip.GPRN_E_UNSUPPORTED
    assert b'elbo_form' in lib.gprn_last_error(ctx._h)
    assert lib.gprn_keep_sigma(ctx._h, 0) == 0
    # ... and the other way round
    assert ctx.option('elbo_form', _hip.ELBO_REFERENCE) == _hip.ELBO_BOUND
    assert lib.gprn_keep_sigma(ctx._h, 1) == 0
    assert lib.gprn_set_option(ctx._h, b'elbo_form', _hip.ELBO_BOUND, None) == _hip.GPRN_E_UNSUPPORTED
    assert b'keep_sigma' in lib.gprn_last_error(ctx._h)
    ctx.close()
    # the bound form, then a communicator
    ctx = _hip.Context(0)
    ctx.option('elbo_form', _hip.ELBO_BOUND)
    buf = ctypes.create_string_buffer(128)
    assert lib.gprn_comm_init(ctx._h, 2, 0, buf) == _hip.GPRN_E_UNSUPPORTED
    assert b'elbo_form' in lib.gprn_last_error(ctx._h)
    ctx.close()
    # a communicator (one rank, for real), then the bound form
    monkeypatch.setenv('GPRN_FORCE_RCCL', '1')
    ctx = _hip.Context(0)
    ctx.comm_init(1, 0, _hip.comm_unique_id())
    assert lib.gprn_set_option(ctx._h, b'elbo_form', _hip.ELBO_BOUND, None) == _hip.GPRN_E_UNSUPPORTED
    assert b'communicator' in lib.gprn_last_error(ctx._h)
    assert lib.gprn_set_option(ctx._h, b'elbo_form', _hip.ELBO_REFERENCE, None) == 0
    ctx.close()


def test_the_reference_restatements_keep_the_reference_form():
    """ELBOaux restates a reference function: the reference's value whatever the object's form, and the object's form is
    back on the device afterwards."""
    tag = 'step_p3q2'
    pr = BR.problem(tag)
    Kf, Kw, Lf, Lw, yres, yerr2, j2 = pr['args']
    out = {}
    for form in ('reference', 'bound'):
        meta, d, g = _model(tag, elbo=form)
        out[form] = g.ELBOaux(Kf, Kw, Lf, Lw, yres, j2, d['mu_init'], d['var_init'])[:3]
        assert g.elbo == form and g._backend().option('elbo_form') == g._ELBO_FORMS[form]
    for a, b in zip(out['reference'], out['bound']):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(out['bound'][0], d['elbo_sweeps'][0], rtol=RTOL)
    ctx = _device(g)                                           # (the context is in the bound form again)
    ctx.set_muvar(d['mu_init'], d['var_init'])
    np.testing.assert_allclose(ctx.sweep(1)[0][0], BR.sweep(*pr['args'], d['mu_init'], d['var_init'])[0], rtol=RTOL)
    with pytest.raises(NotImplementedError):
        gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d), elbo='bound', comm=object())
    _assert_default_schedule(ctx)
