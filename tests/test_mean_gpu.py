"""Mean programs on the GPU (csrc/mean.hip: gprn_set_mean, gprn_eval_mean, gprn_eval_mean_grad) against the 40-digit reference
tests/golden/mean_highprec, to the bound of tests/_mean_fixture.py -- (4 |m| + 2 kappa) 2^-53, the bound NumPy's own
evaluation is held to in tests/test_mean_keplerian.py, c0 raised for no case:

1. every fixture case, value and every derivative, one program on one output;
2. p = 3 mixing programs -- output 0 Keplerian + Constant, output 1 no mean, output 2 Sine * Linear + Cubic -- with
   n_eval in {1, 3}, each evaluation at its own parameters, and nt in {1, 45, 257}, the last crossing a workgroup; the data
   times (t = NULL) give the bits of the same times passed explicitly; two calls return the same bits;
3. a Keplerian out of range poisons its own evaluation only: the others return the bits they return without it;
4. what is refused;
5. ``inference(..., device_means=True)``: ``_mean_values_batch`` (behind ``predict_batch`` / ``posterior_predictive``) makes
   ONE gprn_eval_mean call and meets the bound per vector; with the option off the entry point is not called;
6. the side-by-side ELBO batches under ``device_means=True`` (``_batch_stage``'s third layout: y - mean of all B vectors
   formed on the device inside gprn_elbocalc_batch_means): ``nELBO_batch`` against the same vectors one by one from the same start, the project's 1e-8 on
   the ELBO and ``_cases.assert_state`` on the states, at N = 45, p = 2, q = 1, B = 5 (one tile) and N = 200, p = 2, q = 2,
   B = 3 (above one tile); at N = 45 under a mask with ``batch_under_mask=True`` and NaN y at the masked entries; the bound
   form's mean entries (``_mean_grads_batch``: one gprn_eval_mean_grad call) against the contraction with the fixture-pinned
   derivatives; one vector with e = 1.2 among five returns inf and the other four the bits they return without it; with the
   option off ``nELBO_batch`` on a Linear mean calls neither new entry point; a two-planet model through
   ``mcmc(batch=True)`` under the emcee stand-in;
7. gprn_elbocalc_batch_means itself: against gprn_elbocalc_batch_grad fed its own ``resid_out``, bit for bit (elbo, iterations,
   converged, info, states, grad_out), at both shapes and once more in chunks (``batch_mem_mb``: chunks of 2 above one tile;
   a one-tile chunk holds sixteen evaluations at least, so there B = 20 in chunks of 16), ``resid_out`` against the data
   minus gprn_eval_mean's bits; ``mean_grad_out`` against the host contraction of the RETURNED state with the
   fixture-pinned derivatives, allowed sum_n |w_n| allowed_n + N 2^-53 sum_n |w_n dm_n|, the same bits from two calls, and
   ``nELBO_and_grad_batch``'s mean entries being those rows; under a mask with NaN y against the host path; the refusals."""
import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc

from . import _mean_fixture as fx

pytestmark = pytest.mark.gpu

META, D = fx.load()
CASES = META['cases']
BY_NAME = {c['name']: c for c in CASES}


def _context(p, t):
    ctx = _hip.Context(0)
    ctx.set_data(t, np.zeros((p, t.size)), np.ones((p, t.size)), 1)
    return ctx


@pytest.fixture(scope='module')
def ctx1():
    ctx = _context(1, D['t_A'])
    yield ctx
    ctx.close()


@pytest.fixture(scope='module')
def ctx3():
    ctx = _context(3, D['t_mix45'])
    yield ctx
    ctx.close()


def _check(what, values, ref):
    ratios = []
    bad = fx.violations(values, ref, ratios=ratios)
    print('%-40s %.3f of the bound' % (what, ratios[0]))
    assert not bad, (what, bad[:5])


@pytest.mark.parametrize('case', [c for c in CASES if not c['name'].startswith('mix_')],
                         ids=[c['name'] for c in CASES if not c['name'].startswith('mix_')])
def test_every_fixture_case(ctx1, case):
    mean = fx.build(case)
    ops, par = mean._device_program()
    ctx1.set_mean(0, ops, par)
    t = fx.times(case, D)
    ref_v, ref_d = fx.reference(case, D)
    val = ctx1.eval_mean(par[None], t)
    der = ctx1.eval_mean_grad(par[None], t)
    assert val.shape == (1, 1, t.size) and der.shape == (1, par.size, t.size)
    _check(case['name'] + ' value', val[0, 0], ref_v)
    _check(case['name'] + ' derivatives', der[0], ref_d)


def _mix_programs(ctx):
    rows = []
    for s in range(3):
        m0, m2 = fx.build(BY_NAME[f'mix_set{s}_out0_nt1']), fx.build(BY_NAME[f'mix_set{s}_out2_nt1'])
        (ops0, par0), (ops2, par2) = m0._device_program(), m2._device_program()
        rows.append(np.r_[par0, par2])
    ctx.set_mean(0, ops0, par0)
    ctx.set_mean(1, None, None)
    ctx.set_mean(2, ops2, par2)
    return np.array(rows), par0.size


@pytest.mark.parametrize('nt', [1, 45, 257])
@pytest.mark.parametrize('n_eval', [1, 3])
def test_three_outputs_mixing_programs(ctx3, n_eval, nt):
    rows, n0 = _mix_programs(ctx3)
    rows = rows[:n_eval]
    t = D[f't_mix{nt}']
    val, der = ctx3.eval_mean(rows, t), ctx3.eval_mean_grad(rows, t)
    assert val.shape == (n_eval, 3, nt) and der.shape == (n_eval, rows.shape[1], nt)
    assert np.all(val[:, 1] == 0.0)
    for e in range(n_eval):
        for o, sl in ((0, slice(0, n0)), (2, slice(n0, None))):
            case = BY_NAME[f'mix_set{e}_out{o}_nt{nt}']
            ref_v, ref_d = fx.reference(case, D)
            _check(case['name'] + ' value', val[e, o], ref_v)
            _check(case['name'] + ' derivatives', der[e, sl], ref_d)
    # a fixed order: the same bits again
    assert np.array_equal(val, ctx3.eval_mean(rows, t), equal_nan=True)
    assert np.array_equal(der, ctx3.eval_mean_grad(rows, t), equal_nan=True)
    if nt == 45:                                         # the data times are these times
        assert np.array_equal(val, ctx3.eval_mean(rows))
        assert np.array_equal(der, ctx3.eval_mean_grad(rows))


@pytest.mark.parametrize('poison', [(2, 1.2), (2, -0.1), (0, 0.0), (1, np.nan), (4, np.inf)])
def test_a_keplerian_out_of_range_poisons_its_own_evaluation_only(ctx3, poison):
    rows, n0 = _mix_programs(ctx3)
    t = D['t_mix45']
    clean_v, clean_d = ctx3.eval_mean(rows, t), ctx3.eval_mean_grad(rows, t)
    bad = rows.copy()
    bad[1, poison[0]] = poison[1]
    val, der = ctx3.eval_mean(bad, t), ctx3.eval_mean_grad(bad, t)
    assert np.isnan(val[1, 0]).all() and np.isnan(der[1, :5]).all()
    assert np.array_equal(val[1, 1:], clean_v[1, 1:]) and np.array_equal(der[1, n0:], clean_d[1, n0:])
    for e in (0, 2):
        assert np.array_equal(val[e], clean_v[e]) and np.array_equal(der[e], clean_d[e])


def test_refusals(ctx3):
    rows, _ = _mix_programs(ctx3)
    with pytest.raises(_hip.BackendError):
        ctx3.eval_mean(rows[:, :-1], D['t_mix45'])       # not the sum of the programs' parameters
    with pytest.raises(_hip.BackendError):
        ctx3.set_mean(3, [(0, 0, 0)], [1.0])             # no such output
    with pytest.raises(_hip.BackendError):
        ctx3.set_mean(0, [(0, meanfunc.MID['KEPLERIAN'], 0)], [1.0, 2.0])      # the leaf's parameters run past n_params
    with pytest.raises(_hip.BackendError):
        ctx3.set_mean(0, [(0, 0, 0), (1, 0, 0)], [1.0])  # an operator without two operands
    with pytest.raises(_hip.BackendError):
        ctx3.set_mean(0, [(0, 9, 0)], [1.0])             # no such mean
    deep = [(0, 0, 0)] * 9 + [(1, 0, 0)] * 8
    with pytest.raises(_hip.BackendError):
        ctx3.set_mean(0, deep, [1.0])
    # a refused program leaves the one before it
    assert ctx3.eval_mean(rows, D['t_mix1']).shape == (3, 3, 1)
    ctx3.set_mean(0, None, None)
    ctx3.set_mean(2, None, None)
    assert np.all(ctx3.eval_mean(np.zeros((2, 0)), D['t_mix45']) == 0.0)


# ------------------------------------------------------------------ inference(..., device_means=)
def _model(device_means, means):
    t = D['t_mix45']
    r = np.random.RandomState(5)
    y, e = r.randn(3, 45), 0.1 + r.rand(3, 45)
    g = gpyrn.inference(1, t, y[0], e[0], y[1], e[1], y[2], e[2], device_means=device_means)
    g.set_components(covfunc.SquaredExponential(1.0, 5.0), [covfunc.SquaredExponential(1.0, 9.0) for _ in range(3)],
                     means, [0.1, 0.2, 0.3])
    return g


def _count_calls(monkeypatch):
    calls = []
    inner = _hip.Context.eval_mean
    monkeypatch.setattr(_hip.Context, 'eval_mean', lambda self, *a, **k: calls.append(1) or inner(self, *a, **k))
    return calls


def _count_fused(monkeypatch):
    """calls of Context.elbocalc_batch that form y - mean on the device (gprn_elbocalc_batch_means)"""
    calls = []
    inner = _hip.Context.elbocalc_batch

    def counted(self, kp, yr, *a, **k):
        if isinstance(yr, _hip.MeanParams):
            calls.append(1)
        return inner(self, kp, yr, *a, **k)
    monkeypatch.setattr(_hip.Context, 'elbocalc_batch', counted)
    return calls


def test_mean_values_batch_on_the_device(monkeypatch):
    sets = [[fx.build(BY_NAME[f'mix_set{s}_out0_nt45']), meanfunc.Constant(0.25 * s),
             fx.build(BY_NAME[f'mix_set{s}_out2_nt45'])] for s in range(3)]
    g = _model(True, sets[0])
    vecs = []
    for means in sets:
        x = g.get_parameters(include_frozen=True).copy()
        x[8:-3] = np.concatenate([m_.pars for m_ in means])
        vecs.append(x)
    calls = _count_calls(monkeypatch)
    out = g._mean_values_batch(vecs, D['t_mix45'])
    assert len(calls) == 1 and out.shape == (3, 3, 45)
    for s in range(3):
        for o in (0, 2):
            _check(f'vector {s} output {o}', out[s, o], fx.reference(BY_NAME[f'mix_set{s}_out{o}_nt45'], D)[0])
        assert np.all(out[s, 1] == 0.25 * s)
    assert np.array_equal(g.get_parameters(include_frozen=True), vecs[-1])


def test_option_off_keeps_the_host_path(monkeypatch):
    means = [meanfunc.Linear(0.03, -2.0), meanfunc.Constant(0.0), meanfunc.Sine(2.5, 7.7, 0.4)]
    on, off = _model(True, means), _model(False, [meanfunc.Linear(0.03, -2.0), meanfunc.Constant(0.0), meanfunc.Sine(2.5, 7.7, 0.4)])
    x = off.get_parameters()
    vecs = [x * (1 + 0.01 * k) for k in range(3)]
    tstar = np.linspace(-3.0, 66.0, 31)
    calls = _count_calls(monkeypatch)
    host = off._mean_values_batch(vecs, tstar)
    assert not calls
    dev = on._mean_values_batch(vecs, tstar)
    assert len(calls) == 1
    # both evaluate the same formulas in fp64: a handful of roundings of values of size |m|, at arguments of size 2 pi t / P
    scale = np.abs(host).max(axis=2, keepdims=True)
    assert np.all(np.abs(dev - host) <= 64 * 2.0 ** -53 * (1 + 2 * np.pi * 66.0 / 7.7) * scale)


# ------------------------------------------------------------------ the side-by-side ELBO batches under device_means
def _rv_model(N, p, q, device_means, mask=None, nan_under_mask=False, two_planets=False, **kw):
    """a planet in output 0 over p outputs on N times in [0, 60]; the same numbers for every call with the same arguments"""
    r = np.random.RandomState(100 + N)
    t = np.sort(r.uniform(0.0, 60.0, N))
    planet = meanfunc.Keplerian(11.3, 3.7, 0.4, 0.8, 2.1)
    y = 0.3 * r.randn(p, N)
    y[0] += planet(t)
    e = 0.1 + 0.1 * r.rand(p, N)
    if mask is not None and nan_under_mask:
        y, e = np.where(mask, y, np.nan), np.where(mask, e, np.nan)
    args = [a for i in range(p) for a in (y[i], e[i])]
    g = gpyrn.inference(q, t, *args, device_means=device_means, mask=mask, **kw)
    first = meanfunc.Keplerian(11.0, 3.5, 0.35, 0.7, 2.0) + meanfunc.Constant(0.1)
    if two_planets:
        first = meanfunc.Keplerian(11.0, 3.5, 0.35, 0.7, 2.0) + meanfunc.Keplerian(27.0, 0.5, 0.1, 2.0, 9.0)
    means = [first] + [meanfunc.Linear(0.001, 0.05) for _ in range(p - 1)]
    g.set_components([covfunc.SquaredExponential(1.0, 7.0 + j) for j in range(q)],
                     [covfunc.SquaredExponential(0.5, 15.0 + k) for k in range(q * p)], means, [0.2] * p)
    return g


def _perturbed(x0, B):
    r = np.random.RandomState(8)
    return [x0 * (1 + 0.02 * r.uniform(-1, 1, x0.size)) for _ in range(B)]


MAX_ITER = 40
SHAPES = [(45, 2, 1, 5), (200, 2, 2, 3)]                # the one-tile path; above one tile


@pytest.mark.parametrize('N,p,q,B', SHAPES)
def test_nelbo_batch_with_device_means_against_one_by_one(monkeypatch, N, p, q, B):
    g, g1 = _rv_model(N, p, q, True), _rv_model(N, p, q, False)
    x0 = np.array(g.get_parameters(), dtype=float)
    _, mu0, var0, _ = g1.ELBOcalc(max_iter=MAX_ITER)
    g._mu, g._var = np.array(mu0), np.array(var0)       # both start every vector from this state
    sets = _perturbed(x0, B)
    calls, fused = _count_calls(monkeypatch), _count_fused(monkeypatch)
    staged = g._batch_stage(sets)
    assert staged is not None and isinstance(staged[2], _hip.MeanParams)       # the third layout: the mean columns, no array
    g.set_parameters(x0.copy())
    g._mu, g._var = np.array(mu0), np.array(var0)
    vals = g.nELBO_batch(sets, max_iter=MAX_ITER)
    assert len(fused) == 1 and not calls                # one fused call, y - mean never on the host
    for b, x in enumerate(sets):
        g1.set_parameters(x.copy())
        e, mu_1, var_1, _ = g1.ELBOcalc(max_iter=MAX_ITER, mu=np.array(mu0), var=np.array(var0))
        print('device_means N %d vector %d: nELBO %.10f one by one %.10f' % (N, b, vals[b], -e))
        np.testing.assert_allclose(vals[b], -e, rtol=1e-8)
    # the states, side by side from the same start, against the last vector's own loop
    g.set_parameters(x0.copy())
    g._mu, g._var = np.array(mu0), np.array(var0)
    mu_b, var_b = g._final_states(sets, MAX_ITER)
    from . import _cases
    _cases.assert_state('device_means N %d last vector' % N, mu_b[-1], mu_1, var_b[-1], var_1)


def test_nelbo_batch_with_device_means_under_a_mask(monkeypatch):
    N, p, q, B = 45, 2, 1, 5
    mask = np.random.RandomState(2).rand(p, N) > 0.2
    g = _rv_model(N, p, q, True, mask=mask, nan_under_mask=True, batch_under_mask=True)
    g1 = _rv_model(N, p, q, False, mask=mask, batch_under_mask=True)
    x0 = np.array(g.get_parameters(), dtype=float)
    _, mu0, var0, _ = g1.ELBOcalc(max_iter=MAX_ITER)
    g._mu, g._var = np.array(mu0), np.array(var0)
    sets = _perturbed(x0, B)
    calls = _count_fused(monkeypatch)
    vals = g.nELBO_batch(sets, max_iter=MAX_ITER)
    assert len(calls) == 1 and np.isfinite(vals).all()
    for b, x in enumerate(sets):
        g1.set_parameters(x.copy())
        e = g1.ELBOcalc(max_iter=MAX_ITER, mu=np.array(mu0), var=np.array(var0))[0]
        np.testing.assert_allclose(vals[b], -e, rtol=1e-8)


def test_mean_gradient_entries_against_the_pinned_derivatives():
    """``_mean_grads_batch`` under device_means (one gprn_eval_mean_grad call, contracted on the host) against the
    contraction of the same weights with the fixture's 40-digit derivatives: the deviation allowed is the sum of the terms'
    bounds plus the summation's own rounding, sum_n |w_n| allowed_n + N 2^-53 sum_n |w_n dm_n|."""
    sets = [[fx.build(BY_NAME[f'mix_set{s}_out0_nt45']), meanfunc.Constant(0.25 * s),
             fx.build(BY_NAME[f'mix_set{s}_out2_nt45'])] for s in range(3)]
    g = _model(True, sets[0])
    vecs = []
    for means in sets:
        x = g.get_parameters(include_frozen=True).copy()
        x[8:-3] = np.concatenate([m_.pars for m_ in means])
        vecs.append(x)
    r = np.random.RandomState(4)
    N = 45
    mu, resid, jit = r.randn(3, 4, 1, N), r.randn(3, 3, N), 0.1 + r.rand(3, 3)
    got = g._mean_grads_batch(vecs, jit, mu, resid)
    fit = np.einsum('biqn,bqn->bin', mu[:, 1:], mu[:, 0])
    w = (resid - fit) / (jit[:, :, None] ** 2 + g.yerr2[None])
    assert got.shape == (3, 16)
    for s in range(3):
        col = 0
        for o in (0, 1, 2):
            if o == 1:
                ref, lim = w[s, 1].sum(), N * 2.0 ** -53 * np.abs(w[s, 1]).sum()
                assert abs(got[s, col] - ref) <= lim
                col += 1
                continue
            hi, lo, kap = fx.reference(BY_NAME[f'mix_set{s}_out{o}_nt45'], D)[1]
            for k in range(hi.shape[0]):
                ref = float(np.sum(np.array([float(a) for a in hi[k] * w[s, o]])) + np.sum(lo[k] * w[s, o]))
                lim = np.sum(np.abs(w[s, o]) * fx.allowed((hi[k], lo[k], kap[k]))) + \
                    N * 2.0 ** -53 * np.sum(np.abs(w[s, o] * hi[k]))
                assert abs(got[s, col] - ref) <= lim, (s, o, k, got[s, col], ref, lim)
                col += 1


def test_a_poisoned_vector_returns_inf_and_leaves_the_others_their_bits():
    """nELBO_and_grad_batch in the bound form: e = 1.2 in one vector of five gives inf and a zero gradient row there, and
    the other four the bits they return without it; the clean call agrees with the option off to the project's 1e-8
    (values, and gradient rows against their largest entry)."""
    N, p, q, B = 45, 2, 1, 5
    g, g_off = _rv_model(N, p, q, True, elbo='bound'), _rv_model(N, p, q, False, elbo='bound')
    x0 = np.array(g.get_parameters(), dtype=float)
    _, mu0, var0, _ = g_off.ELBOcalc(max_iter=MAX_ITER)
    sets = _perturbed(x0, B)
    ie = next(i for i, n in enumerate(g.parameters_dict) if n.endswith('.e'))
    assert 0 < sets[2][ie] < 1

    def run(obj, vectors):
        obj.set_parameters(x0.copy())
        return obj.nELBO_and_grad_batch(vectors, sweeps=3, start=(np.array(mu0), np.array(var0)))
    clean_v, clean_g = run(g, sets)
    off_v, off_g = run(g_off, sets)
    assert np.isfinite(clean_v).all() and np.abs(clean_g[:, ie]).min() > 0
    np.testing.assert_allclose(clean_v, off_v, rtol=1e-8)
    assert np.all(np.abs(clean_g - off_g).max(axis=1) <= 1e-8 * np.abs(off_g).max(axis=1))
    bad = [x.copy() for x in sets]
    bad[2][ie] = 1.2
    vals, grads = run(g, bad)
    assert vals[2] == np.inf and np.all(grads[2] == 0.0)
    keep = [0, 1, 3, 4]
    assert np.array_equal(np.array(vals)[keep], np.array(clean_v)[keep]) and np.array_equal(grads[keep], clean_g[keep])
    # nELBO_batch reports a non-finite ELBO as it always has: the value itself
    g.set_parameters(x0.copy())
    g._mu, g._var = np.array(mu0), np.array(var0)
    plain = g.nELBO_batch(bad, max_iter=MAX_ITER)
    assert not np.isfinite(plain[2]) and np.isfinite(np.array(plain)[keep]).all()


def test_option_off_nelbo_batch_never_calls_the_new_entry_points(monkeypatch):
    g = _rv_model(45, 2, 1, False)
    g.means[0] = meanfunc.Linear(0.01, 0.2)
    g.set_components(g.nodes, g.weights, [meanfunc.Linear(0.01, 0.2), meanfunc.Linear(0.001, 0.05)], [0.2, 0.2])
    calls = _count_calls(monkeypatch)
    grad_calls = []
    inner = _hip.Context.eval_mean_grad
    monkeypatch.setattr(_hip.Context, 'eval_mean_grad', lambda self, *a, **k: grad_calls.append(1) or inner(self, *a, **k))
    x0 = np.array(g.get_parameters(), dtype=float)
    g.ELBOcalc(max_iter=MAX_ITER)
    vals = g.nELBO_batch(_perturbed(x0, 3), max_iter=MAX_ITER)
    assert np.isfinite(vals).all() and not calls and not grad_calls


def test_two_planets_run_mcmc_side_by_side(monkeypatch, tmp_path):
    """a two-planet model at N = 45 through mcmc(batch=True) under the tests' emcee stand-in, device_means on, end to end:
    every half-step's walkers are one gprn_elbocalc_batch_means call, and every log-probability is finite"""
    import os
    from scipy import stats
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fake_emcee'))
    monkeypatch.chdir(tmp_path)
    g = _rv_model(45, 2, 1, True, two_planets=True)
    assert [n.split('.')[1] for n in g.parameters_dict if n.startswith('mean1.')] == \
        ['P1', 'K1', 'e1', 'w1', 'Tp1', 'P2', 'K2', 'e2', 'w2', 'Tp2']
    priors = {n: stats.uniform(v - 0.01 * abs(v) - 1e-3, 0.02 * abs(v) + 2e-3) for n, v in g.parameters_dict.items()}
    calls = _count_fused(monkeypatch)
    np.random.seed(3)
    sampler = g.mcmc(priors, niter=2, batch=True)
    assert calls and np.all(np.isfinite(sampler.get_log_prob()))
    assert sampler.get_chain().shape[0] == 2 and sampler.get_chain().shape[2] == len(priors)


# ------------------------------------------------------------------ gprn_elbocalc_batch_means itself
def _staged(g, sets, start):
    g._mu, g._var = np.array(start[0]), np.array(start[1])
    staged = g._batch_stage(sets)
    assert staged is not None and isinstance(staged[2], _hip.MeanParams)
    return staged


def _same_bits(res_m, res_g):
    for a, b in zip(res_m, res_g):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('N,p,q,B,chunked', [(45, 2, 1, 5, False), (200, 2, 2, 3, False), (45, 2, 1, 20, True), (200, 2, 2, 3, True)])
def test_batch_means_against_batch_grad_fed_its_own_resid_out(N, p, q, B, chunked):
    g = _rv_model(N, p, q, True, elbo='bound')
    x0 = np.array(g.get_parameters(), dtype=float)
    _, mu0, var0, _ = g.ELBOcalc(max_iter=MAX_ITER)
    sets = _perturbed(x0, B)
    ctx, kp, yr, jt, m0, v0 = _staged(g, sets, (mu0, var0))
    budgets = [None]
    if chunked:
        budgets = [1] if N == 45 else [4, 8, 12, 16, 24, 32, 48, 64, 96, 128]
    found = False
    for mb in budgets:
        if mb is not None:
            ctx.option('batch_mem_mb', mb)
        res_m = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True, want_grad=True)
        assert res_m is not None and not res_m[3].any()
        chunk = ctx.option('batch_chunk')
        if chunked and N != 45 and chunk != 2:
            continue
        found = True
        assert (1 <= chunk < B) if chunked else chunk == B
        resid, mean_grad = yr.resid.copy(), yr.mean_grad.copy()
        res_g = ctx.elbocalc_batch(kp, resid, jt, m0, v0, MAX_ITER, want_state=True, want_grad=True)
        _same_bits(res_m, res_g)
        assert np.array_equal(resid, yr.host_resid(ctx))            # y - mean: the data minus gprn_eval_mean's bits
        ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True, want_grad=True)
        assert np.array_equal(yr.mean_grad, mean_grad) and np.array_equal(yr.resid, resid)      # a fixed order: the same bits
        break
    assert found, 'no budget gave chunks of 2'


def test_mean_grad_out_against_the_returned_state_and_the_pinned_derivatives():
    sets = [[fx.build(BY_NAME[f'mix_set{s}_out0_nt45']), meanfunc.Constant(0.25 * s),
             fx.build(BY_NAME[f'mix_set{s}_out2_nt45'])] for s in range(3)]
    g = _model(True, sets[0])
    g.elbo = 'bound'
    vecs = []
    for means in sets:
        x = g.get_parameters(include_frozen=True).copy()
        x[8:-3] = np.concatenate([m_.pars for m_ in means])
        vecs.append(x)
    _, mu0, var0, _ = g.ELBOcalc(max_iter=MAX_ITER)
    start = (np.array(mu0), np.array(var0))
    ctx, kp, yr, jt, m0, v0 = _staged(g, vecs, start)
    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 3, want_state=True, want_grad=True, forced=True)
    assert not res[3].any()
    mu_f, got, N = res[4], yr.mean_grad, 45
    resid = yr.resid.reshape(3, 3, N)
    fit = np.einsum('biqn,bqn->bin', mu_f[:, 1:], mu_f[:, 0])
    w = (resid - fit) / (jt[:, :, None] ** 2 + g.yerr2[None])
    worst = 0.0
    for s in range(3):
        col = 0
        for o in (0, 1, 2):
            if o == 1:
                ref, lim = float(np.sum(w[s, 1])), N * 2.0 ** -53 * np.abs(w[s, 1]).sum()
                assert abs(got[s, col] - ref) <= lim
                col += 1
                continue
            hi, lo, kap = fx.reference(BY_NAME[f'mix_set{s}_out{o}_nt45'], D)[1]
            for k in range(hi.shape[0]):
                import math
                ref = math.fsum(hi[k] * w[s, o]) + math.fsum(lo[k] * w[s, o])
                lim = np.sum(np.abs(w[s, o]) * fx.allowed((hi[k], lo[k], kap[k]))) + N * 2.0 ** -53 * np.sum(np.abs(w[s, o] * hi[k]))
                worst = max(worst, abs(got[s, col] - ref) / lim)
                assert abs(got[s, col] - ref) <= lim, (s, o, k, got[s, col], ref, lim)
                col += 1
    print('mean_grad_out: worst deviation %.3f of the allowed one' % worst)
    # nELBO_and_grad_batch hands out these rows
    g.set_parameters(vecs[0].copy())
    vals, grads = g.nELBO_and_grad_batch(vecs, sweeps=3, start=start)
    assert np.array_equal(grads[:, 8:-3], -got)


def test_mean_grad_out_under_a_mask_with_nan_data():
    N, p, q, B = 45, 2, 1, 5
    mask = np.random.RandomState(2).rand(p, N) > 0.2
    g = _rv_model(N, p, q, True, mask=mask, nan_under_mask=True, batch_under_mask=True, elbo='bound')
    g_off = _rv_model(N, p, q, False, mask=mask, batch_under_mask=True, elbo='bound')
    x0 = np.array(g.get_parameters(), dtype=float)
    _, mu0, var0, _ = g_off.ELBOcalc(max_iter=MAX_ITER)
    start = (np.array(mu0), np.array(var0))
    sets = _perturbed(x0, B)
    out = []
    for obj in (g, g_off):
        obj.set_parameters(x0.copy())
        out.append(obj.nELBO_and_grad_batch(sets, sweeps=3, start=start))
    (v_on, g_on), (v_off, g_ref) = out
    assert np.isfinite(v_on).all() and np.isfinite(g_on).all()
    np.testing.assert_allclose(v_on, v_off, rtol=1e-8)
    assert np.all(np.abs(g_on - g_ref).max(axis=1) <= 1e-8 * np.abs(g_ref).max(axis=1))


def test_batch_means_refusals():
    g = _rv_model(45, 2, 1, True)                        # the reference form of the ELBO
    x0 = np.array(g.get_parameters(), dtype=float)
    _, mu0, var0, _ = g.ELBOcalc(max_iter=MAX_ITER)
    sets = _perturbed(x0, 3)
    ctx, kp, yr, jt, m0, v0 = _staged(g, sets, (mu0, var0))
    assert not yr.want_mean_grad
    assert ctx.elbocalc_batch(kp, yr, jt, m0, v0, 3, want_grad=True) is not None and yr.mean_grad is None
    yr.want_mean_grad = True                             # quirk Q3: the reported ELBO does not read the means
    assert ctx.elbocalc_batch(kp, yr, jt, m0, v0, 3, want_grad=True) is None
    short = _hip.MeanParams(yr.params[:, :-1], yr.y_raw)
    with pytest.raises(_hip.BackendError):
        ctx.elbocalc_batch(kp, short, jt, m0, v0, 3)
    # a mean without a program keeps the whole call on the old path

    class Mine(meanfunc.Linear):
        pass
    g.set_components(g.nodes, g.weights, [g.means[0], Mine(0.001, 0.05)], [0.2, 0.2])
    g._mu, g._var = np.array(mu0), np.array(var0)
    staged = g._batch_stage(_perturbed(np.array(g.get_parameters(), dtype=float), 3))
    assert staged is not None and isinstance(staged[2], np.ndarray)
