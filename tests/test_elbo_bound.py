"""The bound form of the ELBO (inference(..., elbo='bound'), option "elbo_form") without a GPU: the two routes of its
restatement tests/_bound_ref.py against each other, its anchor to the reference's fixtures at q = 1 (where quirks Q1 and Q2
are vacuous), that it rises on every sweep of the sequential order, that its fixed-state gradient is the total gradient at
convergence (which the reference form's is not), and the host side of the public interface."""
import inspect
import os
import re

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _bound_ref as BR, _cases, _mask_ref as MR, _order_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mask_of(pr, seed):
    p, N = pr['y_raw'].shape
    return None if seed is None else MR.partial_mask(p, N, seed=seed)


def _start(pr, mask):
    """_initMuVar -- under a mask on the zero-filled y, as inference does."""
    if mask is None:
        return pr['mu0'], pr['var0']
    return MR.init_state(pr, mask)


# ------------------------------------------------------------------ 1. the two routes
@pytest.mark.parametrize('order', BR.ORDERS)
@pytest.mark.parametrize('tag,seed', [('step_p3q2', None), ('step_p2q3', None), ('step_p2q3', 3)])
def test_the_two_routes_agree(tag, seed, order):
    """Explicit covariances (cho_solve traces, Cholesky entropies) against the B-form over three forced sweeps: 1e-9 relative
    on the ELBO and its parts."""
    pr = BR.problem(tag)
    mask = _mask_of(pr, seed)
    mu0, var0 = _start(pr, mask)
    Eb, Pb, mu_b, var_b = BR.sweeps(*pr['args'], mu0, var0, 3, mask=mask, order=order, route='B')
    Ed, Pd, mu_d, var_d = BR.sweeps(*pr['args'], mu0, var0, 3, mask=mask, order=order, route='dense')
    print(tag, seed, order, 'ELBO rel %.2e, parts rel %.2e' % (np.abs(Eb / Ed - 1).max(), np.abs(Pb / Pd - 1).max()))
    np.testing.assert_allclose(Eb, Ed, rtol=1e-9)
    np.testing.assert_allclose(Pb, Pd, rtol=1e-9)
    _cases.assert_state('bound restatement, routes %s %s %s' % (tag, seed, order), mu_b, mu_d, var_b, var_d)


def test_the_bound_is_the_sum_of_its_parts_and_is_not_divided_by_q():
    pr = BR.problem('step_p2q3')
    E, _, _, parts = BR.sweep(*pr['args'], pr['mu0'], pr['var0'])
    assert E == parts[0] + parts[1] + parts[2]


# ------------------------------------------------------------------ 2. the anchor at q = 1
@pytest.mark.parametrize('tag', ['step_p1q1', 'step_p2q1', 'cfg1_N200'])
def test_with_one_node_prior_term_entropy_and_states_are_the_reference_s(tag):
    """At q = 1 there is no cumulative covariance (Q1) and the raw reshape is the identity (Q2): LogP and Ent of every
    recorded sweep are the fixture's, and so are the states.  cfg1_N200 has zero mean functions, so Q3 is vacuous too (and
    Q5 divides by 1): LogL and the ELBO as well."""
    pr = BR.problem(tag)
    d = pr['d']
    assert pr['meta']['q'] == 1
    n = len(d['elbo_sweeps'])
    E, P, mu, var = BR.sweeps(*pr['args'], d['mu_init'], d['var_init'], n)
    want = np.array(d['parts_sweeps'])
    np.testing.assert_allclose(P[:, 1], want[:, 1], rtol=1e-8)
    np.testing.assert_allclose(P[:, 2], want[:, 2], rtol=1e-8)
    _cases.assert_state('bound restatement at q = 1 ' + tag, mu, d['mu_final'], var, d['var_final'])
    if tag == 'cfg1_N200':
        assert all(m is None or not np.any(m(pr['time'])) for m in pr['means'])
        np.testing.assert_allclose(P[:, 0], want[:, 0], rtol=1e-8)
        np.testing.assert_allclose(E, d['elbo_sweeps'], rtol=1e-8)
    else:
        assert not np.allclose(P[:, 0], want[:, 0], rtol=1e-3)      # (non-zero means: the reference reads the raw y there)


# ------------------------------------------------------------------ 3. monotone
@pytest.mark.parametrize('tag,seed', [('mid_N300_p3q2', None), ('step_p2q3', 3), ('step_p2q3', None), ('step_p3q2', None)])
def test_the_bound_rises_on_every_sequential_sweep(tag, seed):
    """25 sweeps of the sequential order (a coordinate ascent on this very function) from _initMuVar.  The reference form's
    value is not monotone on the same sweeps at q = 3."""
    pr = BR.problem(tag)
    mask = _mask_of(pr, seed)
    mu0, var0 = _start(pr, mask)
    E, _, _, _ = BR.sweeps(*pr['args'], mu0, var0, 25, mask=mask, order='sequential')
    steps = np.diff(E)
    print(tag, seed, 'bound %.6f -> %.6f, smallest step %+.3e' % (E[0], E[-1], steps.min()))
    assert np.all(np.isfinite(E))
    assert np.all(steps >= -1e-10 * np.abs(E[1:]))


# ------------------------------------------------------------------ 4. the envelope theorem
def _free_parameters(pr):
    """(owner, index) of every parameter in inference.grad_ELBO's order: nodes, weights, means, jitters."""
    out = []
    for o in list(pr['nodes']) + list(pr['weights']) + [m for m in pr['means'] if m is not None]:
        out += [(o.pars, i) for i in range(o.pars.size)]
    return out + [(pr['jitters'], i) for i in range(len(pr['jitters']))]


@pytest.fixture(scope='module')
def converged():
    """step_p3q2 after 3000 sweeps of the sequential order: the problem, the state, the state one sweep before."""
    pr = BR.problem('step_p3q2')
    pr['jitters'] = list(pr['jitters'])
    mu, var = pr['mu0'], pr['var0']
    for _ in range(3000):
        mu_p, var_p = mu, var
        E, mu, var, _ = BR.sweep(*pr['args'], mu, var, order='sequential')
    return dict(pr=pr, E=E, mu=mu, var=var, mu_p=mu_p, var_p=var_p)


WARM = 40     # sweeps that re-converge a vector moved by 1e-5 from the converged state (the bound is back to rounding after ~20)


def _central_differences(c, value):
    """d value / d theta for every parameter, theta +- 1e-5 max(1, |theta|), `value()` re-converged at each."""
    fd = []
    for pars, i in _free_parameters(c['pr']):
        v = pars[i]
        h = 1e-5 * max(1.0, abs(v))
        pars[i] = v + h; up = value()
        pars[i] = v - h; dn = value()
        pars[i] = v
        fd.append((up - dn) / (2 * h))
    return np.array(fd)


def test_at_convergence_the_fixed_state_gradient_is_the_total_gradient(converged):
    """Every parameter class -- all four parameters of both QuasiPeriodic nodes, the SE weights, the Constant / Linear /
    Sine means, the jitters: the analytic fixed-state gradient against central differences of the RE-CONVERGED bound."""
    c = converged
    pr = c['pr']
    np.testing.assert_allclose(c['E'], -158.031077117, rtol=1e-10)
    grad, _ = BR.gradient(pr, pr['args'], c['mu_p'], c['var_p'], c['mu'], c['var'])

    def value():
        args = BR.setup_args(pr)
        return BR.sweeps(*args, c['mu'], c['var'], WARM, order='sequential')[0][-1]
    fd = _central_differences(c, value)
    assert grad.shape == fd.shape
    off = np.abs(grad - fd).max() / np.abs(fd).max()
    print('envelope: analytic vs re-converged differences, %.2e of the largest entry (%d parameters)' % (off, fd.size))
    assert off <= 1e-6
    # ... the mean-function entries among them are not zero: the bound sees the mean functions
    n_m = sum(m.pars.size for m in pr['means'] if m is not None)
    assert np.all(np.abs(grad[-3 - n_m:-3]) > 1e-3)


def test_the_reference_form_s_fixed_state_gradient_is_not(converged):
    """What the switch buys: the same inequality for the reference form's value and its fixed-state jitter entries (closed
    form with the raw y, divided by q) fails by orders of magnitude -- the state the updates converge to is not stationary
    for that function."""
    c = converged
    pr = c['pr']
    q, (p, N) = pr['meta']['q'], pr['y_raw'].shape

    def value():
        Kf, Kw, Lf, Lw, yres, yerr2, jitt2 = BR.setup_args(pr)
        return OR.sweeps(Kf, Kw, Lf, Lw, yres, pr['y_raw'], yerr2, jitt2, c['mu'], c['var'], WARM, order='sequential')[0][-1]
    fd = []
    jit = pr['jitters']
    for i in range(p):
        v = jit[i]
        h = 1e-5 * max(1.0, abs(v))
        jit[i] = v + h; up = value()
        jit[i] = v - h; dn = value()
        jit[i] = v
        fd.append((up - dn) / (2 * h))
    fd = np.array(fd)
    mu, var = c['mu'], c['var']
    variance = np.asarray(jit, dtype=float)[:, None] ** 2 + pr['yerr2']
    fit = np.einsum('iqn,qn->in', mu[1:], mu[0])
    A = sum(var[0, j] * mu[1:, j] ** 2 + var[1:, j] * mu[0, j] ** 2 + var[0, j] * var[1:, j] for j in range(q))
    dv = -0.5 * (1.0 / variance - ((pr['y_raw'] - fit) ** 2 + A) / variance ** 2)
    grad = np.sum(dv, axis=1) * 2 * np.asarray(jit, dtype=float) / q
    off = np.abs(grad - fd).max() / np.abs(fd).max()
    print('reference form: fixed-state jitter entries', grad, 'total', fd, 'off by %.2e of the largest' % off)
    assert off > 1e-3


# ------------------------------------------------------------------ 5. the host side of the interface
def _data(p=2, N=12, seed=0):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(N)) * 10
    return t, [a for i in range(p) for a in (rng.randn(N), rng.rand(N) + 0.1)]


def test_validation_raises_before_any_device_call():
    t, args = _data()
    for bad in ('Bound', 'exact', '', None, 1, True):
        with pytest.raises(ValueError):
            gpyrn.inference(2, t, *args, elbo=bad)
    g = gpyrn.inference(2, t, *args)
    assert g.elbo == 'reference' and g._ctx is None
    g.elbo = 'bound'
    assert g.elbo == 'bound' and g._ctx is None
    with pytest.raises(ValueError):
        g.elbo = 'tight'
    assert g.elbo == 'bound'
    assert gpyrn.inference(2, t, *args, elbo='bound').elbo == 'bound'
    assert inspect.signature(gpyrn.inference.__init__).parameters['elbo'].default == 'reference'
    # through from_series too
    series = [(t, args[0], args[1]), (t[::2], args[2][::2], args[3][::2])]
    assert gpyrn.inference.from_series(1, series, elbo='bound').elbo == 'bound'
    with pytest.raises(ValueError):
        gpyrn.inference.from_series(1, series, elbo='no')


def test_a_sharded_object_refuses_the_bound_form():
    t, args = _data()
    with pytest.raises(NotImplementedError):
        gpyrn.inference(2, t, *args, elbo='bound', comm=object())
    g = gpyrn.inference(2, t, *args, comm=object())
    with pytest.raises(NotImplementedError):
        g.elbo = 'bound'
    assert g.elbo == 'reference'


class _RecordingContext:
    """Stands in for _hip.Context through a set-up: holds the options it is given, as the library does."""
    rank = 0

    def __init__(self):
        self.options, self.values, self.factored = [], {}, 0

    def option(self, name, value=-1):
        old = self.values.get(name, 0)
        self.options.append((name, value))
        if value >= 0:
            self.values[name] = value
        return old

    def owner_of(self, gp):
        return 0

    def set_kernel(self, gp, ops, params, add_nugget):
        pass

    def upload_K(self, gp, K):
        pass

    def factor_priors(self):
        self.factored += 1
        return 0

    def set_y_resid(self, y):
        pass

    def set_jitters(self, j):
        pass


def _object(**kw):
    t, args = _data(p=2, N=12)
    g = gpyrn.inference(1, t, *args, **kw)
    g.set_components([covfunc.SquaredExponential(1.0, 3.0)], [covfunc.SquaredExponential(0.8, 5.0)] * 2,
                     [meanfunc.Constant(0.1), meanfunc.Linear(0.02, -0.1)], [0.3, 0.4])
    return g


def test_the_form_reaches_the_context_with_every_set_up_and_a_change_drops_the_cached_one():
    g = _object(elbo='bound')
    g._ctx = fake = _RecordingContext()
    g._setup_device(*g._get_components())
    assert [v for n, v in fake.options if n == 'elbo_form'] == [_hip.ELBO_BOUND] and fake.factored == 1
    g._setup_device(*g._get_components())                  # unchanged kernels: no new factors, the option all the same
    assert [v for n, v in fake.options if n == 'elbo_form'] == [_hip.ELBO_BOUND] * 2 and fake.factored == 1
    g._mu, g._var = np.zeros(3), np.ones(3)
    g.elbo = 'bound'                                       # (no change: everything stays)
    assert g._prior_key is not None and g._mu is not None
    g.elbo = 'reference'
    assert g._prior_key is None and g._mu is None and g._var is None
    assert fake.values['elbo_form'] == _hip.ELBO_REFERENCE
    g._setup_device(*g._get_components())
    assert fake.factored == 2
    # the default object sends the reference form, and nothing else changes for it
    g = _object()
    g._ctx = fake = _RecordingContext()
    g._setup_device(*g._get_components())
    assert [v for n, v in fake.options if n == 'elbo_form'] == [_hip.ELBO_REFERENCE]


def test_the_header_and_the_binding_carry_the_two_constants():
    text = open(os.path.join(ROOT, 'include', 'gprn_hip.h')).read()
    assert re.search(r'#define\s+GPRN_ELBO_REFERENCE\s+0\b', text) and re.search(r'#define\s+GPRN_ELBO_BOUND\s+1\b', text)
    assert '"elbo_form"' in text[text.index('int gprn_set_option') - 4000:text.index('int gprn_set_option')]
    assert (_hip.ELBO_REFERENCE, _hip.ELBO_BOUND) == (0, 1)
    # no new exported symbol
    assert not [n for n in _hip.SIGNATURES if 'elbo_form' in n or 'bound' in n]


def test_fused_is_the_only_gradient_form_and_its_keyword_keeps_its_default():
    for f in (gpyrn.inference.grad_ELBO, gpyrn.inference.nELBO_and_grad):
        assert inspect.signature(f).parameters['fused'].default is False
    g = _object(elbo='bound')
    with pytest.raises(ValueError):                         # (as in the reference form: fused= needs jac=True)
        g.optimize(fused=True)


class _Tanh(meanfunc.meanFunction):
    """A user-defined mean function without a closed form of its own: the base class differences it."""
    _param_names = ('a', 'tau')
    _parsize = 2

    def __call__(self, t):
        return self.pars[0] * np.tanh(np.asarray(t, dtype=float) / self.pars[1])


MEANS = [lambda t: _Tanh(1.5, 8.0), lambda t: _Tanh(0.7, 3.0) + meanfunc.Constant(0.2), lambda t: meanfunc.Constant(1.3), lambda t: meanfunc.Linear(0.2, 1.0), lambda t: meanfunc.Parabola(0.01, -0.2, 3.0),
         lambda t: meanfunc.Cubic(1e-3, 0.01, -0.2, 3.0), lambda t: meanfunc.Sine(2.0, 7.0, 0.3),
         lambda t: meanfunc.MultiConstant([0.5, -0.3, 2.0], np.r_[np.ones(5), 2 * np.ones(6), 3 * np.ones(4)], t),
         lambda t: meanfunc.Constant(1.0) + meanfunc.Sine(2.0, 7.0, 0.3),
         lambda t: meanfunc.Linear(0.2, 1.0) * meanfunc.Sine(2.0, 7.0, 0.3),
         lambda t: (meanfunc.Constant(0.5) + meanfunc.Linear(0.1, 0.2)) * meanfunc.Parabola(0.01, 0.0, 1.0)]


@pytest.mark.parametrize('make', MEANS, ids=lambda f: repr(f(np.arange(15.0))))
def test_mean_function_derivatives_against_differences(make):
    t = np.sort(np.random.RandomState(0).rand(15)) * 30
    m = make(t)
    D = m._dm_dpars(t)
    pars = np.array(m.pars, dtype=float)
    assert D.shape == (pars.size, t.size) and pars.size == m._parsize
    fd = []
    for k in range(pars.size):
        h = 1e-6 * max(1.0, abs(pars[k]))
        x = pars.copy()
        x[k] = pars[k] + h; m.set_parameters(x); up = m(t)
        x[k] = pars[k] - h; m.set_parameters(x); dn = m(t)
        fd.append((up - dn) / (2 * h))
    m.set_parameters(pars)
    np.testing.assert_array_equal(m.pars, pars)             # (the differences of the base class leave the object as it was)
    fd = np.array(fd)
    assert np.abs(D - fd).max() <= 1e-7 * np.abs(fd).max()


@pytest.mark.parametrize('tag,seed', [('step_p3q2', None), ('step_p2q3', None), ('step_p3q2', 2)])
def test_grad_from_state_pairs_every_latent_gp_with_its_own_mean(tag, seed):
    """inference._grad_from_state(bound=True) with NumPy in place of the device (K^-1 and K^-1 Sigma_g K^-1 of the latent
    GP's OWN covariance, as tests/test_oracle.py does for the reference form) against the restatement's fixed-state
    gradient: kernel entries, mean-function entries, jitter entries.  The explicit inverse of K (cond ~ 1e8) limits the
    kernel entries exactly as in tests/test_oracle.py::test_gradient_formula_against_finite_differences, whose tolerance
    this is; the other entries involve no inverse: 1e-9."""
    pr = BR.problem(tag)
    meta, d = pr['meta'], pr['d']
    mask = _mask_of(pr, seed)
    kw = {} if mask is None else {'mask': mask}
    g = gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d), elbo='bound', **kw)
    g.set_components(pr['nodes'], pr['weights'], pr['means'], pr['jitters'])
    mu_p, var_p = _start(pr, mask)
    _, mu, var, _ = BR.sweep(*pr['args'], mu_p, var_p, mask=mask)
    want, _ = BR.gradient(pr, pr['args'], mu_p, var_p, mu, var, mask=mask)
    Kf, Kw = pr['args'][0], pr['args'][1]
    q, p = meta['q'], meta['p']
    d_f, d_w = BR.precisions(pr['args'], mu_p, var_p, mu, var, mask)

    def matrices(gp):
        K, dd = (Kf[gp], d_f[gp]) if gp < q else (Kw[gp - q], d_w[divmod(gp - q, p)])
        Kinv = np.linalg.inv(K)
        return Kinv, Kinv @ MR._gp(K, dd, np.zeros(K.shape[0]))[0] @ Kinv
    got = np.array(g._grad_from_state(g.nodes, g.weights, g.means, list(g.jitters), mu, var, matrices, bound=True))
    assert got.shape == want.shape
    n_k = sum(k.pars.size for k in list(g.nodes) + list(g.weights))
    scale = np.abs(want[:n_k]).max()
    print(tag, seed, 'kernel entries off by %.2e of the largest, the others by %.2e'
          % (np.abs(got[:n_k] - want[:n_k]).max() / scale, np.abs(got[n_k:] / want[n_k:] - 1).max()))
    np.testing.assert_allclose(got[:n_k], want[:n_k], rtol=2e-5, atol=1e-6 * scale)
    np.testing.assert_allclose(got[n_k:], want[n_k:], rtol=1e-9)
    # the reference form's pairing and scaling are another function's: they do not pass for it
    ref = np.array(g._grad_from_state(g.nodes, g.weights, g.means, list(g.jitters), mu, var, matrices))
    assert not np.allclose(ref[:n_k], want[:n_k], rtol=2e-5, atol=1e-6 * scale)


def test_the_vectorised_entries_are_grad_from_state_s():
    """nELBO_and_grad_batch's jitter and mean-function entries, per vector with its own residual."""
    g = _object(elbo='bound')
    rng = np.random.RandomState(3)
    B, p, q, N = 3, g.p, g.q, g.N
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * (1.0 + 0.1 * rng.standard_normal(x0.size)) for _ in range(B)]
    mu, var = rng.randn(B, p + 1, q, N), 0.05 + rng.rand(B, p + 1, q, N)

    class NoKernels:                                        # (the kernel entries are not under test)
        def grad_elbo(self, n):
            return np.zeros(n)

    want, resid, jit = [], [], []
    for b, x in enumerate(sets):
        g.set_parameters(x)
        nodes, weights, means, jitters = g._get_components()
        resid.append(g.y - g._mean(means).reshape(p, N))
        jit.append(np.array(jitters, dtype=float))
        want.append(g._grad_from_state(nodes, weights, means, list(jitters), mu[b], var[b], None, fused=NoKernels(), bound=True))
    want = np.array(want)
    n_m = 3
    got_j = g._jitter_grads_batch(np.array(jit), mu, var, resid=np.array(resid))
    got_m = g._mean_grads_batch(sets, np.array(jit), mu, np.array(resid))
    np.testing.assert_allclose(got_j, want[:, -p:], rtol=1e-13)
    np.testing.assert_allclose(got_m, want[:, -p - n_m:-p], rtol=1e-12)
    assert np.all(want[:, -p - n_m:-p] != 0.0)
