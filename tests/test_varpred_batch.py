"""Prediction from each vector's own posterior at the end of a batch chunk (gprn_elbocalc_batch_predict, Context.
elbocalc_batch_predict, inference.predict_batch(from_sweeps=True)) without a GPU: the header and the binding agree on the new
entry, the method's argument checks come before anything touches the device, the one-by-one fallback behind a stand-in
context, the mixture of posterior_predictive, the binding's shape checks."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gprn_hip.h')


def _prototype(name):
    """The argument list of `name` in the header, comments removed: [(type, argument name)] (tests/test_grad_batch.py's
    approach, re-stated)."""
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, text, flags=re.S)
    assert m, name
    out = []
    for arg in m.group(1).split(','):
        arg = ' '.join(arg.split())
        typ, _, ident = arg.rpartition(' ')
        while ident.startswith('*'):
            typ, ident = typ + '*', ident[1:]
        out.append((typ.replace(' *', '*'), ident))
    return out


_CTYPES = {'gprn_ctx*': ctypes.c_void_p, 'int': ctypes.c_int, 'const double*': ctypes.POINTER(ctypes.c_double),
           'double*': ctypes.POINTER(ctypes.c_double), 'int*': ctypes.POINTER(ctypes.c_int)}


def test_header_declares_the_entry_and_the_binding_matches():
    args = _prototype('gprn_elbocalc_batch_predict')
    assert [a[1] for a in args] == ['ctx', 'n_eval', 'kernel_params', 'n_kernel_params', 'y_resid', 'jitters', 'mu', 'var',
                                    'max_iter', 'flags', 'ns', 'tstar', 'elbo', 'iterations', 'converged', 'info', 'mu_out',
                                    'var_out', 'lat_mean', 'lat_var', 'out_mean', 'out_var']
    restype, argtypes = _hip.SIGNATURES['gprn_elbocalc_batch_predict']
    assert restype is ctypes.c_int
    assert argtypes == [_CTYPES[typ] for typ, _ in args]
    # the entry it extends is this one without the prediction's arguments, with grad_out at its end
    grad = _prototype('gprn_elbocalc_batch_grad')
    assert [a for a in args if a[1] not in ('ns', 'tstar', 'lat_mean', 'lat_var', 'out_mean', 'out_var')] == grad[:-1]
    # the header cites the reference code the entry stands for
    text = open(HEADER).read()
    comment = text[:text.index('int gprn_elbocalc_batch_predict(')].rsplit('/*', 1)[1]
    assert '_Prediction' in comment and 'meanfield.py:1289-1381' in comment


def test_python_keywords():
    sig = inspect.signature(_hip.Context.elbocalc_batch_predict).parameters
    assert list(sig)[1:] == ['kernel_params', 'y_resid', 'jitters', 'mu', 'var', 'max_iter', 'tstar', 'forced', 'latent',
                             'outputs']
    assert sig['forced'].default is False and sig['latent'].default is True and sig['outputs'].default is True
    sig = inspect.signature(gpyrn.inference.predict_batch).parameters
    assert list(sig)[1:] == ['parameter_sets', 'tstar', 'states', 'max_iter', 'separate', 'from_sweeps', 'sweeps', 'start']
    assert sig['from_sweeps'].default is False and sig['separate'].default is False
    assert all(sig[k].default is None for k in ('tstar', 'states', 'max_iter', 'sweeps', 'start'))
    assert 'from_sweeps' not in inspect.signature(gpyrn.inference.posterior_predictive).parameters   # (it forwards **kw)


def _object(p=2, q=2, N=20, **kw):
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0, 50, N))
    args = []
    for _ in range(p):
        args += [np.sin(t / 6) + 0.1 * rng.standard_normal(N), np.full(N, 0.2)]
    g = gpyrn.inference(q, t, *args, **kw)
    nodes = [covfunc.SquaredExponential(1.0 + 0.1 * j, 10.0) for j in range(q)]
    weights = [covfunc.SquaredExponential(0.8 + 0.05 * k, 20.0) for k in range(q * p)]
    g.set_components(nodes, weights, [meanfunc.Constant(0.1 * i) for i in range(p)], [0.3] * p)
    return g


def test_argument_checks_come_before_the_device():
    g = _object()                                             # the reference form
    x = np.array(g.get_parameters(), dtype=float)
    state = (np.zeros((g.p + 1, g.q, g.N)), np.ones((g.p + 1, g.q, g.N)))
    with pytest.raises(ValueError, match="predict='variational'"):
        g.predict_batch([x, x], from_sweeps=True)
    with pytest.raises(ValueError, match='from_sweeps'):      # the forced sweeps belong to the new form
        g.predict_batch([x, x], sweeps=2)
    assert g._ctx is None
    g = _object(predict='variational')
    with pytest.raises(ValueError, match='states'):           # a state carries no X
        g.predict_batch([x, x], states=(np.zeros((2, 3)), np.ones((2, 3))), from_sweeps=True)
    with pytest.raises(ValueError, match='start'):            # a start state belongs to the forced sweeps
        g.predict_batch([x, x], from_sweeps=True, start=state)
    with pytest.raises(ValueError):
        g.predict_batch([x, x], from_sweeps=True, sweeps=0, start=state)
    with pytest.raises(ValueError):
        g.predict_batch([x, x], from_sweeps=True, max_iter=0)
    with pytest.raises(ValueError):
        g.predict_batch([], from_sweeps=True)
    with pytest.raises(ValueError):
        g.posterior_predictive([x, x], from_sweeps=True, states=state)
    # without the keyword: the refusal tests/test_varpred.py pins, which now names the keyword
    for call in (g.predict_batch, g.posterior_predictive):
        with pytest.raises(NotImplementedError, match='end of a batch chunk') as exc:
            call([x, x])
        assert 'from_sweeps=True' in str(exc.value)
    assert np.array_equal(g.get_parameters(), x)
    assert g._ctx is None
    g._comm = object()                                        # (what a sharded object holds: any communicator)
    with pytest.raises(NotImplementedError, match='sharded'):
        g.predict_batch([x, x], from_sweeps=True)
    with pytest.raises(NotImplementedError, match='sharded'):
        g.posterior_predictive([x, x], from_sweeps=True, sweeps=2)
    assert g._ctx is None


class _OneByOneContext:
    """Stands in for _hip.Context on the one-by-one branch: counts the calls, and predict returns rows that depend on the
    kernels, the jitters, the state the loop left and the times, so that a wrong pairing shows."""
    rank = 0

    def __init__(self, g):
        self.G, self.shape = g.q * (g.p + 1), (g.p + 1, g.q, g.N)
        self.kernels, self.calls = {}, []
        self.form = None

    def option(self, name, value=-1):
        if name == 'predict_form' and value >= 0:
            self.form = value
        return 0

    def set_sweep_order(self, *a):
        pass

    def set_kernel(self, gp, ops, params, add_nugget):
        self.kernels[gp] = np.array(params, dtype=float)

    def factor_priors(self):
        self.calls.append('factor_priors')
        return 0

    def set_y_resid(self, y):
        self.y = np.array(y, dtype=float)

    def set_jitters(self, j):
        self.jit = np.array(j, dtype=float)

    def set_muvar(self, mu, var):
        self.mu, self.var = np.array(mu, dtype=float), np.array(var, dtype=float)

    def _left(self, trips):
        self.mu = self.mu + 0.01 * trips * self.jit.sum() + self.y.mean()
        self.var = self.var * (1.0 + 0.1 * trips)

    def sweep(self, n, commit=False):
        assert commit
        self.calls.append(('sweep', n))
        self._left(n)
        return np.zeros(n), np.zeros((n, 3)), 0

    def get_muvar(self):
        return self.mu.reshape(self.shape), self.var.reshape(self.shape)

    def elbocalc(self, max_iter, **kw):
        self.calls.append(('elbocalc', max_iter))
        self._left(5)
        return np.zeros(6), 5, True, 0, self.mu.reshape(self.shape), self.var.reshape(self.shape)

    def elbocalc_batch_predict(self, *a, **kw):
        self.calls.append('batch')
        return None

    def predict(self, tstar):
        assert self.form == _hip.PREDICT_POSTERIOR
        self.calls.append('predict')
        ts = np.asarray(tstar, dtype=float)
        amp = np.array([self.kernels[g][0] for g in range(self.G)])
        mean = amp[:, None] * np.sin(ts[None, :] / 7.0 + np.arange(self.G)[:, None]) + self.mu.mean()
        var = 0.1 + amp[:, None] ** 2 * np.cos(ts[None, :] / 5.0) ** 2 + self.var.mean()
        return mean, var, 0


def _expected(g, fake, x, tstar, start, trips, forced):
    """What the one-by-one branch must return for vector x: the stand-in's rows, combined with the jitter once."""
    g.set_parameters(x)
    nodes, weights, means, jitters = g._get_components()
    ctx = g._setup_device(nodes, weights, means, jitters)
    ctx.option('predict_form', _hip.PREDICT_POSTERIOR)
    ctx.set_muvar(*start)
    if forced:
        ctx.sweep(trips, commit=True)
    else:
        ctx.elbocalc(trips)
    gm, gv, _ = ctx.predict(tstar)
    return g._combine_prediction(gm, gv, means, jitters, tstar, True, once=True)


@pytest.mark.parametrize('forced', [True, False])
def test_one_by_one_fallback_under_a_stand_in_context(forced):
    B = 3
    g = _object(predict='variational')
    g.batch_max_N = 0                                         # (N above batch_max_N: the side-by-side form does not apply)
    g._ctx = fake = _OneByOneContext(g)
    g._predict_sent = 'reference'
    rng = np.random.default_rng(0)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * rng.uniform(0.9, 1.1, x0.size) for _ in range(B)]
    tstar = np.linspace(-5, 60, 17)
    shape = (g.p + 1, g.q, g.N)
    start = (rng.standard_normal(shape), rng.uniform(0.5, 1.5, shape))
    if forced:
        kw = dict(sweeps=2, start=start)
    else:
        g._mu, g._var = start
        kw = dict(max_iter=30)
    mean, var, lat = g.predict_batch(sets, tstar=tstar, from_sweeps=True, separate=True, **kw)
    loops = [c for c in fake.calls if isinstance(c, tuple)]
    assert loops == [('sweep', 2) if forced else ('elbocalc', 30)] * B
    assert fake.calls.count('predict') == B and 'batch' not in fake.calls
    assert mean.shape == (B, tstar.size, g.p) and var.shape == mean.shape and lat.shape == (B, g.q * (g.p + 1), tstar.size)
    np.testing.assert_array_equal(g.get_parameters(), sets[-1])
    if not forced:
        assert g._mu is not start[0]                          # (the last converged loop's state is kept)
    for b in range(B):
        m1, v1, parts = _expected(g, fake, sets[b], tstar, start, 2 if forced else 30, forced)
        assert np.array_equal(mean[b], m1) and np.array_equal(var[b], v1)
        assert np.array_equal(lat[b], np.concatenate([np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)]))
    assert not np.array_equal(mean[0], mean[1])
    two = g.predict_batch(sets, tstar=tstar, from_sweeps=True, **({'sweeps': 2, 'start': start} if forced else
                                                                 {'max_iter': 30}))
    assert len(two) == 2 and two[0].shape == mean.shape
    if forced:
        assert np.array_equal(two[0], mean) and np.array_equal(two[1], var)


def test_posterior_predictive_forwards_from_sweeps_and_mixes():
    B, ns, p = 4, 9, 2
    rng = np.random.default_rng(1)
    mean_b, var_b = rng.standard_normal((B, ns, p)), rng.uniform(0.1, 2.0, (B, ns, p))
    g = _object(p=p, predict='variational')
    seen = {}

    def stand_in(self, parameter_sets, tstar=None, **kw):
        seen.update(kw, tstar=tstar)
        return mean_b, var_b
    g.predict_batch = types.MethodType(stand_in, g)
    ts = np.linspace(0, 1, ns)
    w = np.array([3.0, 1.0, 0.5, 2.0])
    mean, var = g.posterior_predictive(list(range(B)), tstar=ts, weights=w, from_sweeps=True, sweeps=3, start='s')
    assert seen == dict(from_sweeps=True, sweeps=3, start='s', tstar=ts)
    wn = w / w.sum()
    ref_mean = sum(wn[b] * mean_b[b] for b in range(B))
    ref_second = sum(wn[b] * (var_b[b] + mean_b[b] ** 2) for b in range(B))
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(var, ref_second - ref_mean ** 2, rtol=1e-12, atol=1e-14)
    assert g._ctx is None


def test_binding_shape_checks_come_before_the_library():
    """An object with the problem's sizes and no handle stands in (tests/test_predict_batch.py's way)."""
    ctx = types.SimpleNamespace(p=2, q=1, N=10, G=3, _lib=None, _h=None)
    call = lambda *a, **kw: _hip.Context.elbocalc_batch_predict(ctx, *a, **kw)
    B, d, n_k = 4, 3 * 10, 6
    kp, yr, jt = np.ones((B, n_k)), np.zeros((B, 2, 10)), np.ones((B, 2))
    mu, var, ts = np.zeros((B, d)), np.ones((B, d)), np.linspace(0, 1, 5)
    with pytest.raises(ValueError, match='latent pair, the output pair or both'):
        call(kp, yr, jt, mu, var, 3, ts, latent=False, outputs=False)
    with pytest.raises(ValueError, match='kernel_params'):
        call(np.ones(n_k), yr, jt, mu, var, 3, ts)
    with pytest.raises(ValueError, match='y_resid'):
        call(kp, yr[:, :1], jt, mu, var, 3, ts)
    with pytest.raises(ValueError, match='jitters'):
        call(kp, yr, jt[:, :1], mu, var, 3, ts)
    with pytest.raises(ValueError, match='mu and var'):
        call(kp, yr, jt, mu[:, :-1], var, 3, ts)
    with pytest.raises(ValueError, match='tstar is empty'):
        call(kp, yr, jt, mu, var, 3, np.zeros(0))
    with pytest.raises(ValueError, match='committed sweep'):
        call(kp, yr, jt, mu, var, 0, ts)
