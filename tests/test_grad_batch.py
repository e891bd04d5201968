"""The side-by-side ELBO gradient (gprn_elbocalc_batch_grad, inference.nELBO_and_grad_batch) without a GPU: the header and
the binding agree on the new entry, the method's argument checks come before anything touches the device, and the vectorised
jitter entries are _grad_from_state's."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gprn_hip.h')


def _prototype(name):
    """The argument list of `name` in the header, comments removed: [(type, argument name)]."""
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


def test_header_declares_the_entry_and_the_flag():
    text = open(HEADER).read()
    assert re.search(r'^#define\s+GPRN_BATCH_FORCED\s+1\s*$', text, flags=re.M)
    assert _hip.GPRN_BATCH_FORCED == 1
    args = _prototype('gprn_elbocalc_batch_grad')
    assert [a[1] for a in args] == ['ctx', 'n_eval', 'kernel_params', 'n_kernel_params', 'y_resid', 'jitters', 'mu', 'var',
                                    'max_iter', 'flags', 'elbo', 'iterations', 'converged', 'info', 'mu_out', 'var_out',
                                    'grad_out']


@pytest.mark.parametrize('name', ['gprn_elbocalc_batch_grad', 'gprn_elbocalc_batch'])
def test_binding_matches_the_prototype(name):
    restype, argtypes = _hip.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert argtypes == [_CTYPES[typ] for typ, _ in _prototype(name)]
    # the older entry is the new one without `flags` and `grad_out`
    new = [a for a in _prototype('gprn_elbocalc_batch_grad') if a[1] not in ('flags', 'grad_out')]
    assert new == _prototype('gprn_elbocalc_batch')


def test_python_keywords():
    sig = inspect.signature(_hip.Context.elbocalc_batch).parameters
    assert sig['want_grad'].default is False and sig['forced'].default is False
    sig = inspect.signature(gpyrn.inference.nELBO_and_grad_batch).parameters
    assert list(sig)[1:] == ['parameter_sets', 'max_iter', 'sweeps', 'start']
    assert all(sig[k].default is None for k in ('max_iter', 'sweeps', 'start'))


def _small_model(p=2, q=2, N=14, seed=0):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(N)) * 30
    args = []
    for _ in range(p):
        args += [rng.randn(N), 0.1 + 0.2 * rng.rand(N)]
    g = gpyrn.inference(q, t, *args)
    nodes = [covfunc.SquaredExponential(1.0, 5.0 + j) for j in range(q)]
    weights = [covfunc.SquaredExponential(0.7, 9.0 + k) for k in range(q * p)]
    g.set_components(nodes, weights, [meanfunc.Constant(0.1 * i) for i in range(p)], [0.3 + 0.1 * i for i in range(p)])
    return g


def test_without_a_gpu_it_raises_what_nelbo_batch_raises():
    if _hip.device_count() > 0:
        pytest.skip('a GPU is present')
    g = _small_model()
    x = np.array(g.get_parameters(), dtype=float)
    with pytest.raises(_hip.BackendUnavailable):
        g.nELBO_batch([x, x * 1.01])
    with pytest.raises(_hip.BackendUnavailable):
        g.nELBO_and_grad_batch([x, x * 1.01])
    with pytest.raises(_hip.BackendUnavailable):
        g.nELBO_and_grad_batch([x, x * 1.01], sweeps=2)


def test_argument_checks_come_first():
    g = _small_model()
    x = np.array(g.get_parameters(), dtype=float)
    with pytest.raises(ValueError, match='Wrong number of parameters'):      # the reference's message (set_parameters)
        g.nELBO_and_grad_batch([x, x[:-1]])
    with pytest.raises(ValueError):
        g.nELBO_and_grad_batch([x], sweeps=0)
    with pytest.raises(ValueError):
        g.nELBO_and_grad_batch([x], max_iter=0)
    with pytest.raises(ValueError):                          # two-dimensional, of the right size
        g.nELBO_and_grad_batch([x, (2.0 * x).reshape(1, -1)])
    with pytest.raises(ValueError, match='start'):           # a start state belongs to the forced sweeps
        g.nELBO_and_grad_batch([x], start=(np.zeros(3), np.ones(3)))
    assert np.array_equal(g.get_parameters(), x)
    vals, grads = g.nELBO_and_grad_batch([])
    assert vals == [] and grads.shape == (0, x.size)
    g._comm = object()                                       # (what a sharded object holds: any communicator)
    with pytest.raises(NotImplementedError):
        g.nELBO_and_grad_batch([x])


@pytest.mark.parametrize('p,q,masked', [(1, 1, False), (2, 2, False), (3, 2, True)])
def test_vectorised_jitter_entries_are_grad_from_state_s(p, q, masked):
    g = _small_model(p, q, N=11, seed=p + q)
    if masked:
        g.mask = np.random.RandomState(5).rand(p, g.N) > 0.2
    rng = np.random.RandomState(3)
    B = 4
    mu = rng.randn(B, p + 1, q, g.N)
    var = 0.05 + rng.rand(B, p + 1, q, g.N)
    jit = 0.2 + rng.rand(B, p)
    got = g._jitter_grads_batch(jit, mu, var)
    assert got.shape == (B, p)
    nodes, weights, means, _ = g._get_components()

    class NoKernels:                                          # (the kernel entries are not under test: zeros from a stand-in)
        def grad_elbo(self, n):
            return np.zeros(n)

    for b in range(B):
        want = g._grad_from_state(nodes, weights, means, list(jit[b]), mu[b], var[b], None, fused=NoKernels())[-p:]
        np.testing.assert_allclose(got[b], want, rtol=1e-13)
