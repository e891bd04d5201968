"""The sequential sweep order without a GPU: the restatement (tests/_order_ref.py) against the oracle and the reference's
fixtures, what the two orders share bit for bit, the divergence at q = 3 and its end, validation before any device call
and the C ABI's new entry point."""
import os
import re

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip
from oracle import cpu_ref
from tests import _cases, _order_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


@pytest.mark.parametrize('tag', ['step_p3q2', 'step_p2q3'])
def test_reference_order_is_the_oracles_sweep(tag):
    pr = R.problem(tag)
    d, meta = pr['d'], pr['meta']
    mu, var = pr['mu0'], pr['var0']
    assert np.array_equal(mu, d['mu_init']) and np.array_equal(var, d['var_init'])
    E = []
    for _ in range(meta['nsweeps']):
        e_o, mu_o, var_o, parts_o = cpu_ref.sweep_B(*pr['args'], mu, var)
        e, mu, var, parts = R.sweep(*pr['args'], mu, var, order='reference')
        np.testing.assert_allclose(e, e_o, rtol=1e-12)
        np.testing.assert_allclose(parts, parts_o, rtol=1e-12)
        np.testing.assert_allclose(mu, mu_o, rtol=1e-12, atol=0)
        np.testing.assert_allclose(var, var_o, rtol=1e-12, atol=0)
        E.append(e)
    np.testing.assert_allclose(E, d['elbo_sweeps'], rtol=RTOL)


@pytest.mark.parametrize('tag', ['step_p1q1', 'step_p2q1', 'cfg1_N200'])
def test_with_one_node_the_two_orders_are_the_same_computation(tag):
    pr = R.problem(tag)
    assert pr['meta']['q'] == 1
    a = R.sweeps(*pr['args'], pr['mu0'], pr['var0'], 2, order='reference')
    b = R.sweeps(*pr['args'], pr['mu0'], pr['var0'], 2, order='sequential')
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('tag', ['step_p3q2', 'step_p2q3'])
def test_what_the_first_sweep_shares_between_the_orders(tag):
    """d reads none of the means the order is about: all node variances, mu_f0 and the variances of node 0's weights are the
    reference order's bit for bit; mu_f1 is not."""
    pr = R.problem(tag)
    _, mu_r, var_r, _ = R.sweep(*pr['args'], pr['mu0'], pr['var0'], order='reference')
    _, mu_s, var_s, _ = R.sweep(*pr['args'], pr['mu0'], pr['var0'], order='sequential')
    assert np.array_equal(var_s[0], var_r[0])                  # every node variance
    assert np.array_equal(mu_s[0, 0], mu_r[0, 0])              # mu_f0
    assert np.array_equal(var_s[1:, 0], var_r[1:, 0])          # variances of node 0's weights
    assert not np.array_equal(mu_s[0, 1], mu_r[0, 1])          # mu_f1 has seen the new mu_f0
    assert not np.allclose(mu_s[0, 1], mu_r[0, 1], rtol=1e-6, atol=0)


def test_at_three_nodes_the_reference_order_diverges_and_the_sequential_one_stops():
    pr = R.problem('step_p2q3')
    E, _, _, _ = R.sweeps(*pr['args'], pr['mu0'], pr['var0'], 10, order='reference')
    assert np.all(np.abs(E[1:]) > np.abs(E[:-1])), E
    e, mu, var, it, hist, crit = R.elbo_calc(*pr['args'], pr['mu0'], pr['var0'], max_iter=200, order='sequential')
    print('step_p2q3, sequential: trips', it, 'ELBO', hist[1], '->', e)
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(mu)) and np.all(var > 0)
    assert 3 < it < 200 and crit[-1] < 1e-3                    # the rule fired
    assert e > hist[1]


def test_reference_order_of_the_restatement_follows_the_fixtures_loop():
    pr = R.problem('step_p3q2')
    d = pr['d']
    e, mu, var, it, hist, _ = R.elbo_calc(*pr['args'], pr['mu0'], pr['var0'], order='reference')
    assert it == int(d['calc_iter'])
    np.testing.assert_allclose(hist, d['calc_elbo_array'], rtol=RTOL)
    _cases.assert_state('order ref ELBOcalc step_p3q2', mu, d['calc_mu'], var, d['calc_var'])


# ------------------------------------------------------------------ the public interface, no device
def _data(p=2, N=10, seed=0):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(N)) * 10
    return t, rng.randn(p, N), rng.rand(p, N) + 0.1


def _args(y, e):
    return [a for i in range(y.shape[0]) for a in (y[i], e[i])]


def test_validation_raises_before_any_device_call():
    t, y, e = _data()
    g = gpyrn.inference(2, t, *_args(y, e))
    assert g.sweep_order == 'reference' and g._ctx is None
    g = gpyrn.inference(2, t, *_args(y, e), sweep_order='sequential')
    assert g.sweep_order == 'sequential' and g._ctx is None
    g.sweep_order = 'reference'
    assert g.sweep_order == 'reference' and g._ctx is None
    for bad in ('jacobi', 'Sequential', 1, None):
        with pytest.raises(ValueError, match='sweep_order'):
            gpyrn.inference(2, t, *_args(y, e), sweep_order=bad)
        with pytest.raises(ValueError, match='sweep_order'):
            g.sweep_order = bad
    assert g.sweep_order == 'reference'

    m = np.ones((2, 10), dtype=bool)
    m[0, 2] = False
    with pytest.raises(NotImplementedError, match='mask'):
        gpyrn.inference(2, t, *_args(y, e), mask=m, sweep_order='sequential')
    gm = gpyrn.inference(2, t, *_args(y, e), mask=m)
    with pytest.raises(NotImplementedError, match='mask'):
        gm.sweep_order = 'sequential'
    assert gm.sweep_order == 'reference' and gm._ctx is None

    class FakeComm:
        world, rank, local_rank = 2, 0, 0
    with pytest.raises(NotImplementedError, match='sharded'):
        gpyrn.inference(2, t, *_args(y, e), comm=FakeComm(), sweep_order='sequential')
    gc = gpyrn.inference(2, t, *_args(y, e), comm=FakeComm())
    with pytest.raises(NotImplementedError, match='sharded'):
        gc.sweep_order = 'sequential'

    s = [(t, y[0], e[0]), (t[:7], y[1, :7], e[1, :7])]
    assert gpyrn.inference.from_series(2, s).sweep_order == 'reference'
    with pytest.raises(NotImplementedError, match='mask'):
        gpyrn.inference.from_series(2, s, sweep_order='sequential')


def test_set_sweep_order_is_in_the_header_and_the_binding():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gprn_hip.h')).read(), flags=re.S)
    assert re.search(r'int\s+gprn_set_sweep_order\s*\(\s*gprn_ctx\*\s*\w+\s*,\s*int\s+\w+\s*\)', text)
    ids = dict(re.findall(r'(GPRN_ORDER_[A-Z]+)\s*=\s*(\d+)', text))
    assert ids == {'GPRN_ORDER_REFERENCE': str(_hip.ORDER_REFERENCE), 'GPRN_ORDER_SEQUENTIAL': str(_hip.ORDER_SEQUENTIAL)}
    assert 'gprn_set_sweep_order' in _hip.SIGNATURES and hasattr(_hip.Context, 'set_sweep_order')
    if os.path.exists(_hip.LIB_PATH):
        assert hasattr(_hip.load_library(), 'gprn_set_sweep_order')
