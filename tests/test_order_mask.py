"""The sequential sweep order under a data mask without a GPU: the restatement (tests/_order_mask_ref.py) against the two
restatements it combines, the point of the combination at q = 3 on the restatement alone, and the keyword
``sequential_under_mask`` validated before any device call."""
import numpy as np
import pytest

import gpyrn_amd as gpyrn
from tests import _cases, _mask_ref as M, _order_mask_ref as R, _order_ref as O

RTOL = 1e-8


@pytest.mark.parametrize('tag', ['step_p2q3', 'step_p3q2', 'kmix_N200_p2q2'])
def test_all_true_mask_sequential_is_the_unmasked_sequential_restatement(tag):
    """Explicit Sigma pred against the B-form of tests/_order_ref.py, two sweeps (measured: ELBO <= 6.5e-12, state <= 2e-13)."""
    po = O.problem(tag)
    pm = M.problem(tag)
    mask = np.ones(pm['y_raw'].shape, dtype=bool)
    mu, var = po['mu0'], po['var0']
    mu_m, var_m = mu, var
    for _ in range(2):
        e_o, mu, var, parts_o = O.sweep(*po['args'], mu, var, order='sequential')
        e, mu_m, var_m, parts = R.sweep(*R.args(pm), mu_m, var_m, mask, order='sequential')
        print(tag, 'ELBO rel', abs(e / e_o - 1), 'parts rel', np.abs(np.array(parts) / np.array(parts_o) - 1).max())
        np.testing.assert_allclose(e, e_o, rtol=RTOL)
        np.testing.assert_allclose(parts, parts_o, rtol=RTOL)
        _cases.assert_state('all-True mask, sequential ' + tag, mu_m, mu, var_m, var)


@pytest.mark.parametrize('tag,seed', [('step_p2q3', 3), ('step_p3q2', 5)])
def test_reference_order_is_the_masked_restatement(tag, seed):
    pm = M.problem(tag)
    p, N = pm['y_raw'].shape
    mask = M.partial_mask(p, N, seed=seed)
    assert not mask.all()
    mu, var = M.init_state(pm, mask)
    a = M.sweeps(*R.args(pm), mu, var, mask, 2)
    b = R.sweeps(*R.args(pm), mu, var, mask, 2, order='reference')
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_under_a_mask_the_first_sweep_shares_variances_and_group_zero():
    """d reads none of the means the order is about -- under a mask too, rows of zero precision included."""
    pm = M.problem('step_p2q3')
    mask = M.partial_mask(2, 40, seed=3)
    mu, var = M.init_state(pm, mask)
    _, mu_r, var_r, _ = R.sweep(*R.args(pm), mu, var, mask, order='reference')
    _, mu_s, var_s, _ = R.sweep(*R.args(pm), mu, var, mask, order='sequential')
    assert np.array_equal(var_s[0], var_r[0])                  # every node variance
    assert np.array_equal(mu_s[0, 0], mu_r[0, 0])              # mu_f0
    assert np.array_equal(var_s[1:, 0], var_r[1:, 0])          # the variances of node 0's weights, U rows included
    assert not np.allclose(mu_s[0, 1], mu_r[0, 1], rtol=1e-6, atol=0)


def test_at_three_nodes_under_a_mask_the_reference_order_diverges_and_the_sequential_one_stops():
    """The point of the combination, on the restatement alone: step_p2q3 with 22.5 % of its entries masked."""
    pm = M.problem('step_p2q3')
    mask = M.partial_mask(2, 40, seed=3)
    print('masked fraction', 1 - mask.mean())
    mu0, var0 = M.init_state(pm, mask)
    E, _, _, _ = R.sweeps(*R.args(pm), mu0, var0, mask, 5, order='reference')
    print('reference order, trips 1-5:', E)
    assert abs(E[4]) > 1e4 * abs(E[0])
    e, mu, var, it, hist, crit = R.elbo_calc(*R.args(pm), mu0, var0, mask, max_iter=200, order='sequential')
    print('sequential order: trips', it, 'ELBO', hist[1], '->', e, 'criterion', crit[-1], 'max |mu|', np.abs(mu).max())
    assert it == 17 and crit[-1] < 1e-3                        # the rule fired
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(mu)) and np.all(np.isfinite(var)) and np.all(var > 0)


# ------------------------------------------------------------------ the public interface, no device
def _data(p=2, N=10, seed=0):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(N)) * 10
    return t, rng.randn(p, N), rng.rand(p, N) + 0.1


def _args(y, e):
    return [a for i in range(y.shape[0]) for a in (y[i], e[i])]


def test_the_keyword_lifts_the_refusal_before_any_device_call():
    t, y, e = _data()
    m = np.ones((2, 10), dtype=bool)
    m[0, 2] = False
    s = [(t, y[0], e[0]), (t[:7], y[1, :7], e[1, :7])]

    # default: today's refusals, in the constructor, the setter and from_series
    with pytest.raises(NotImplementedError, match='mask'):
        gpyrn.inference(2, t, *_args(y, e), mask=m, sweep_order='sequential')
    gm = gpyrn.inference(2, t, *_args(y, e), mask=m)
    assert gm.sequential_under_mask is False
    with pytest.raises(NotImplementedError, match='mask'):
        gm.sweep_order = 'sequential'
    assert gm.sweep_order == 'reference' and gm._ctx is None
    with pytest.raises(NotImplementedError, match='mask'):
        gpyrn.inference.from_series(2, s, sweep_order='sequential')
    with pytest.raises(NotImplementedError, match='mask'):
        gpyrn.inference(2, t, *_args(y, e), mask=m, sweep_order='sequential', sequential_under_mask=False)

    # keyword set: all three accept
    g = gpyrn.inference(2, t, *_args(y, e), mask=m, sweep_order='sequential', sequential_under_mask=True)
    assert g.sweep_order == 'sequential' and g.sequential_under_mask is True and g._ctx is None
    g = gpyrn.inference(2, t, *_args(y, e), mask=m, sequential_under_mask=True)
    assert g.sweep_order == 'reference'
    g.sweep_order = 'sequential'
    assert g.sweep_order == 'sequential' and g._ctx is None
    g.sweep_order = 'reference'
    assert g.sweep_order == 'reference' and g._ctx is None
    g = gpyrn.inference.from_series(2, s, sweep_order='sequential', sequential_under_mask=True)
    assert g.sweep_order == 'sequential' and g.mask is not None and not g.mask.all() and g._ctx is None
    # the attribute may be set later
    gm.sequential_under_mask = True
    gm.sweep_order = 'sequential'
    assert gm.sweep_order == 'sequential' and gm._ctx is None

    # a comm is still refused (mask and comm refuse each other as before; the order on a sharded object too)
    class FakeComm:
        world, rank, local_rank = 2, 0, 0
    with pytest.raises(NotImplementedError, match='sharded'):
        gpyrn.inference(2, t, *_args(y, e), comm=FakeComm(), sweep_order='sequential', sequential_under_mask=True)
    with pytest.raises(NotImplementedError, match='sharded'):
        gpyrn.inference(2, t, *_args(y, e), comm=FakeComm(), mask=m, sweep_order='sequential', sequential_under_mask=True)
    gc = gpyrn.inference(2, t, *_args(y, e), comm=FakeComm(), sequential_under_mask=True)
    with pytest.raises(NotImplementedError, match='sharded'):
        gc.sweep_order = 'sequential'
    assert gc._ctx is None
