"""The problem of tests/test_schedule_matrix_gpu.py (tests/_schedule_cases.py: N = 1290, p = 2, q = 3) on the CPU: its shape is
what the GPU module's comments say it is, and its restatements agree with each other far inside the bound they are used at."""
import numpy as np

from tests import _cases, _mask_ref, _order_mask_ref, _schedule_cases as S


def test_the_shape_runs_the_full_outer_panel_schedule():
    """The arithmetic of ensure_tasks (csrc/factor.hip) for T = 11, GPRN_OUTER = 4, restated: three outer panels, a first-touch
    B tile and rows of R in the first panel's "rest", both phases above GPRN_LAT_MAX."""
    T, outer, lat_max = S.T, 4, 32
    assert (S.N, T, T * S.TILE, S.N - (T - 1) * S.TILE) == (1290, 11, 1408, 10)
    assert S.Q * T > lat_max and S.Q * S.P * T > lat_max
    panels = [(k0, min(T, k0 + outer)) for k0 in range(0, T, outer)]
    assert panels == [(0, 4), (4, 8), (8, 11)]
    k1 = panels[0][1]
    n1 = min(T, k1 + outer)
    n2 = min(T, n1 + outer)

    def cls_b(i, j):
        if j < n1 and i <= j + 1:
            return -2
        if j == k1:
            return 0
        if j < n1 or (j < n2 and i <= j + 1):
            return 1
        return 2
    rest_b = [(i, j) for i in range(k1, T) for j in range(k1, i + 1) if cls_b(i, j) == 2]
    rest_r = [i for i in range(k1, T) if i >= n1]
    assert rest_b == [(10, 8)] and rest_r == [8, 9, 10]
    # the runs of masked entries: across a tile boundary, across the boundary of outer panels 1 and 2, inside the last tile
    mask = S.data_mask()
    assert mask.any(axis=0).all()                             # (q >= 2: every time keeps an observed output)
    z0, z1 = S.ZERO_ROWS
    assert z0.size + z1.size == 40 and not mask[0, z0].any() and not mask[1, z1].any()
    assert {255, 256}.issubset(set(z0)) and {1023, 1024}.issubset(set(z1))
    assert np.sum(z0 >= (T - 1) * S.TILE) == 4 and np.sum(z1 >= (T - 1) * S.TILE) == 4
    assert (~mask).sum(axis=1).min() > 0.15 * S.N


def test_the_restatements_agree_under_an_all_true_mask():
    """Conditioning of the chosen kernels: with an all-True mask and the reference's order, tests/_mask_ref.py's and
    tests/_order_mask_ref.py's sweeps (explicit Sigma = K - K S (I + S K S)^-1 S K, cho_solve traces) and oracle/cpu_ref.py's
    (the B-form) are three roundings of one computation.  Over the four sweeps they agree to 1e-10 on the ELBO and its parts
    and to _cases.assert_state's bound on the state, so the 1e-8 of the GPU module is not eaten by cond(K) ~ 1e9 of the
    SquaredExponential weights under the 1e-6 nugget.  Measured (both modules alike): 3.0e-12 on the ELBO, 5.3e-13 on its parts;
    means 2.6e-13, 2.1e-13, 4.3e-13, 1.1e-12 and variances 9.3e-13, 3.0e-12, 5.8e-12, 2.6e-11 after sweeps 1 .. 4."""
    ref = S.reference('plain')
    pr = ref['pr']
    every = np.ones((S.P, S.N), dtype=bool)
    args = (pr['Kf'], pr['Kw'], pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2'])
    for name, sweep in (('_mask_ref', lambda mu, var: _mask_ref.sweep(*args, mu, var, every)),
                        ('_order_mask_ref', lambda mu, var: _order_mask_ref.sweep(*args, mu, var, every, 'reference'))):
        E, parts, states = S.run_sweeps(sweep, pr['mu0'], pr['var0'])
        print(name, 'ELBO rel %.2e, parts rel %.2e' % (np.abs(E / ref['elbo'] - 1).max(), np.abs(parts / ref['parts'] - 1).max()),
              'state (means, variances) per sweep', ['%.1e %.1e' % (_cases._rowwise(m, rm), _cases._rowwise(v, rv))
                                                     for (m, v), (rm, rv) in zip(states, ref['states'])])
        np.testing.assert_allclose(E, ref['elbo'], rtol=1e-10)
        np.testing.assert_allclose(parts, ref['parts'], rtol=1e-10)
        for k, ((mu, var), (mu_r, var_r)) in enumerate(zip(states, ref['states'])):
            _cases.assert_state('%s against cpu_ref, all-True mask, sweep %d' % (name, k + 1), mu, mu_r, var, var_r)
            assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
