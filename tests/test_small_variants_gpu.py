"""Every instantiation of the one-tile kernels, reached by name and held against a NumPy restatement.

The launchers of csrc/smalln.hip and csrc/order.hip select a kernel variant from runtime flags (with_flags): the data mask
(MASKED), the ELBO form (BOUND), forced batches (FORCED), the prior's substitution panels (ACC), tiles per edge (T) and the
half-sweep (WEIGHTS).  A wrong arm launches a valid kernel that computes something else, so each of the eight combinations of
(data mask, sweep order, ELBO form) runs

    single, N = 40     k_small_prior<1, ACC>, k_small_phase<W, 1, M>, k_order_small<W, 1, M>, k_small_tail<1, M, B>
    single, N = 150    the same at T = 2 (option "small_path" = 2; single-problem forms only)
    batch, forced      k_small_prior_b<1, ACC>, k_small_phase_b<W, M>, k_order_small_b<W, M>, k_small_tail_b<1, M, true, B>
    batch, stop rule   ... k_small_tail_b<1, M, false, B>

for W in {node, weight}, with ACC = true (the default) and, on the plain combination, ACC = false as well.  The restatements are
tests/_small_variant_cases.py's (composed by tests/_schedule_cases.compose_sweep): p = q = 2, three parameter vectors that
differ in every parameter, three forced sweeps.  Bounds: the project's -- 1e-8 relative on every sweep's ELBO and its three
parts (a batch returns the value alone), _cases.assert_state on the state; trip counts equal.  On the CPU the two routes of each
restatement (B-form against explicit Sigma) agree to 4.2e-11 on ELBO and parts and 2.8e-11 on the state over the three sweeps
at both sizes, and the stop rule's criterion stays 2.3e-3 of its threshold away from it at least: the bounds measure the device.
"""
import numpy as np
import pytest

from tests import _cases, _small_variant_cases as C

pytestmark = pytest.mark.gpu
RTOL = 1e-8
IDS = [C.combo_id(c) for c in C.COMBOS]
PLAIN = (False, 'reference', 'reference')


def _single(N, combo, acc=None):
    """Three forced sweeps of every parameter vector on a single context, each against its own restatement."""
    ref = C.reference(N, combo)
    g = C.model(N, combo)
    ctx = g._backend()
    if N > 128:
        ctx.option('small_path', 2)
    if acc is not None:
        ctx.option('accurate_factor', acc)
    for k, (x, r) in enumerate(zip(ref['sets'], ref['vectors'])):
        g.set_parameters(x.copy())
        ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
        assert g.last_info == 0
        ctx.set_muvar(ref['mu0'], ref['var0'])
        elbo, parts, info = ctx.sweep(C.N_SWEEPS, commit=True)
        assert info == 0
        mu, var = ctx.get_muvar()
        print('small_variants single N %d %s acc %s vector %d: ELBO rel %.2e, parts rel %.2e, means %.2e, variances %.2e' % (
            N, C.combo_id(combo), acc, k, np.abs(elbo / r['elbo'] - 1).max(), np.abs(parts / r['parts'] - 1).max(),
            _cases._rowwise(mu, r['states'][-1][0]), _cases._rowwise(var, r['states'][-1][1])))
        np.testing.assert_allclose(elbo, r['elbo'], rtol=RTOL)
        np.testing.assert_allclose(parts, r['parts'], rtol=RTOL)
        _cases.assert_state('single N %d %s vector %d' % (N, C.combo_id(combo), k), mu, r['states'][-1][0], var, r['states'][-1][1])
    assert ctx.option('fallbacks') == 0


def _batch(combo, forced, acc=None):
    """The three vectors side by side, slot by slot against each vector's own restatement."""
    ref = C.reference(C.N_ONE, combo)
    g = C.model(C.N_ONE, combo)
    staged = g._batch_stage([x.copy() for x in ref['sets']], start=(ref['mu0'], ref['var0']))
    assert staged is not None, 'the side-by-side form does not apply'
    ctx, kp, yr, jt, m0, v0 = staged
    if acc is not None:
        ctx.option('accurate_factor', acc)
    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, C.N_SWEEPS if forced else C.MAX_ITER, want_state=True, forced=forced)
    assert res is not None, 'the library has no batched form for this problem'
    elbo, iters, conv, info, mu, var = res
    assert not info.any() and ctx.option('batch_chunk') == len(ref['sets']) and ctx.option('fallbacks') == 0
    for b, r in enumerate(ref['vectors']):
        want, mu_r, var_r = (r['elbo'][-1],) + r['states'][-1] if forced else (r['loop_elbo'], r['loop_mu'], r['loop_var'])
        print('small_variants batch %s %s acc %s slot %d: ELBO rel %.2e, means %.2e, variances %.2e, trips %d' % (
            C.combo_id(combo), 'forced' if forced else 'stop rule', acc, b, abs(elbo[b] / want - 1),
            _cases._rowwise(mu[b], mu_r), _cases._rowwise(var[b], var_r), iters[b]))
        if forced:
            assert iters[b] == C.N_SWEEPS and not conv[b]
        else:
            assert min(abs(c - 1e-3) for c in r['crit']) > 1e-4 * 1e-3        # (the restatement's trip count is the rule's)
            assert 3 < r['trips'] < C.MAX_ITER and iters[b] == r['trips'] and conv[b]
        np.testing.assert_allclose(elbo[b], want, rtol=RTOL)
        _cases.assert_state('batch %s slot %d' % (C.combo_id(combo), b), mu[b], mu_r, var[b], var_r)
    assert len({float(e) for e in elbo}) == len(elbo)               # (the slots differ: a lane mix-up cannot hide)


@pytest.mark.parametrize('combo', C.COMBOS, ids=IDS)
def test_three_forced_sweeps_on_one_tile(combo):
    _single(C.N_ONE, combo)


@pytest.mark.parametrize('combo', C.COMBOS, ids=IDS)
def test_three_forced_sweeps_on_two_tiles(combo):
    _single(C.N_TWO, combo)


@pytest.mark.parametrize('combo', C.COMBOS, ids=IDS)
def test_a_forced_batch_slot_by_slot(combo):
    _batch(combo, forced=True)


@pytest.mark.parametrize('combo', C.COMBOS, ids=IDS)
def test_a_batch_under_the_stop_rule_slot_by_slot(combo):
    _batch(combo, forced=False)


@pytest.mark.parametrize('acc', [0, 1])
def test_the_prior_factor_forms_single_and_batch(acc):
    """Option "accurate_factor": 0 runs k_small_prior<T, false> / k_small_prior_b<1, false> (product panels), 1 the
    substitution panels; both meet the same bounds."""
    _single(C.N_ONE, PLAIN, acc)
    _single(C.N_TWO, PLAIN, acc)
    _batch(PLAIN, True, acc)
    _batch(PLAIN, False, acc)

