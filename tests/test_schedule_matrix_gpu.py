"""Data masks, the sweep orders and the two ELBO forms on the FULL outer-panel schedule of a sweep (csrc/api_sweep.hip:
phase_core, run_phase, sweep_impl; csrc/factor.hip: factor_invert_launches), on the flag schedule and on the event schedule a
time-out falls back to, under every bit of option "overlap", with "accurate_factor" in the sweeps, gprn_keep_sigma, and
through the consumers of what a committed sweep leaves in the workspaces (gprn_grad_elbo, the posterior form of prediction).

The problem is tests/_schedule_cases.py's: q = 3, p = 2, N = 1290 -- T = 11 tiles, ld = 1408, a last tile of 10 rows -- the
smallest shape on which both phases take the throughput task lists, there are three outer panels, the first panel's "rest"
holds a first-touch B tile (10, 8) and rows of R, rows_final runs between panels and node_joins is true, so that the ends of
sweeps 1 .. 3 of a call of four are deferred (that module's docstring derives each of these from ensure_tasks and sweep_impl;
tests/test_schedule_matrix.py restates the arithmetic).  Under the mask 15-30 % of each output is unobserved, with runs of
masked entries across a tile boundary, across the boundary of two outer panels and inside the ragged last tile: rows of zero
precision of the weight phase's matrices (the node phase has none at q >= 2: the library refuses a time at which every output
is masked).

Six configurations, each against its NumPy restatement (four forced sweeps, computed once per process):
plain (oracle/cpu_ref.py), mask (tests/_mask_ref.py), sequential (tests/_order_ref.py), order_mask (tests/_order_mask_ref.py),
bound and bound_order_mask (tests/_bound_ref.py, route 'B').  Tolerances: the project's own -- 1e-8 on every sweep's ELBO and on
its parts, _cases.assert_state on the state, rows of zero precision included.  On this problem the restatements agree with
each other to 3e-12 on the ELBO, 6e-13 on its parts, 1.2e-12 / 2.7e-11 on the means / variances over the four sweeps
(tests/test_schedule_matrix.py), so the bound measures the device.

Not here: the one-tile and mid-size batch paths (smalln.hip, midn.hip) do not take the outer-panel schedule at their sizes
(one or two tiles; T = 3 at N = 300), and on a sharded context may_defer is off and the phases hold one or two matrices.
"""
import contextlib
import os

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip
from tests import _cases, _grad_ref as GR, _schedule_cases as S

pytestmark = pytest.mark.gpu
RTOL = 1e-8
PROJECT_BOUND = 1e-8
OVERLAPS = (0, 1, 2, 4, 8, 16, 31)
NAMES = tuple(S.CONFIGS)

_MODELS = {}
_RUNS = {}
_DEVICE_ERROR = []


@contextlib.contextmanager
def _guard():
    """After a device error nothing more of this module runs on the GPU."""
    if _DEVICE_ERROR:
        pytest.fail('an earlier case of this module met a device error (%s): nothing more is run on the GPU' % _DEVICE_ERROR[0])
    try:
        yield
    except _hip.BackendError as exc:
        _DEVICE_ERROR.append(str(exc))
        raise


def _model(name):
    """The inference object of configuration `name` and its context, set up once; the masked y / yerr handed over are NaN /
    inf."""
    if name not in _MODELS:
        masked, order, form = S.CONFIGS[name]
        pr = S.problem(masked)
        y, e, mask = pr['y_raw'], pr['yerr'], pr['mask']
        if masked:
            y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
        args = [a for i in range(S.P) for a in (y[i], e[i])]
        g = gpyrn.inference(S.Q, pr['time'], *args, mask=mask, sweep_order=order, sequential_under_mask=True, elbo=form)
        g.set_components(pr['nodes'], pr['weights'], pr['means'], pr['jitters'])
        with _guard():
            ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
        assert g.last_info == 0 and g.N == S.N
        _MODELS[name] = (g, ctx)
    return _MODELS[name]


def _default_flags(ctx):
    return 1 if ctx.option('flags') else 0


def _call(ctx, pr, overlap):
    """One committed call of four forced sweeps from the problem's starting state under `overlap`: (elbo (4,), parts (4, 3),
    mu, var)."""
    ctx.option('overlap', overlap)
    ctx.set_muvar(pr['mu0'], pr['var0'])
    elbo, parts, info = ctx.sweep(S.N_SWEEPS, commit=True)
    assert info == 0
    return (elbo, parts) + ctx.get_muvar()


def _runs(name, flags):
    """The calls of part 1 for (configuration, flags), made once: {overlap: (elbo, parts, mu, var)} plus 'fallbacks' and 'flags'
    as the context reads them afterwards.  flags = 1 is skipped where the context has no device-side flags."""
    g, ctx = _model(name)
    if flags and not ctx.option('flags'):
        pytest.skip('device-side flags are off for this context (GPRN_FLAGS=0, a serialising tool or no stream memory operations)')
    key = (name, flags)
    if key not in _RUNS:
        pr = S.problem(S.CONFIGS[name][0])
        out = {}
        try:
            with _guard():
                old = ctx.option('flags', flags)
                try:
                    for overlap in OVERLAPS:
                        out[overlap] = _call(ctx, pr, overlap)
                    out['fallbacks'], out['flags'] = ctx.option('fallbacks'), ctx.option('flags')
                finally:
                    ctx.option('overlap', 31)
                    ctx.option('flags', old)
            _RUNS[key] = (out, None)
        except Exception as exc:                               # (kept: the case is not run a second time)
            _RUNS[key] = (None, exc)
    out, exc = _RUNS[key]
    if exc is not None:
        raise exc
    return out


def _figures(res, ref):
    elbo, parts, mu, var = res
    mu_r, var_r = ref['states'][-1]
    return (float(np.abs(elbo / ref['elbo'] - 1).max()), float(np.abs(parts / ref['parts'] - 1).max()),
            _cases._rowwise(mu, mu_r), _cases._rowwise(var, var_r))


def _assert_matches_the_restatement(what, res, ref):
    """Part 2's comparison: every sweep's ELBO and parts to 1e-8, the state by _cases.assert_state (all rows), all finite."""
    elbo, parts, mu, var = res
    print('schedule_matrix %s: ELBO rel %.2e, parts rel %.2e, means %.2e, variances %.2e' % ((what,) + _figures(res, ref)))
    for a in res:
        assert np.all(np.isfinite(a))
    np.testing.assert_allclose(elbo, ref['elbo'], rtol=RTOL)
    np.testing.assert_allclose(parts, ref['parts'], rtol=RTOL)
    mu_r, var_r = ref['states'][-1]
    _cases.assert_state('schedule matrix, ' + what, mu, mu_r, var, var_r)


def _same_bits(a, b, what):
    for x, y, part in zip(a, b, ('ELBO', 'parts', 'means', 'variances')):
        assert np.array_equal(x, y), '%s: the %s differ (largest deviation %.3g)' % (what, part, np.abs(np.asarray(x) - y).max())


# ------------------------------------------------------------------ 1. bits across the overlap masks
@pytest.mark.parametrize('flags', [1, 0])
@pytest.mark.parametrize('name', NAMES)
def test_every_overlap_mask_gives_the_same_bits(name, flags):
    """Four committed sweeps from one starting state under overlap 0, 1, 2, 4, 8, 16 and 31: every sweep's ELBO, its parts and
    the state are those of overlap = 0, bit for bit.  A deviation under one bit alone points at that bit's hand-over (1: the
    first-touch build of B from K and s on the bulk stream; 2: rows_final between panels; 4: the node term beside the weight
    phase; 8: log det B in k_reduce_finalize; 16: mu_k_mu and vec_elbo of sweeps 1 .. 3 beside the next node phase, which
    rewrites the state rows they read).  On the flag schedule no call may have fallen back."""
    runs = _runs(name, flags)
    for overlap in OVERLAPS:
        for a in runs[overlap]:
            assert np.all(np.isfinite(a)), overlap
        _same_bits(runs[overlap], runs[0], '%s, flags %d, overlap %d against 0' % (name, flags, overlap))
    assert not np.allclose(runs[0][0][0], runs[0][0][-1], rtol=1e-6)       # (the state moves: a stale read cannot hide)
    assert runs['fallbacks'] == 0
    if flags:
        assert runs['flags'] == 1


# ------------------------------------------------------------------ 2. overlap = 0 against the restatement
@pytest.mark.parametrize('flags', [1, 0])
@pytest.mark.parametrize('name', NAMES)
def test_the_sequential_launch_order_matches_the_restatement(name, flags):
    """overlap = 0 (with part 1: every mask) against the configuration's restatement, each of the four sweeps: the deferred ends
    are those of sweeps 1 .. 3."""
    runs = _runs(name, flags)
    _assert_matches_the_restatement('%s flags %d' % (name, flags), runs[0], S.reference(name))


# ------------------------------------------------------------------ 3. flags against events
@pytest.mark.parametrize('name', NAMES)
def test_the_flag_and_the_event_schedule_give_the_same_bits(name):
    """factor_invert_launches hands every task to the same arithmetic on both schedules: the chain's kernels (k_diag_block,
    launch_tile_rows), the in-panel and outer updates and the last step's row take the same kernels with the same task ranges
    and shapes (shape_upd and the first-touch decision read the task counts only).  ONE launch differs in form: the panel of a
    tile step on stream3 is one k_tile_panel launch under flags and two k_tile_gemm launches (TS_64x128_BTRI, TS_128x64_ATRI)
    under events -- both run tile_mma<64, 128, 2, 2, 1> / tile_mma<128, 64, 2, 2, 2> on the same tasks (and, with
    accurate_factor, launch_tiles sends the L half to k_tile_panel<true> on either schedule).  The split of an in-panel update
    into its critical tiles and the rest, and the folded synchronisation, are for phases of one or two matrices: not here.
    Everything else is streams and waits (the sweep's end is in line under events: may_defer asks for flags).  So the two
    schedules must agree bit for bit, under every overlap mask; both are held against the restatement in part 2 as well."""
    with_flags, with_events = _runs(name, 1), _runs(name, 0)
    for overlap in OVERLAPS:
        _same_bits(with_flags[overlap], with_events[overlap], '%s, overlap %d, flags against events' % (name, overlap))


# ------------------------------------------------------------------ 4. accurate_factor in the sweeps
@pytest.mark.parametrize('flags', [1, 0])
@pytest.mark.parametrize('name', ['plain', 'mask', 'bound_order_mask'])
def test_accurate_factor_in_the_sweeps(name, flags):
    """Option "accurate_factor" set behind the set-up (the priors keep their default, substitution, factors), overlap = 31:
    0 is the sweeps' default (product panels) and 1 runs k_tile_panel<true> -- C = A in place -- on B matrices beside the
    first-touch build, rows_final and the deferred ends.  Each meets part 2's bound; -2 brings the default's bits back."""
    default = _runs(name, flags)[31]
    g, ctx = _model(name)
    pr, ref = S.problem(S.CONFIGS[name][0]), S.reference(name)
    out = {}
    with _guard():
        old = ctx.option('flags', flags)
        try:
            for acc in (0, 1, -2):
                ctx.option('accurate_factor', acc)
                out[acc] = _call(ctx, pr, 31)
            assert ctx.option('fallbacks') == 0
        finally:
            ctx.option('accurate_factor', -2)
            ctx.option('flags', old)
    for acc in (0, 1):
        _assert_matches_the_restatement('%s flags %d accurate_factor %d' % (name, flags, acc), out[acc], ref)
    _same_bits(out[-2], default, '%s, flags %d: accurate_factor back at its default' % (name, flags))
    _same_bits(out[0], default, '%s, flags %d: accurate_factor 0 is the default of a sweep' % (name, flags))
    assert not np.array_equal(out[1][2], default[2])           # (the substitution panels did run: other roundings)


# ------------------------------------------------------------------ 5. what a committed sweep leaves
N_KERNEL_PARAMETERS = 4 * S.Q + 2 * S.Q * S.P                   # QuasiPeriodic nodes, SquaredExponential weights


def _tstar(pr):
    """Five times, two of them data times: one in the second tile and one inside the ragged last tile (under the mask a row of
    zero precision of output 1's weights), then a gap's midpoint, one before the first and one behind the last time."""
    t = pr['time']
    assert 1285 in S.ZERO_ROWS[1]
    return np.array([t[300], t[1285], 0.5 * (t[700] + t[701]), t[0] - 1.3, t[-1] + 2.1])


def _consumers(name):
    """After the committed call under overlap 0, 16 and 31: gprn_grad_elbo and the posterior form of gprn_predict at _tstar."""
    g, ctx = _model(name)
    key = (name, 'consumers')
    if key not in _RUNS:
        pr = S.problem(S.CONFIGS[name][0])
        out = {}
        try:
            with _guard():
                try:
                    for overlap in (0, 16, 31):
                        _call(ctx, pr, overlap)
                        assert ctx.option('state_ready') == 1
                        grad = ctx.grad_elbo(N_KERNEL_PARAMETERS)
                        old = ctx.option('predict_form', _hip.PREDICT_POSTERIOR)
                        try:
                            mean, var, info = ctx.predict(_tstar(pr))
                        finally:
                            ctx.option('predict_form', old)
                        assert info == 0
                        out[overlap] = (grad, mean, var)
                    assert ctx.option('fallbacks') == 0
                finally:
                    ctx.option('overlap', 31)
            _RUNS[key] = (out, None)
        except Exception as exc:                               # (kept: the case is not run a second time)
            _RUNS[key] = (None, exc)
    out, exc = _RUNS[key]
    if exc is not None:
        raise exc
    return out


@pytest.mark.parametrize('name', ['plain', 'order_mask', 'bound'])
def test_gradient_and_posterior_prediction_read_the_same_workspaces_under_every_mask(name):
    """gprn_grad_elbo and the posterior form of prediction read X, s and X^T X z of the LAST sweep from the workspaces that
    the Q1 product (it overwrites BUF_B) and the deferred ends also touch: the same bits after overlap 0, 16 and 31."""
    out = _consumers(name)
    for overlap in (16, 31):
        for a, b, part in zip(out[overlap], out[0], ('gradient', 'predictive means', 'predictive variances')):
            assert np.all(np.isfinite(a))
            assert np.array_equal(a, b), '%s, overlap %d against 0: the %s differ' % (name, overlap, part)
    grad, mean, var = out[0]
    assert grad.shape == (N_KERNEL_PARAMETERS,) and np.all(grad != 0.0)
    assert mean.shape == var.shape == (S.Q + S.Q * S.P, 5) and np.all(var > 0.0)


def test_the_gradient_behind_four_sweeps_matches_the_restatement():
    """The plain configuration's gprn_grad_elbo behind the four-sweep call against tests/_grad_ref.py at the restatement's own
    fourth sweep (from its state after three), in the norm and at the bound of
    tests/test_grad_fused_gpu.py::test_fused_gradient_against_the_restatement: |dev - ref| / sum |G| |dK/dtheta| below the larger
    of 100 x the spread of the restatement's two LAPACK routes and the deviation of the explicit path (gprn_grad_kernel after a
    keep_sigma sweep) from the same restatement, and below 1e-8.  dK/dtheta: the kernels' own float64 closed forms, evaluated
    once (1e-13 from oracle/kernel_formulas.py's long-double ones, which take half a minute per route at this size).  A state
    that is wrong under every mask alike fails here."""
    name = 'plain'
    ref = S.reference(name)
    pr = ref['pr']
    mu3, var3 = ref['states'][2]
    st = GR.sweep_state(pr, mu3, var3, None)
    np.testing.assert_allclose(st['elbo'], ref['elbo'][3], rtol=1e-10)
    r = pr['time'][:, None] - pr['time'][None, :]
    dks = [[np.asarray(dk, dtype=float) for dk in k._dk_dpars(r)] for k in list(pr['nodes']) + list(pr['weights'])]

    def contract(G):
        return (np.array([np.sum(Gg * dk) / S.Q for Gg, kd in zip(G, dks) for dk in kd]),
                np.array([np.sum(np.abs(Gg) * np.abs(dk)) / S.Q for Gg, kd in zip(G, dks) for dk in kd]))
    want, norm = contract(GR.G_matrices(pr, st, 'chol'))
    want_inv, _ = contract(GR.G_matrices(pr, st, 'inv'))
    assert want.size == N_KERNEL_PARAMETERS
    spread = float((np.abs(want - want_inv) / norm).max())
    g, ctx = _model(name)
    dev = _consumers(name)[31][0] / S.Q
    fused = float((np.abs(dev - want) / norm).max())
    with _guard():
        ctx.set_muvar(mu3, var3)
        ctx.keep_sigma(True)
        try:
            _, _, info = ctx.sweep(1, commit=True)
            assert info == 0
            mu, _ = ctx.get_muvar()
            m_scr = mu[1:].reshape(S.Q, S.P, S.N)
            rows = [mu[0, j] for j in range(S.Q)] + [m_scr[j, i] for j in range(S.Q) for i in range(S.P)]
            par = []
            for gp, (kernel, m) in enumerate(zip(list(g.nodes) + list(g.weights), rows)):
                par += list(ctx.grad_kernel(gp, m, kernel.pars.size) / S.Q)
        finally:
            ctx.keep_sigma(False)
    parent = float((np.abs(np.array(par) - want) / norm).max())
    print('schedule_matrix gradient: fused %.2e, spread of the two LAPACK routes %.2e, explicit path %.2e' % (fused, spread, parent))
    assert fused <= max(100.0 * spread, parent)
    assert fused <= PROJECT_BOUND
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 6. keep_sigma
def test_keep_sigma_changes_no_bit():
    """gprn_keep_sigma(1) switches the deferral off and runs lauum_lower in line behind every phase: the ELBO, its parts and
    the state are those of the call without it (reference form; the bound form and a data mask refuse keep_sigma)."""
    g, ctx = _model('plain')
    flags = _default_flags(ctx)
    without = _runs('plain', flags)[31]
    pr = S.problem(False)
    with _guard():
        ctx.keep_sigma(True)
        try:
            kept = _call(ctx, pr, 31)
            assert ctx.option('fallbacks') == 0
        finally:
            ctx.keep_sigma(False)
            ctx.option('overlap', 31)
    _same_bits(kept, without, 'plain, flags %d: keep_sigma on against off' % flags)
    _assert_matches_the_restatement('plain flags %d keep_sigma' % flags, kept, S.reference('plain'))


@pytest.mark.parametrize('name', ['mask', 'bound'])
def test_keep_sigma_stays_refused_under_a_mask_and_in_the_bound_form(name):
    """... so part 6 has no masked and no bound-form case: the refusal is the contract (include/gprn_hip.h), and the context
    goes on as before."""
    g, ctx = _model(name)
    lib = _hip.load_library()
    assert lib.gprn_keep_sigma(ctx._h, 1) == _hip.GPRN_E_UNSUPPORTED
    flags = _default_flags(ctx)
    with _guard():
        try:
            again = _call(ctx, S.problem(S.CONFIGS[name][0]), 31)
        finally:
            ctx.option('overlap', 31)
    _same_bits(again, _runs(name, flags)[31], '%s: the call behind a refused keep_sigma' % name)


def test_no_call_of_this_module_fell_back():
    for name, (g, ctx) in _MODELS.items():
        assert ctx.option('fallbacks') == 0, name
        if os.environ.get('GPRN_FLAGS', '1') != '0' and not os.environ.get('ROCPROF_COUNTER_COLLECTION'):
            assert ctx.option('flags') == 1, name
