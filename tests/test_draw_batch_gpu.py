"""Joint posterior draws for many vectors side by side (gprn_elbocalc_batch_draws, Context.elbocalc_batch_draws,
inference.sample_posterior_batch, posterior_predictive(draws=k)) on the GPU: every slot against the dense restatement
tests/_draw_batch_ref.py at its own kernels, the loop's outputs against gprn_elbocalc_batch_grad(grad_out = NULL) to the bit,
against the device one by one, across chunks and groups, around a failed pivot, the ladder per slot, at the data times, the
draws' moments, the Python surface and the contract of the entry point.

Shapes: those of tests/test_varpred_batch_gpu.py (its problems, models, vectors and times are imported, not restated) -- (a)
N = 45, p = q = 2, composite + WhiteNoise, masked; (c) N = 129, p = 2, q = 1, masked (the worker); (d) mid_N300_p3q2, masked;
(e) step_p2q3, sequential under a mask; (f) case (d) in the sequential order.  B = 4 vectors (5 where a middle one fails or
chunks are asked for), ns in {129, 300} from V.mixed_times: a ragged second tile of t*, and above ld = 128 / 256 several row
blocks of W.  Forced sweeps, so that the restatement is one sweep from the initial state.

Bounds.  mean*: 1e-8 norm-wise per latent GP (tests/_cases.assert_state).  L L^T - nu I against the restatement's C*: 1e-8
of its largest diagonal entry (COV_TOL of tests/test_predict_cov_gpu.py).  mean* + L z: 1e-12, out = sum_j w o f: 1e-13
(test_draws_with_fixed_normals' bounds: the same code path).  nu in [1.25e-12, 1.25e-6].  Moments: 5 standard errors, the
variance's from the draws' fourth moment (test_draw_moments_match_the_prediction's bound).  L is recovered column by column from
unit vectors z = e_d and compared backward (L L^T), never forward against another factor: C* is singular to rounding.
No call may fall back to the event schedule."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from tests import _cases, _draw_batch_ref as D, _varpred_ref as V
from tests import test_varpred_batch_gpu as VB

pytestmark = pytest.mark.gpu
TOL = 1e-8          # means, norm-wise per latent GP
COV_TOL = 1e-8      # covariances, of the largest diagonal entry
DRAW_TOL = 1e-12
OUT_TOL = 1e-13
POST = _hip.PREDICT_POSTERIOR
NS = (129, 300)
MAX_ITER = VB.MAX_ITER
SCALES, STOP_SCALES = VB.SCALES, VB.STOP_SCALES
FORMS = [('a', 'reference'), ('a', 'bound'), ('c', 'reference'), ('c', 'bound'), ('d', 'reference'), ('e', 'reference'),
         ('e', 'bound'), ('f', 'reference')]
SEED = 20240917     # test 8 (tests/test_draw_batch.py confirms the restatement's own draws under it)


def _in_range(nug):
    return bool(np.all(nug >= D.NU_MIN) and np.all(nug <= D.NU_MAX * 1.0001))


def _reference(pr, mask, order, mu0, var0, g, sets, ts, skip=()):
    """Per vector: the restatement's mean* (G, ns), C* (G, ns, ns) after ONE sweep from (mu0, var0) at that vector's own
    components, and its jitters; None for the vectors in `skip`."""
    out = []
    for b, x in enumerate(sets):
        if b in skip:
            out.append(None)
            continue
        g.set_parameters(np.array(x, dtype=float))
        comp = g._get_components()
        lat_mean, lat_cov, _, _ = D.posterior(pr, mask, order, mu0, var0, comp, ts)
        out.append((lat_mean, lat_cov, tuple(float(j) for j in comp[3])))
    return out


@functools.lru_cache(maxsize=None)
def _restated(name, ns, scales=SCALES):
    """... of the named case's vectors at the mixed times; computed once, shared, never written."""
    pr, mask, order, mu0, var0 = VB._problem(name)
    g = VB._model(name)
    refs = _reference(pr, mask, order, mu0, var0, g, VB._sets(g, scales), VB._times(name, ns))
    for r in refs:
        for a in r[:2]:
            a.setflags(write=False)
    return refs


def _check_every_slot(what, ctx, arrs, ts, refs, p, q):
    """Test 1's checker: three forced one-sweep calls -- z = 0 (the means), z = e_d (L column by column, n_draws = ns) and five
    seeded random draws -- and every slot with a reference against it.  Returns the nuggets (B, G)."""
    kp, yr, jt, m0, v0 = arrs
    B, G, ns = kp.shape[0], q * (p + 1), ts.size
    eye = np.broadcast_to(np.eye(ns), (B, G, ns, ns)).copy()
    z = np.random.default_rng(7).standard_normal((B, G, 5, ns))
    r0 = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, 1, ts, np.zeros((B, G, 1, ns)), forced=True)
    assert r0 is not None, 'the library has no batched form for this problem'
    rI = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, 1, ts, eye, forced=True, outputs=False)
    rz = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, 1, ts, z, forced=True)
    assert rI[7] is None and r0[6].shape == (B, G, 1, ns) and rz[7].shape == (B, p, 5, ns)
    worst = dict(mean=0.0, cov=0.0, draw=0.0)
    for b, ref in enumerate(refs):
        if ref is None:
            continue
        ref_mean, ref_cov, jit = ref
        for r in (r0, rI, rz):
            assert r[3][b] == 0 and r[9][b] == 0 and r[1][b] == 1
            assert np.array_equal(r[8][b], r0[8][b])                       # (the nuggets do not depend on z)
        nug = r0[8][b]
        assert _in_range(nug), nug
        mean = r0[6][b][:, 0, :]
        _cases.assert_state('%s slot %d' % (what, b), mean, ref_mean, tol=TOL)
        worst['mean'] = max(worst['mean'], _cases.ACHIEVED[-1][1])
        for gi in range(G):
            L = (rI[6][b][gi] - mean[gi][None, :]).T                       # column d = L e_d
            assert np.all(L[np.triu_indices(ns, 1)] == 0.0), 'L of slot (%d, %d) is not lower triangular' % (b, gi)
            back = np.abs(L @ L.T - nug[gi] * np.eye(ns) - ref_cov[gi]).max() / np.abs(np.diag(ref_cov[gi])).max()
            worst['cov'] = max(worst['cov'], float(back))
            assert back <= COV_TOL, '%s slot (%d, %d): L L^T - nu I off by %.3g of C*\'s largest diagonal entry' % (what, b, gi, back)
            expect = mean[gi][None, :] + z[b, gi] @ L.T
            off = np.abs(rz[6][b][gi] - expect).max() / np.abs(expect).max()
            worst['draw'] = max(worst['draw'], float(off))
            assert off <= DRAW_TOL, '%s slot (%d, %d): draws off mean + L z by %.3g' % (what, b, gi, off)
        lat = rz[6][b]
        comb = D.output_draws(lat, ref_cov, p, q, jit)
        np.testing.assert_allclose(rz[7][b], comb, rtol=OUT_TOL, atol=OUT_TOL * np.abs(comb).max())
    print('%s ns = %d: worst mean %.2e (norm-wise), L L^T - nu I %.2e (of max diag C*), draws %.2e; nuggets %s' % (
        what, ns, worst['mean'], worst['cov'], worst['draw'], sorted(set(np.ravel(r0[8]).tolist()))))
    return r0[8]


# ------------------------------------------------------------------ 1. every slot is the posterior's draw
@pytest.mark.parametrize('name,elbo', FORMS)
def test_every_slot_is_the_posteriors_draw(name, elbo):
    pr, mask, order, mu0, var0 = VB._problem(name)
    g = VB._model(name, elbo=elbo)
    ctx, *arrs = VB._inputs(g, VB._sets(g), (mu0, var0))
    for ns in NS:
        _check_every_slot('draw_batch %s %s' % (name, elbo), ctx, arrs, VB._times(name, ns), _restated(name, ns), g.p, g.q)
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 2. the loop's outputs keep their bits
@pytest.mark.parametrize('name', ['a', 'd'])
def test_the_loops_outputs_keep_their_bits(name):
    pr, mask, order, mu0, var0 = VB._problem(name)
    g = VB._model(name)
    x = np.array(g.get_parameters(), dtype=float)
    _, kp, yr, jt, m0, v0 = VB._inputs(g, VB._sets(g, STOP_SCALES), (mu0, var0))
    g.set_parameters(x.copy())
    ts = VB._times(name, 300)
    B, G = kp.shape[0], g.q * (g.p + 1)
    z = np.random.default_rng(3).standard_normal((B, G, 2, ts.size))
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    ctx.option('predict_form', POST)

    def swept():
        ctx.set_muvar(mu0, var0)
        e, parts, info = ctx.sweep(1, commit=True)
        assert info == 0
        return [np.asarray(e), np.asarray(parts)] + list(ctx.get_muvar())

    before = swept()
    assert ctx.option('state_ready') == 1
    first = ctx.predict(ts)
    assert not ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, 3, ts, z)[3].any()
    assert ctx.option('state_ready') == 1                          # (the validity flags are not touched)
    for a, b in zip(first, ctx.predict(ts)):                       # (the committed sweep's X, s and ct are where they were)
        assert np.array_equal(a, b)
    for a, b in zip(before, swept()):                              # (the parent's own sweep: the same bits behind the call)
        assert np.array_equal(a, b)
    for forced, trips in ((True, 2), (False, MAX_ITER)):
        plain = ctx.elbocalc_batch(kp, yr, jt, m0, v0, trips, want_state=True, forced=forced)   # (grad_out = NULL)
        res = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, trips, ts, z, forced=forced)
        assert not res[3].any() and not res[9].any()
        for a, b in zip(plain, res[:6]):
            assert np.array_equal(a, b)
        behind = ctx.elbocalc_batch(kp, yr, jt, m0, v0, trips, want_state=True, forced=forced)  # (its task lists are rebuilt)
        for a, b in zip(plain, behind):
            assert np.array_equal(a, b)
        again = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, trips, ts, z, forced=forced)
        for a, b in zip(res, again):
            assert np.array_equal(a, b)
    for a, b in zip(before, swept()):
        assert np.array_equal(a, b)
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 3. against the device one by one
@pytest.mark.parametrize('name', ['a', 'c', 'e'])
def test_against_the_device_one_by_one(name):
    """Both routes are pinned to ONE reference, the restatement after as many sweeps as the loop made; the nuggets are equal
    and the z = 0 rows agree to 1e-12.  No forward comparison of the two factors (test_draws_with_fixed_normals says why)."""
    pr, mask, order, mu0, var0 = VB._problem(name)
    g, g1 = VB._model(name), VB._model(name)
    sets = VB._sets(g)
    ts = VB._times(name, 129)
    ns, G = ts.size, g.q * (g.p + 1)
    ctx, kp, yr, jt, m0, v0 = VB._inputs(g, sets, (mu0, var0))
    B = len(sets)
    eye = np.broadcast_to(np.eye(ns), (G, ns, ns)).copy()
    r0 = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, MAX_ITER, ts, np.zeros((B, G, 1, ns)), outputs=False)
    rI = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, MAX_ITER, ts, np.broadcast_to(eye, (B, G, ns, ns)).copy(), outputs=False)
    assert not r0[3].any() and not r0[9].any() and np.array_equal(r0[1], rI[1])
    for b, x in enumerate(sets):
        g1.set_parameters(x.copy())
        nodes, weights, means, jitters = g1._get_components()
        c1 = g1._setup_device(nodes, weights, means, jitters)
        assert g1.last_info == 0
        c1.option('predict_form', POST)
        c1.set_muvar(np.array(mu0, dtype=float), np.array(var0, dtype=float))
        hist, it1, conv1, info1, mu1, var1 = c1.elbocalc(MAX_ITER)
        assert info1 == 0 and it1 == r0[1][b] and bool(conv1) == bool(r0[2][b])
        lat0, _, nug1, dinfo = c1.predict_draws(ts, np.zeros((G, 1, ns)), outputs=False)
        latI, _, nugI, dinfoI = c1.predict_draws(ts, eye, outputs=False)
        assert dinfo == 0 and dinfoI == 0
        assert np.array_equal(nug1, r0[8][b]) and np.array_equal(nugI, rI[8][b])
        what = 'draw_batch against one by one %s slot %d (%d trips)' % (name, b, it1)
        _cases.assert_state(what, r0[6][b][:, 0, :], lat0[:, 0, :], tol=DRAW_TOL)
        _, ref_cov, _, _ = D.posterior(pr, mask, order, mu0, var0, (nodes, weights, means, jitters), ts, sweeps=int(it1))
        for gi in range(G):
            for route, lI, l0 in (('side by side', rI[6][b][gi], r0[6][b][gi, 0]), ('one by one', latI[gi], lat0[gi, 0])):
                L = (lI - l0[None, :]).T
                assert np.all(L[np.triu_indices(ns, 1)] == 0.0)
                back = np.abs(L @ L.T - nug1[gi] * np.eye(ns) - ref_cov[gi]).max() / np.abs(np.diag(ref_cov[gi])).max()
                assert back <= COV_TOL, '%s, %s, latent GP %d: L L^T - nu I off by %.3g' % (what, route, gi, back)
        assert c1.option('fallbacks') == 0
    print('draw_batch_vs_one_by_one %s: trips %s' % (name, r0[1].tolist()))
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 4. chunks and groups
def _slab_bytes_per_eval(g):
    """What one evaluation takes in a chunk above one tile (csrc/midn.hip mid_bytes_per_eval, restated): 4 G + (q - 1)
    matrices of ld^2, the per-slot vectors, the states and, under a mask, WT and C of every latent GP with unobserved points."""
    N, p, q = g.N, g.p, g.q
    G, ld = q * (p + 1), -(-N // 128) * 128
    T, d = ld // 128, (p + 1) * q * N
    n_q1 = q - 1                                                     # (the reference form of the ELBO)
    dbl = (4 * G + n_q1) * ld * ld + G * ld * (7 + 2 * T + 2) + n_q1 * q // 2 * ld + 2 * d + 2 * p * N + 64
    ne, lane = 0, 0
    if g.mask is not None:
        holes = (~np.asarray(g.mask, dtype=bool)).sum(axis=1)        # (every time keeps an observed output: no node has a U)
        ne = q * int((holes > 0).sum())
        upad = -(-int(holes.max()) // 128) * 128
        dbl += ne * (2 * upad * ld + 4)
        lane = 8 * 8 + 8                                             # (MaskLane: eight pointers and an int, padded)
    return dbl * 8 + ne * lane


def _draw_bytes(g, evals, ns, nd):
    """The draw pass's scratch for a group of `evals` (csrc/batch_layout.h draw_scratch, restated without its paddings)."""
    G, ld = g.q * (g.p + 1), -(-g.N // 128) * 128
    ns_pad, nd_pad, nblk = -(-ns // 128) * 128, -(-nd // 128) * 128, -(-ns // ld)
    per_slot = ns_pad * ld + 3 * ns_pad * ns_pad + 2 * nd_pad * ns_pad + 3 * ns_pad
    return 8 * (evals * G * per_slot + evals * g.p * nd * ns + ns + (nblk * 4 + 3) * evals * G)


@pytest.mark.parametrize('name,B,chunk', [('d', 5, 2), ('c', 3, 3)])
def test_chunks_and_groups(name, B, chunk):
    """(d): the budget holds 2.5 evaluations' slabs, so B = 5 runs as chunks of 2 + 2 + 1, and half an evaluation's slabs are
    left for the pass: groups of one.  (c): the slabs of all three fit, and behind them 1.5 evaluations' scratch: one chunk,
    the pass in groups of one inside it."""
    pr, mask, order, mu0, var0 = VB._problem(name)
    g = VB._model(name)
    scales = STOP_SCALES[:B]
    ctx, *arrs = VB._inputs(g, VB._sets(g, scales), (mu0, var0))
    ts = VB._times(name, 129)
    slab, one = _slab_bytes_per_eval(g), _draw_bytes(g, 1, ts.size, ts.size)
    budget = 2.5 * slab if chunk < B else B * slab + 1.5 * one
    ctx.option('batch_mem_mb', int(np.ceil(budget / 2 ** 20)))
    print('draw_batch chunks %s: %.1f MB of slabs per evaluation, %.1f MB of scratch, budget %d MB' % (
        name, slab / 2 ** 20, one / 2 ** 20, int(np.ceil(budget / 2 ** 20))))
    _check_every_slot('draw_batch chunks %s' % name, ctx, arrs, ts, _restated(name, ts.size, scales), g.p, g.q)
    assert ctx.option('batch_chunk') == chunk
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 5. a failed pivot in the middle
@pytest.mark.parametrize('name', ['a', 'd'])
def test_a_failed_pivot_in_the_middle_of_a_batch(name):
    """tests/test_grad_batch_gpu.py's construction: a NaN jitter in vector 2, so no pivot of its B is positive -- a numerical
    verdict, not a device fault."""
    pr, mask, order, mu0, var0 = VB._problem(name)
    g = VB._model(name)
    bad = [x.copy() for x in VB._sets(g, STOP_SCALES)]
    bad[2][-1] = np.nan
    ts = VB._times(name, 129)
    ctx, *arrs = VB._inputs(g, bad, (mu0, var0))
    refs = list(_restated(name, ts.size, STOP_SCALES))
    refs[2] = None
    _check_every_slot('draw_batch failed pivot %s' % name, ctx, arrs, ts, refs, g.p, g.q)
    kp, yr, jt, m0, v0 = arrs
    z = np.random.default_rng(5).standard_normal((5, g.q * (g.p + 1), 3, ts.size))
    got = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, 1, ts, z, forced=True)
    assert got[3][2] > 0 and np.isnan(got[0][2])
    assert np.all(np.isnan(got[6][2])) and np.all(np.isnan(got[7][2]))
    keep = [0, 1, 3, 4]
    assert not got[3][keep].any() and not got[9][keep].any()
    assert np.all(np.isfinite(got[6][keep])) and np.all(np.isfinite(got[7][keep])) and _in_range(got[8][keep])
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 6. the ladder per slot
def _unmasked_a():
    """Case (a) without its mask: the model, the initial state."""
    pr = VB._problem('a')[0]
    mu0, var0 = (np.asarray(a, dtype=float) for a in V.init_state(pr, None))
    y, e = pr['y_raw'], np.sqrt(pr['yerr2'])
    g = gpyrn.inference(len(pr['nodes']), pr['time'], *[a for i in range(y.shape[0]) for a in (y[i], e[i])])
    g.set_components(*copy.deepcopy((list(pr['nodes']), list(pr['weights']), list(pr['means']), list(pr['jitters']))))
    return pr, g, mu0, var0


def test_the_ladder_per_slot():
    """Every entry of t* three times: C* is singular by construction (a handled verdict, not a fault;
    test_duplicated_times_raise_the_nugget does the same one by one).  Case (a) without its mask, B = 2.

    Which two vectors is the test's to choose, and the choice follows from the number format, as in the one-by-one test.  With
    a time given three times the pivots of its second and third copy in C* + nu I are about 2 nu and 1.5 nu, whatever the
    entry a = C*[t, t] is; they are formed as differences of numbers of size a, so fp64 loses them once eps a = 1.1e-16 a
    reaches nu.  The first rung, nu = 1.25e-12, therefore factors for a << 1e4 and fails for a >> 1e4.  Vector 0 is the
    fixture's at 1.01 (entries below 1): all of its slots must stay on the first rung.  Vector 1 has the amplitude of the
    plain node (node 1, QuasiPeriodic; the composite node 0 keeps its children's parameters) times 1e3 -- prior variance 1e6
    away from the data, the one-by-one test's amplitude: that slot must climb, its five neighbours must not.  Both run in the
    same launches: only the failed slot is factored again.  The call behind it, on ordinary times and the fixture's vectors
    (the checker's bounds are those of well-conditioned problems), passes test 1: the task lists and flag words the ladder
    left at its own geometry are rebuilt."""
    pr, g, mu0, var0 = _unmasked_a()
    sets = VB._sets(g, SCALES[:2])
    loud = [sets[0], sets[1].copy()]
    loud[1][g.nodes[0].pars.size] *= 1e3
    ctx, kp, yr, jt, m0, v0 = VB._inputs(g, loud, (mu0, var0))
    ts3 = np.repeat(V.mixed_times(pr['time'], 43, seed=43), 3)
    assert ts3.size == 129
    G = g.q * (g.p + 1)
    z = np.random.default_rng(11).standard_normal((2, G, 4, ts3.size))
    res = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, 1, ts3, z, forced=True)
    nug = res[8]
    print('draw_batch ladder: nuggets', nug.tolist())
    assert not res[3].any() and not res[9].any()
    assert np.all(np.isfinite(res[6])) and np.all(np.isfinite(res[7]))
    assert _in_range(nug)
    assert nug.max() > D.NU_MIN
    assert np.all(nug[0] == D.NU_MIN) and nug[1][1] > D.NU_MIN and np.all(np.delete(nug[1], 1) == D.NU_MIN)
    # the call right behind it, on ordinary times
    ctx, kp, yr, jt, m0, v0 = VB._inputs(g, sets, (mu0, var0))
    ts = VB._times('a', 129)
    refs = _reference(pr, None, 'reference', mu0, var0, g, sets, ts)
    _check_every_slot('draw_batch behind the ladder', ctx, (kp, yr, jt, m0, v0), ts, refs, g.p, g.q)
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 7. at the data times
@pytest.mark.parametrize('name', ['a', 'c', 'f'])
def test_data_times_give_each_slots_state(name):
    """tstar = time under a mask: mean* and diag(L L^T) - nu are each slot's returned state (the imputation rows included)."""
    pr, mask, order, mu0, var0 = VB._problem(name)
    assert mask is not None and (~mask).sum() > 0
    g = VB._model(name)
    start = (2.0 * mu0, var0) if name == 'c' else (mu0, var0)
    ctx, kp, yr, jt, m0, v0 = VB._inputs(g, VB._sets(g), start)
    ts = np.asarray(g.time, dtype=float)
    ns, G, B = ts.size, g.q * (g.p + 1), kp.shape[0]
    r0 = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, MAX_ITER, ts, np.zeros((B, G, 1, ns)), outputs=False)
    rI = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, MAX_ITER, ts, np.broadcast_to(np.eye(ns), (B, G, ns, ns)).copy(),
                                  outputs=False)
    assert not r0[3].any() and not r0[9].any() and np.array_equal(r0[8], rI[8])
    for b in range(B):
        mean = r0[6][b][:, 0, :]
        var = np.array([(((rI[6][b][gi] - mean[gi][None, :]).T) ** 2).sum(axis=1) - r0[8][b][gi] for gi in range(G)])
        _cases.assert_state('draw_batch at the data times %s slot %d (%d trips)' % (name, b, r0[1][b]), mean,
                            VB._rows(r0[4][b], g.p, g.q), var, VB._rows(r0[5][b], g.p, g.q), tol=TOL)
    print('draw_batch data times %s: trips %s' % (name, r0[1].tolist()))
    assert ctx.option('fallbacks') == 0


# ------------------------------------------------------------------ 8. moments
def test_draw_moments_match_the_prediction():
    name, n = 'a', 20000
    pr, mask, order, mu0, var0 = VB._problem(name)
    g, g2 = VB._model(name, predict='variational'), VB._model(name, predict='variational')
    sets = VB._sets(g, SCALES[:2])
    ts = VB._times(name, 37)
    mean, var = g.predict_batch(sets, tstar=ts, from_sweeps=True, sweeps=2, start=(mu0, var0))
    draws = g2.sample_posterior_batch(sets, tstar=ts, n=n, noise=True, rng=SEED, sweeps=2, start=(mu0, var0))
    assert draws.shape == (2, n, ts.size, g.p) and np.all(np.isfinite(draws)) and g2.last_info == 0
    assert g2.last_nuggets.shape == (2, g.q * (g.p + 1)) and _in_range(g2.last_nuggets)
    for b in range(2):
        m = draws[b].mean(axis=0)
        c = draws[b] - m
        s2, m4 = (c ** 2).mean(axis=0), (c ** 4).mean(axis=0)
        zm = np.abs(m - mean[b]) / np.sqrt(var[b] / n)
        zv = np.abs(s2 * n / (n - 1) - var[b]) / np.sqrt((m4 - s2 ** 2) / n)   # (the fourth moment of the draws)
        print('draw_batch moments vector %d: worst mean %.2f SE, worst variance %.2f SE' % (b, zm.max(), zv.max()))
        assert zm.max() < 5 and zv.max() < 5
    assert g2._backend().option('fallbacks') == 0


# ------------------------------------------------------------------ 9. Python
class _Fixed(np.random.Generator):
    """A generator whose standard normals are zeros: the draws are then each vector's mean function + sum_j w o f of mean*."""
    def __init__(self):
        super().__init__(np.random.PCG64(0))

    def standard_normal(self, size=None, *a, **kw):
        return np.zeros(size)


def test_python_side_by_side_and_one_by_one_agree():
    g, g1 = VB._series_model(), VB._series_model()
    g1.batch_max_N = 0                                        # (N above batch_max_N: the one-by-one branch)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * s for s in SCALES]
    ts = V.mixed_times(g.time, 129, seed=2)
    nodes, weights, means, jitters = g._get_components()
    start = g._initMuVar(nodes, weights, jitters)
    G = g.q * (g.p + 1)
    a, la = g.sample_posterior_batch(sets, tstar=ts, n=1, rng=_Fixed(), separate=True, sweeps=2, start=start)
    b, lb = g1.sample_posterior_batch(sets, tstar=ts, n=1, rng=_Fixed(), separate=True, sweeps=2, start=start)
    assert a.shape == (4, 1, 129, g.p) and la.shape == (4, G, 1, 129) and g.last_info == 0 and g1.last_info == 0
    assert g.last_nuggets.shape == (4, G) and np.array_equal(g.last_nuggets, g1.last_nuggets)
    for k in range(len(sets)):
        _cases.assert_state('draw_batch python, z = 0, vector %d' % k, la[k][:, 0], lb[k][:, 0], tol=DRAW_TOL)
        _cases.assert_state('draw_batch python, z = 0, outputs of vector %d' % k, a[k][0].T, b[k][0].T, tol=DRAW_TOL)
    # the same generator on both routes: the same normals, consumed in the same order (noise behind them)
    c = g.sample_posterior_batch(sets, tstar=ts, n=3, rng=5, noise=True, sweeps=2, start=start)
    d = g1.sample_posterior_batch(sets, tstar=ts, n=3, rng=5, noise=True, sweeps=2, start=start)
    assert c.shape == d.shape == (4, 3, 129, g.p) and np.all(np.isfinite(c)) and np.all(np.isfinite(d))
    assert np.array_equal(g.last_nuggets, g1.last_nuggets)
    # (no forward comparison of c and d: two factors of matrices that are singular to rounding)
    np.testing.assert_allclose(g.get_parameters(), sets[-1])
    np.testing.assert_allclose(g1.get_parameters(), sets[-1])
    assert g._backend().option('fallbacks') == 0 and g1._backend().option('fallbacks') == 0


def _rv_model(device_means):
    r = np.random.RandomState(145)
    t = np.sort(r.uniform(0.0, 60.0, 45))
    y = 0.3 * r.randn(2, 45)
    y[0] += meanfunc.Keplerian(11.3, 3.7, 0.4, 0.8, 2.1)(t)
    e = 0.1 + 0.1 * r.rand(2, 45)
    g = gpyrn.inference(1, t, y[0], e[0], y[1], e[1], device_means=device_means, predict='variational')
    g.set_components([covfunc.SquaredExponential(1.0, 7.0)], [covfunc.SquaredExponential(0.5, 15.0), covfunc.SquaredExponential(0.5, 16.0)],
                     [meanfunc.Keplerian(11.0, 3.5, 0.35, 0.7, 2.0) + meanfunc.Constant(0.1), meanfunc.Linear(0.001, 0.05)], [0.2, 0.2])
    return g


@pytest.mark.parametrize('device_means', [False, True])
def test_python_adds_the_mean_functions_per_vector(device_means):
    """A Linear + Keplerian model, three vectors with their own mean parameters: with z = 0 what each output carries on top of
    sum_j f_j w_ji -- rebuilt from the latent rows of the same call -- is that vector's own mean function at t*."""
    g = _rv_model(device_means)
    x0 = np.array(g.get_parameters(), dtype=float)
    r = np.random.RandomState(8)
    sets = [x0 * (1 + 0.02 * r.uniform(-1, 1, x0.size)) for _ in range(3)]
    ts = V.mixed_times(g.time, 129, seed=4)
    draws, lat = g.sample_posterior_batch(sets, tstar=ts, n=2, rng=_Fixed(), separate=True, max_iter=40)
    assert draws.shape == (3, 2, 129, 2) and lat.shape == (3, 3, 2, 129) and g.last_info == 0
    q, p = g.q, g.p
    for b, x in enumerate(sets):
        g.set_parameters(x)
        mv = np.array(np.array_split(g._mean(g._get_components()[2], ts), p))     # (the host's evaluation)
        for i in range(p):
            fit = sum(lat[b][j, 0] * lat[b][q + j * p + i, 0] for j in range(q))
            scale = max(1.0, np.abs(fit).max(), np.abs(mv[i]).max())
            # (the host's evaluation against itself: rounding; against the device's Kepler solver: the project's 1e-8)
            assert np.abs(draws[b][0][:, i] - fit - mv[i]).max() <= (1e-8 if device_means else 1e-13) * scale
    assert not np.array_equal(draws[0], draws[1])
    assert g._backend().option('fallbacks') == 0


def test_posterior_predictive_with_draws_and_the_refusals():
    g = VB._series_model()
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * s for s in SCALES]
    ts = V.mixed_times(g.time, 129, seed=1)
    mean, var, curves = g.posterior_predictive(sets, tstar=ts, draws=3, rng=2, max_iter=60)
    assert mean.shape == (129, g.p) and var.shape == mean.shape and curves.shape == (4 * 3, 129, g.p)
    assert np.all(np.isfinite(curves)) and g.last_info == 0
    g2 = VB._series_model()
    m2, v2 = g2.posterior_predictive(sets, tstar=ts, from_sweeps=True, max_iter=60)      # (without draws: unchanged)
    np.testing.assert_array_equal(m2, mean)
    np.testing.assert_array_equal(v2, var)
    # the curves scatter around the mixture's mean by about its standard deviation
    assert np.abs(curves - mean[None]).max() <= 8 * np.sqrt(var.max()) + np.abs(mean).max()
    with pytest.raises(ValueError, match='resample'):
        g.posterior_predictive(sets, tstar=ts, draws=3, weights=[1.0, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError, match='go with `draws`'):
        g.posterior_predictive(sets, tstar=ts, from_sweeps=True, rng=2)
    _, _, one = g.posterior_predictive(sets, tstar=ts, draws=1, weights=[2.0, 2.0, 2.0, 2.0], max_iter=60)   # (uniform: passes)
    assert one.shape == (4, 129, g.p)
    assert g._backend().option('fallbacks') == 0
    g._comm = object()                                        # (what a sharded object holds: any communicator)
    with pytest.raises(NotImplementedError, match='sharded'):
        g.sample_posterior_batch(sets, tstar=ts)


# ------------------------------------------------------------------ 10. contract
def _raw_call(ctx, kp, yr, jt, m0, v0, max_iter, ts, nd=2, flags=0, latent=True, outputs=True, ns=None, z=True, n_draws=None,
              nugget=True, dinfo=True):
    B, G, p = kp.shape[0], ctx.G, ctx.p
    dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    arrs = [np.ascontiguousarray(a, dtype=float) for a in (kp, yr, jt, m0, v0, ts)]
    elbo = np.zeros(B)
    it, cv, info = (np.zeros(B, dtype=np.int32) for _ in range(3))
    zz = np.zeros((B, G, nd, ts.size)) if z else None
    lat = np.zeros((B, G, nd, ts.size)) if latent else None
    out = np.zeros((B, p, nd, ts.size)) if outputs else None
    nug = np.zeros((B, G)) if nugget else None
    di = np.zeros(B, dtype=np.int32) if dinfo else None
    return ctx._lib.gprn_elbocalc_batch_draws(ctx._h, B, dp(arrs[0]), kp.shape[1], dp(arrs[1]), dp(arrs[2]), dp(arrs[3]),
                                              dp(arrs[4]), max_iter, flags, ts.size if ns is None else ns, dp(arrs[5]),
                                              nd if n_draws is None else n_draws, dp(zz), dp(elbo), ip(it), ip(cv), ip(info),
                                              None, None, dp(lat), dp(out), dp(nug), ip(di))


def test_refusals_and_argument_errors():
    name = 'a'
    pr, mask, order, mu0, var0 = VB._problem(name)
    g = VB._model(name)
    ctx, kp, yr, jt, m0, v0 = VB._inputs(g, VB._sets(g), (mu0, var0))
    ts = VB._times(name, 129)
    lib = ctx._lib
    E_ARG, E_UNS = _hip.GPRN_E_ARG, _hip.GPRN_E_UNSUPPORTED
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == 0
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 0, ts) == E_ARG                            # no sweep is committed
    assert b'committed sweep' in lib.gprn_last_error(ctx._h)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, ns=0) == E_ARG
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, n_draws=0) == E_ARG
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, z=False) == E_ARG
    assert b'normals' in lib.gprn_last_error(ctx._h)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, latent=False, outputs=False) == E_ARG
    assert b'neither' in lib.gprn_last_error(ctx._h)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, flags=2) == E_ARG                   # an unknown flag
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, nugget=False) == E_ARG
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, dinfo=False) == E_ARG
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, flags=_hip.GPRN_BATCH_FORCED, outputs=False) == 0
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts, flags=_hip.GPRN_BATCH_FORCED, latent=False) == 0
    ctx.option('predict_form', _hip.PREDICT_REFERENCE)                                  # always the posterior form
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == 0
    ctx.option('batch_mask', 0)                                                          # a mask without "batch_mask"
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == E_UNS
    assert b'mask' in lib.gprn_last_error(ctx._h)
    ctx.option('batch_mask', 1)
    ctx.option('small_path', 0)                                                          # one tile, the small path off
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == E_UNS
    assert b'small path' in lib.gprn_last_error(ctx._h)
    G = g.q * (g.p + 1)
    assert ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, 2, ts, np.zeros((4, G, 1, ts.size))) is None
    ctx.option('small_path', 1)
    assert _raw_call(ctx, kp, yr, jt, m0, v0, 2, ts) == 0
    assert ctx.option('fallbacks') == 0
