"""The celerite kernels on the device (ids GPRN_K_SHO, GPRN_K_ROTATION, GPRN_K_CELERITE) from the element code up:

1. the symmetric fill against tests/golden/celerite_highprec (mpmath at 40 digits) at the bound of tests/_fill_fixture.py,
   its own instantiation against the generic program, symmetry, NaN;
2. prediction's rectangular fills, both forms, single and batched launches, ns = 130 against N = 129;
3. the exact parameter derivatives: gprn_eval_kernel_grad at 2e-11 of max |d_ref|; gprn_grad_kernel and gprn_grad_elbo on a
   p = 2, q = 2 model (tests/_celerite_model.py) against the contraction of the NumPy closed forms;
4. that model end to end at N = 45 (one tile) and N = 150 (the launch path): forced sweeps and ELBOcalc against
   oracle.cpu_ref at 1e-8, nELBO_batch slot by slot, predict='variational' at the data times, and the bound form's gradient
   batch against tests/_bound_ref.py.

Every test prints its figures before it asserts."""
import functools
import os

import numpy as np
import pytest

from gpyrn_amd import _hip, covfunc
from oracle import cpu_ref
from tests import _bound_ref as BR
from tests import _cases
from tests import _celerite_fixture as cx
from tests import _celerite_model as cm
from tests import _fill_fixture as ff
from tests import _grad_ref as GR

pytestmark = pytest.mark.gpu
RTOL = 1e-8                                                         # the project's, tests/test_parity_gpu.py
GRAD_TOL_CLOSED, GRAD_TOL_FD, GRAD_NOISE = 1e-12, 1e-7, 8.0       # include/gprn_hip.h, gprn_grad_kernel
N_RECT, NS = 129, 130
FORMS = (ff.REF, ff.POST)


def _ctx(t):
    ctx = _hip.Context(0)
    ctx.set_data(t, np.zeros((1, t.size)), np.ones((1, t.size)), 1)
    return ctx


def _assert_default_schedule(ctx):
    assert ctx.option('fallbacks') == 0
    if os.environ.get('GPRN_FLAGS', '1') != '0' and not os.environ.get('ROCPROF_COUNTER_COLLECTION'):
        assert ctx.option('flags') == 1


def _show(fails):
    return '\n'.join(fails[:25]) + ('\n... %d in all' % len(fails) if len(fails) > 25 else '')


# ------------------------------------------------------------------ 1. the fill
@pytest.fixture(scope='module')
def filled():
    """(meta, square arrays, {case: K without nugget}, one context per time set: 200, 200 and 120 points)"""
    meta, d, _ = cx.load()
    ctxs = {reg: _ctx(d['t_' + reg]) for reg in ('R1', 'R2', 'R3')}
    Ks = {c['name']: ctxs[c['tset']].eval_kernel(c['ops'], c['pars'], 0.0) for c in meta['cases']}
    yield meta, d, Ks, ctxs
    for ctx in ctxs.values():
        ctx.close()


def test_fill_within_the_bound(filled):
    """|K - K_ref| <= (4 + 2 kappa) 2^-53 |K_ref| + the denormal floor at every sampled element, NaN where the reference is"""
    meta, d, Ks, _ = filled
    fails, ratios = [], {}
    for c in meta['cases']:
        r = []
        v = ff.violations(Ks[c['name']], c, d, ratios=r)
        ratios[c['kernel']] = max(ratios.get(c['kernel'], 0.0), r[0])
        if v:
            fails.append('%s: %d elements off, e.g. K[%d,%d] = %r, reference %r, allowed %.3g' % (c['name'], len(v), *v[0]))
        if '_nan_' in c['name'] and not np.isnan(Ks[c['name']]).all():
            fails.append('%s: a NaN parameter left finite elements' % c['name'])
        if '_underflow_' in c['name']:
            K = Ks[c['name']]
            if not (np.isfinite(K).all() and (K[~np.eye(K.shape[0], dtype=bool)] == 0).all()):
                fails.append('%s: the deep tail is not 0' % c['name'])
    print('\n' + '\n'.join('celerite_fill_accuracy %-14s worst error / allowed %.3f' % kv for kv in sorted(ratios.items())))
    assert not fails, _show(fails)


def test_fill_is_symmetric_and_the_nugget_is_on_the_diagonal(filled):
    meta, d, Ks, ctxs = filled
    for c in meta['cases']:
        K = Ks[c['name']]
        assert np.array_equal(K, K.T, equal_nan=True), c['name']
    c = next(c for c in meta['cases'] if c['name'] == 'SHO_typical_4')
    Kn = ctxs['R1'].eval_kernel(c['ops'], c['pars'], 1e-6)
    K = Ks[c['name']]
    assert np.array_equal(Kn - np.diag(np.diag(Kn)), K - np.diag(np.diag(K))) and np.array_equal(np.diag(Kn), np.diag(K) + 1e-6)


def test_own_instantiation_equals_the_generic_program(filled):
    """k_fill_sym<24 .. 26> against k_fill_sym<-1> on k * Constant(1.0): the same bits, every one-kernel case"""
    meta, d, Ks, ctxs = filled
    kids = set()
    for c in meta['cases']:
        if len(c['ops']) != 1:
            continue
        kids.add(c['ops'][0][1])
        ops = c['ops'] + [[0, 0, len(c['pars'])], [2, 0, 0]]
        K = ctxs[c['tset']].eval_kernel(ops, list(c['pars']) + [1.0], 0.0)
        assert np.array_equal(K, Ks[c['name']], equal_nan=True), c['name']
    assert kids == {24, 25, 26}


# ------------------------------------------------------------------ 2. the rectangular fills
def _s_pow2(n):
    """s of the posterior form as exact powers of two, zero on a tenth of the rows (none a coincident column)"""
    k = np.arange(n)
    return np.where(k % 10 == 6, 0.0, np.array([0.25, 0.5, 1.0, 2.0])[k % 4])


@pytest.fixture(scope='module')
def rect():
    meta, _, rd = cx.load()
    ctxs = {reg: _ctx(rd['t_' + reg]) for reg in ('R1', 'R2', 'R3')}
    yield meta, rd, ctxs
    assert all(ctx.option('fallbacks') == 0 for ctx in ctxs.values())
    for ctx in ctxs.values():
        ctx.close()


def test_rectangular_fills_meet_the_bound_single_and_batched(rect):
    """gprn_test_fill_rect, every case: K* at the sample and all of k** within the value bound in the reference form and in
    the posterior form (K* diag(s), s powers of two and zeros; the nugget and WhiteNoise exactly where t*_i == t_n, in k**
    always); the batched launches return the single launch's bits from either slot; the padding is 0."""
    meta, rd, ctxs = rect
    s = _s_pow2(N_RECT)
    fails = []
    for c in meta['cases']:
        rc = cx.rect_case(c)
        ts = rd['ts_' + c['tset']]
        assert ts.size == NS and rd['t_' + c['tset']].size == N_RECT
        for form in FORMS:
            def fill(batched):
                return ctxs[c['tset']].test_fill_rect(c['ops'], c['pars'], ff.rect_nugget(meta, rc, form), ts, form=form,
                                                      batched=batched, s=s if form == ff.POST else None)
            Ks, kss = fill(0)
            assert Ks.shape == (256, 256) and kss.shape == (256,)
            vk, vs = ff.rect_views(rc, rd, form, NS)
            if form == ff.POST:
                vk = ff.scale_columns(vk, s)
            for what, K, (cc, dd) in (('K*', Ks, vk), ('k**', kss[:, None], vs)):
                v = ff.violations(K, cc, dd)
                if v:
                    fails.append('%s form %d %s: %d elements off, e.g. [%d,%d] = %r, reference %r, allowed %.3g'
                                 % (c['name'], form, what, len(v), *v[0]))
            if not (np.all(Ks[NS:] == 0.0) and np.all(Ks[:NS, N_RECT:] == 0.0) and np.isnan(kss[NS:]).all()):
                fails.append('%s form %d: the padding is written' % (c['name'], form))
            for slot in (1, 2):
                for what, a, b in zip(('K*', 'k**'), fill(slot), (Ks, kss)):
                    if not np.array_equal(a, b, equal_nan=True):
                        fails.append('%s form %d slot %d %s: differs from the single launch' % (c['name'], form, slot - 1, what))
    assert not fails, _show(fails)


def test_rectangular_instantiations_equal_the_generic_program(rect):
    meta, rd, ctxs = rect
    s = _s_pow2(N_RECT)
    for c in meta['cases']:
        if len(c['ops']) != 1:
            continue
        ops, pars = c['ops'] + [[0, 0, len(c['pars'])], [2, 0, 0]], list(c['pars']) + [1.0]
        for form in FORMS:
            kw = dict(form=form, s=s if form == ff.POST else None)
            nug = ff.rect_nugget(meta, cx.rect_case(c), form)
            own = ctxs[c['tset']].test_fill_rect(c['ops'], c['pars'], nug, rd['ts_' + c['tset']], **kw)
            gen = ctxs[c['tset']].test_fill_rect(ops, pars, nug, rd['ts_' + c['tset']], **kw)
            for what, a, b in zip(('K*', 'k**'), own, gen):
                assert np.array_equal(a, b, equal_nan=True), (c['name'], form, what)


def test_predictions_own_fills_single_and_batched(rect):
    """gprn_test_predict_fill on a q = 2, p = 1 model whose four latent GPs carry fixture cases (SHO, Rotation, CeleriteTerm,
    Rotation + CeleriteTerm) at the fixture's 129 data and 130 prediction times: K* and k** of evaluation 0 within the value
    bound (the reference form), the batched fills the bits of the single ones for both evaluations."""
    import gpyrn_amd as gpyrn
    from gpyrn_amd import meanfunc
    meta, rd, _ = rect
    names = ['SHO_typical_4', 'Rotation_typical_0', 'CeleriteTerm_typical_0', 'Rotation_plus_Celerite_0']
    cases = [next(c for c in meta['cases'] if c['name'] == n) for n in names]
    t, ts = rd['t_R1'], rd['ts_R1']
    g = gpyrn.inference(2, t, np.sin(t / 5.0), np.full(t.size, 0.2))
    ks = [cx.kernel_of(c) for c in cases]
    g.set_components(ks[:2], ks[2:], [meanfunc.Constant(0.0)], [0.3])
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0, x0 * 1.02]
    ctx, kp, jt, _ = g._predict_stage([x.copy() for x in sets], ts)
    var = np.full((2, (g.p + 1) * g.q * g.N), 0.05)
    fails = []
    for e in range(2):
        for gp, c in enumerate(cases):
            single = ctx.test_predict_fill(kp, var, e, gp, ts, batched=False)
            batched = ctx.test_predict_fill(kp, var, e, gp, ts, batched=True)
            for what, a, b in zip(('K + diag v', 'K*', 'k**'), batched, single):
                assert np.all(np.isfinite(b)), (c['name'], what)
                if not np.array_equal(a, b):
                    fails.append('%s evaluation %d %s: batched differs from single' % (c['name'], e, what))
            if e == 0:
                vk, vs = ff.rect_views(cx.rect_case(c), rd, ff.REF, NS)
                for what, K, (cc, dd) in (('K*', single[1], vk), ('k**', single[2][:, None], vs)):
                    v = ff.violations(K, cc, dd)
                    if v:
                        fails.append('%s %s: %d elements off, e.g. [%d,%d] = %r, reference %r, allowed %.3g'
                                     % (c['name'], what, len(v), *v[0]))
    assert ctx.option('fallbacks') == 0
    assert not fails, _show(fails)


# ------------------------------------------------------------------ 3. exact derivatives
def test_eval_kernel_grad_meets_the_bound(filled):
    """k_fill_grad over every case: 2e-11 of max |d_ref| per parameter, dK = dK^T to the bit, finite on the diagonal; with a
    NaN parameter NaN wherever the value is."""
    meta, d, Ks, ctxs = filled
    fails, worst = [], {}
    for c in meta['cases']:
        dK = ctxs[c['tset']].eval_kernel_grad(c['ops'], c['pars'])
        N = dK.shape[1]
        if cx.has_nan(c):
            if not np.isnan(dK).any(axis=0).all():
                fails.append('%s: a NaN parameter left finite derivatives' % c['name'])
            continue
        if c['dk_off'] is None:                         # (dropped from the derivative bound: finite and symmetric all the same)
            if not (np.isfinite(dK).all() and np.array_equal(dK, dK.transpose(0, 2, 1))):
                fails.append('%s: not finite or not symmetric' % c['name'])
            continue
        w = cx.dk_worst(dK, c, d)
        worst[c['kernel']] = max(worst.get(c['kernel'], 0.0), w)
        if not w <= cx.DK_TOL:
            fails.append('%s: off by %.2e of max |ref|' % (c['name'], w))
        if not np.array_equal(dK, dK.transpose(0, 2, 1)):
            fails.append('%s: not symmetric to the bit' % c['name'])
        if not np.isfinite(dK[:, np.arange(N), np.arange(N)]).all():
            fails.append('%s: not finite on the diagonal' % c['name'])
    print('\n' + '\n'.join('celerite_eval_kernel_grad %-14s worst %.2e of max |ref|' % kv for kv in sorted(worst.items())))
    assert not fails, _show(fails)


def _swept(N, keep_sigma=False, **kw):
    g, t = cm.inference(N, **kw)
    nd, wt, mn, jt = g._get_components()
    ctx = g._setup_device(nd, wt, mn, jt)
    assert g.last_info == 0
    mu0, var0 = g._initMuVar(nd, wt, jt)
    ctx.set_muvar(np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float))
    if keep_sigma:
        ctx.keep_sigma(True)
    _, _, info = ctx.sweep(1, commit=True)
    assert info == 0
    return g, ctx, t, list(nd) + list(wt)


def _check_entries(what, k, on, off, G, t, fails):
    """one kernel's entries: option on against sum G dK of the NumPy closed forms in the norm sum |G| |dK| at 1e-12; option
    off within the differences' documented accuracy of option on (SquaredExponential: a closed form, the same bits)"""
    r = t[:, None] - t[None, :]
    dks = cm.dk(k, t)
    GK = float(np.sum(np.abs(G) * np.abs(k(r))))
    for l, dk in enumerate(dks):
        ref, scale = float(np.sum(G * dk)), float(np.sum(np.abs(G) * np.abs(dk)))
        e = abs(on[l] - ref) / scale
        print('%s %-45s parameter %d: exact %.2e of sum |G||dK|, differences %.2e' % (what, str(k)[:45], l, e, abs(off[l] - ref) / scale))
        if not e <= GRAD_TOL_CLOSED:
            fails.append('%s %s parameter %d: device %.15g, NumPy %.15g, off by %.2e of sum |G||dK|' % (what, k, l, on[l], ref, e))
        if isinstance(k, covfunc.SquaredExponential):
            if on[l] != off[l]:
                fails.append('%s %s parameter %d: a closed form moved with the option' % (what, k, l))
        else:
            noise = GRAD_NOISE * 2.0 ** -53 * GK / (1e-6 * max(1.0, abs(k.pars[l])))
            if not abs(on[l] - off[l]) <= (GRAD_TOL_FD + GRAD_TOL_CLOSED) * scale + noise:
                fails.append('%s %s parameter %d: exact %.15g and differences %.15g apart' % (what, k, l, on[l], off[l]))


def test_grad_kernel_exact_and_by_differences():
    """gprn_grad_kernel at N = 130 (two 64-blocks and a ragged third), every latent GP of the model"""
    g, ctx, t, kernels = _swept(130, keep_sigma=True)
    try:
        mu, _ = ctx.get_muvar()
        m_w = mu[1:].reshape(g.q, g.p, g.N)
        ms = [mu[0, gp] if gp < g.q else m_w[divmod(gp - g.q, g.p)] for gp in range(g.q + g.q * g.p)]
        off = [ctx.grad_kernel(gp, ms[gp], k.pars.size) for gp, k in enumerate(kernels)]
        assert ctx.option('grad_exact', 1) == 0
        fails = []
        for gp, k in enumerate(kernels):
            on = ctx.grad_kernel(gp, ms[gp], k.pars.size)
            Kinv, Pm = ctx.grad_matrices(gp)
            a = Kinv @ ms[gp]
            _check_entries('grad_kernel', k, on, off[gp], 0.5 * (Pm - Kinv + np.outer(a, a)), t, fails)
        _assert_default_schedule(ctx)
    finally:
        ctx.keep_sigma(False)
    assert not fails, '\n'.join(fails)


def test_grad_elbo_exact_and_by_differences():
    """gprn_grad_elbo (k_grad_contract_b) at N = 130, one call for all six kernels"""
    g, ctx, t, kernels = _swept(130)
    n_k = sum(k.pars.size for k in kernels)
    off = ctx.grad_elbo(n_k)
    assert ctx.option('grad_exact', 1) == 0
    on = ctx.grad_elbo(n_k)
    assert np.array_equal(on, ctx.grad_elbo(n_k)) and np.all(np.isfinite(on))
    fails, pos = [], 0
    for gp, k in enumerate(kernels):
        n = k.pars.size
        _check_entries('grad_elbo', k, on[pos:pos + n], off[pos:pos + n], ctx.grad_matrix(gp), t, fails)
        pos += n
    assert ctx.option('grad_exact', 0) == 1
    assert np.array_equal(off, ctx.grad_elbo(n_k))
    _assert_default_schedule(ctx)
    assert not fails, '\n'.join(fails)


# ------------------------------------------------------------------ 4. end to end
SIZES = [45, 150]                       # one tile; two tiles, the launch path


@functools.lru_cache(maxsize=None)
def _reference(N):
    """oracle.cpu_ref on the model, computed once per size and left alone: three sweeps and the ELBOcalc loop"""
    pr = cm.problem(N)
    mu, var = pr['mu0'], pr['var0']
    E, parts = [], []
    for _ in range(3):
        e, mu, var, pt = cpu_ref.sweep_ref(*pr['args'], mu, var)
        E.append(e)
        parts.append(pt)
    calc = cpu_ref.elbo_calc(*pr['args'], pr['mu0'], pr['var0'])
    out = dict(pr=pr, E=np.array(E), parts=np.array(parts), mu3=mu, var3=var, calc=calc)
    for a in (out['E'], out['parts'], mu, var) + tuple(x for x in calc if isinstance(x, np.ndarray)):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('N', SIZES)
def test_forced_sweeps_and_elbocalc_match_the_oracle(N):
    ref = _reference(N)
    g, t = cm.inference(N)
    mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
    np.testing.assert_allclose(np.ravel(mu0), np.ravel(ref['pr']['mu0']), rtol=1e-13)
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    assert g.last_info == 0
    ctx.set_muvar(mu0, var0)
    elbo, parts, info = ctx.sweep(3, commit=True)
    assert info == 0
    print('celerite N %d forced sweeps: ELBO rel %.2e, parts rel %.2e' % (N, np.abs(elbo / ref['E'] - 1).max(),
                                                                           np.abs(parts / ref['parts'] - 1).max()))
    np.testing.assert_allclose(elbo, ref['E'], rtol=RTOL)
    np.testing.assert_allclose(parts, ref['parts'], rtol=RTOL)
    mu, var = ctx.get_muvar()
    _cases.assert_state('celerite forced sweeps N %d' % N, mu, ref['mu3'], var, ref['var3'])
    E_ref, mu_ref, var_ref, it_ref, hist_ref = ref['calc']
    E, mu, var, it = g.ELBOcalc()
    print('celerite N %d ELBOcalc: %d trips (oracle %d), ELBO rel %.2e' % (N, it, it_ref, abs(E / E_ref - 1)))
    assert g.last_info == 0 and it == it_ref
    np.testing.assert_allclose(g._elbo_history, hist_ref, rtol=RTOL)
    np.testing.assert_allclose(E, E_ref, rtol=RTOL)
    _cases.assert_state('celerite ELBOcalc N %d' % N, mu, mu_ref, var, var_ref)
    _assert_default_schedule(g._backend())


@pytest.mark.parametrize('N', SIZES)
def test_nelbo_batch_slot_by_slot(N, capsys):
    """B = 5 vectors 1 % around the model's, side by side against one by one, each from its own starting state"""
    g, _ = cm.inference(N)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(11)
    sets = [x0 * (1.0 + 0.01 * rng.standard_normal(x0.size)) for _ in range(5)]
    capsys.readouterr()
    got = np.array(g.nELBO_batch(sets))
    assert 'evaluations side by side' in capsys.readouterr().out, 'the list was evaluated one by one: no batched form?'
    assert g.last_info == 0 and np.all(np.isfinite(got))
    gs, _ = cm.inference(N)
    want = []
    for x in sets:
        gs.set_parameters(x)
        want.append(-gs.ELBOcalc()[0])
    print('celerite N %d nELBO_batch rel %.2e' % (N, np.abs(got / np.array(want) - 1).max()))
    np.testing.assert_allclose(got, want, rtol=1e-9)
    _assert_default_schedule(g._backend())


@pytest.mark.parametrize('N', SIZES)
def test_variational_prediction_at_the_data_times_returns_the_state(N):
    g, ctx, t, _ = _swept(N, predict='variational')
    assert ctx.option('predict_form') == _hip.PREDICT_POSTERIOR and ctx.option('state_ready') == 1
    mu, var = ctx.get_muvar()
    gm, gv, info = ctx.predict(t)
    assert info == 0
    rows = lambda s: np.array([s[0, j] for j in range(g.q)] + [s[1 + i, j] for j in range(g.q) for i in range(g.p)])   # noqa: E731
    _cases.assert_state('celerite varpred at the data times N %d' % N, gm, rows(mu), gv, rows(var), tol=1e-11)
    _assert_default_schedule(ctx)


def _parent_bound(N):
    """The reference form's one-call gradient against its own restatement (tests/_grad_ref.py) on the same model from the same
    state, in the norm sum |G| |dK|: the second term of tests/test_elbo_bound_gpu.py's rule -- nothing the bound form returned"""
    pr = cm.problem(N)
    st = GR.sweep_state(pr, pr['mu0'], pr['var0'], None)
    G = GR.G_matrices(pr, st, 'chol')
    ref, norm = [], []
    for Gg, k in zip(G, list(pr['nodes']) + list(pr['weights'])):
        for dk in cm.dk(k, pr['time']):
            ref.append(np.sum(Gg * dk) / st['q'])
            norm.append(np.sum(np.abs(Gg) * np.abs(dk)) / st['q'])
    g, ctx, _, _ = _swept(N, elbo='reference', exact_derivatives=True)
    dev = ctx.grad_elbo(len(ref)) / g.q
    return float((np.abs(dev - np.array(ref)) / np.array(norm)).max())


@pytest.mark.parametrize('N', SIZES)
def test_bound_form_gradient_batch_against_the_restatement(N):
    """nELBO_and_grad_batch(elbo='bound', exact_derivatives=True), two forced sweeps, two vectors: values at 1e-8, the kernel
    entries within max(100 x the spread of the restatement's two LAPACK routes, the reference form's deviation from its own
    restatement) and within 1e-8 of sum |G| |dK|, mean and jitter entries at 1e-8 -- as kmix_N200_p2q2 is checked."""
    pr = cm.problem(N)
    mu0, var0 = pr['mu0'], pr['var0']
    g, _ = cm.inference(N, elbo='bound', exact_derivatives=True)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(5)
    sets = [x0, x0 * (1.0 + 0.01 * rng.standard_normal(x0.size))]
    values, grads = g.nELBO_and_grad_batch(sets, sweeps=2, start=(mu0, var0))
    assert g.last_info == 0
    parent = _parent_bound(N)
    for b, x in enumerate(sets):
        k = 0
        for o in list(pr['nodes']) + list(pr['weights']) + list(pr['means']):
            o.pars[:] = x[k:k + o.pars.size]
            k += o.pars.size
        pr['jitters'] = [float(v) for v in x[k:]]
        a = BR.setup_args(pr)
        _, mu_a, var_a, _ = BR.sweep(*a, mu0, var0)
        e_b, mu_b, var_b, _ = BR.sweep(*a, mu_a, var_a)
        want, norm = BR.gradient(pr, a, mu_a, var_a, mu_b, var_b, dk=cm.dk)
        want_inv, _ = BR.gradient(pr, a, mu_a, var_a, mu_b, var_b, dk=cm.dk, route='inv')
        n_k = int(np.sum(np.isfinite(norm)))
        spread = float((np.abs(want - want_inv)[:n_k] / norm[:n_k]).max())
        off = float((np.abs(-grads[b] - want)[:n_k] / norm[:n_k]).max())
        print('celerite N %d slot %d: kernel entries %.2e of sum |G||dK| (spread of the two routes %.2e, reference form %.2e), '
              'the others rel %.2e' % (N, b, off, spread, parent, np.abs(-grads[b, n_k:] / want[n_k:] - 1).max()))
        np.testing.assert_allclose(values[b], -e_b, rtol=RTOL)
        assert off <= max(100.0 * spread, parent) and off <= 1e-8
        np.testing.assert_allclose(-grads[b, n_k:], want[n_k:], rtol=1e-8)
    _assert_default_schedule(g._backend())
