"""The exact parameter derivatives on the device (csrc/dk_eval.h; option "grad_exact", inference(exact_derivatives=True)):
gprn_eval_kernel_grad element by element, gprn_grad_kernel, gprn_grad_elbo and the side-by-side batch with the option on.
The reference derivative throughout is oracle.kernel_formulas.dk_dpars_longdouble (long-double Richardson, within 1e-11 of
mpmath: tests/test_fill_highprec.py); the norm of a gradient entry is tests/test_fill_gpu.py's, |dev - ref| / sum |G| |dK|.

Measured on gfx950 (every test prints its figures before it asserts).

1. gprn_eval_kernel_grad, max |dev - ref| / max |ref|, worst parameter and regime (bound 2e-11):
    Constant 4.8e-14, WhiteNoise 7.0e-14, SE 1.7e-13, Periodic 4.5e-13, QuasiPeriodic 1.1e-12, RationalQuadratic 2.2e-12,
    RQP 2.2e-12, Cosine 2.7e-13, Exponential 4.7e-13, Matern32 4.8e-13, Matern52 5.7e-13, GammaExp 6.2e-13, Piecewise 4.9e-13,
    Paciorek 7.8e-13, NewPeriodic 1.5e-12, QuasiNewPeriodic 4.6e-12, CosPeriodic 4.3e-13, QuasiCosPeriodic 1.3e-12,
    Polynomial 4.5e-12, HarmonicPeriodic 6.3e-12, QuasiHarmonicPeriodic 9.8e-12, dSE 1.4e-13, dPeriodic 6.3e-13,
    dQuasiPeriodic 1.9e-12, SE*Periodic 1.8e-12, SE+Matern32 2.8e-12, (SE*Periodic)+Matern32*(RQ+WhiteNoise) 4.8e-12,
    nested sum of six 3.5e-12.

2. gprn_grad_kernel with the option on, |dev - ref| / sum |G| |dK|: the kernels of tests/test_fill_gpu.py's list with a
   plain NumPy error above 2.5e-13.  Only the rows with device > 1e-12 are in BEYOND_THE_REFERENCE and take the last column
   as their bound; the three marked * meet 1e-12 and are held to it, as every kernel not shown (below 5e-13 everywhere).  Device and plain fp64 NumPy agree
   with each other to three digits in every row: what is left is the REFERENCE's own error -- its difference of step
   1e-6 |theta| carries 2^-64 |K| / step, which shows where K is large beside the derivative (WhiteNoise(0.3) on a diagonal
   of 20 or more: the derivative kernels) or where the decay hides a parameter (le = 0.2 at L = 0.1).
    (L, P)      kernel (+ WhiteNoise)                        device     NumPy      bound = 4 x NumPy
    (8, 11)   * QuasiCosPeriodic(0.9, 16, 11, 0.8)           9.82e-13   9.82e-13   (1e-12)
    all three   d Periodic(0.9, P, 0.8)                      5.30e-12   5.30e-12   2.12e-11
    (0.1, 11) * QuasiPeriodic(1.0, 0.2, 11, 0.7) (alone)     4.68e-13   4.68e-13   (1e-12)
    (0.1, 11)   QuasiNewPeriodic(1.1, 0.7, 0.2, 11, 0.9)     2.06e-11   2.05e-11   8.18e-11
    (0.1, 11)   CosPeriodic(1.3, 11, 0.9)                    1.21e-12   1.21e-12   4.83e-12
    (0.1, 11)   QuasiCosPeriodic(0.9, 0.2, 11, 0.8)          2.14e-11   2.14e-11   8.56e-11
    (0.1, 11)   d SquaredExponential(1.2, 0.1)               8.94e-11   8.94e-11   3.58e-10
    (0.1, 11)   d QuasiPeriodic(1.1, 0.2, 11, 0.6)           8.62e-12   8.62e-12   3.45e-11
    (0.1, 11)   SquaredExponential(1.0, 0.1) * Periodic      1.12e-12   1.12e-12   4.46e-12
    (8, 0.3)  * QuasiCosPeriodic(0.9, 16, 0.3, 0.8)          8.35e-13   8.35e-13   (1e-12)
    (8, 0.3)    d QuasiPeriodic(1.1, 16, 0.3, 0.6)           9.02e-11   9.02e-11   3.61e-10

3. gprn_grad_elbo with the option on (mixed model, N = 45 and 200, plain / masked / sequential): every kernel below 3.4e-13
   of sum |G| |dK|.   4. The batch: bit-equal at N = 45 (B = 8, one chunk) and N = 200 (B = 3, chunks of one)."""
from itertools import chain

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc
from oracle import kernel_formulas as kf
from tests import _dk_cases as dc
from tests import _dk_numpy
from tests import _mask_ref as MR
from tests.test_fill_gpu import _grad_kernels

pytestmark = pytest.mark.gpu
CLOSED = (kf.KID['SE'], kf.KID['PERIODIC'], kf.KID['QP'])
GRAD_TOL_CLOSED, GRAD_TOL_FD, GRAD_NOISE = 1e-12, 1e-7, 8.0       # include/gprn_hip.h, gprn_grad_kernel


# ------------------------------------------------------------------ 1. element by element
@pytest.fixture(scope='module')
def ctx130():
    t = dc.times(130)
    ctx = _hip.Context(0)
    ctx.set_data(t, np.zeros((1, t.size)), np.ones((1, t.size)), 1)
    yield ctx, t
    ctx.close()


@pytest.mark.parametrize('L,P', dc.REGIMES)
def test_eval_kernel_grad_against_the_long_double_derivative(ctx130, L, P):
    """N = 130: two 64-blocks and a ragged third.  Per parameter max |dev - ref| <= 2e-11 max |ref|; dK = dK^T to the bit;
    finite on the diagonal.  Every built-in id alone, the three derivative kernels, four composites."""
    ctx, t = ctx130
    eye = np.eye(t.size, dtype=bool)
    fails = []
    for name, k in dc.kernels(L, P):
        ops, pars = dc.program_of(k)
        dK = ctx.eval_kernel_grad(ops, pars)
        assert dK.shape == (pars.size, t.size, t.size)
        w = dc.worst(dK, dc.reference(ops, pars, t))
        print('eval_kernel_grad %-42s L %-4g P %-4g worst %.2e of max |ref|' % (name, L, P, w))
        if not w <= dc.DK_TOL:
            fails.append('%s: off by %.2e of max |ref|' % (name, w))
        if not np.array_equal(dK, dK.transpose(0, 2, 1)):
            fails.append('%s: not symmetric to the bit' % name)
        if not np.isfinite(dK[:, eye]).all():
            fails.append('%s: not finite on the diagonal' % name)
    assert not fails, '\n'.join(fails)


def test_eval_kernel_grad_limits(ctx130):
    """NaN wherever a NaN parameter makes the kernel NaN (every id, every parameter); GammaExp's gamma and ell derivatives are
    0 on the diagonal; Piecewise is 0 beyond its support; an expression whose kernel reads past n_params is refused."""
    ctx, t = ctx130
    eye = np.eye(t.size, dtype=bool)
    for name, k in dc.kernels(8.0, 11.0)[:24]:
        ops, pars = dc.program_of(k)
        for l in range(pars.size):
            bad = pars.copy()
            bad[l] = np.nan
            K = ctx.eval_kernel(ops, bad, 0.0)
            dK = ctx.eval_kernel_grad(ops, bad)
            assert np.isnan(K[eye]).all(), (name, l)
            assert np.isnan(dK[:, np.isnan(K)]).all(), (name, l)
    dK = ctx.eval_kernel_grad([(0, kf.KID['GAMMAEXP'], 0)], [1.2, 1.5, 8.0])
    assert (dK[1][eye] == 0).all() and (dK[2][eye] == 0).all() and (dK[0][eye] == 2.4).all()
    dK = ctx.eval_kernel_grad([(0, kf.KID['PIECEWISE'], 0)], [6.0])
    far = np.abs(t[:, None] - t[None, :]) > 3.0
    assert (dK[0][far] == 0).all() and (dK[0][~far & ~eye] > 0).all()
    with pytest.raises(RuntimeError):
        ctx.eval_kernel_grad([(0, kf.KID['SE'], 0)], [1.0])


# ------------------------------------------------------------------ 2. gprn_grad_kernel
def _big_problem(L, P):
    """The set-up of tests/test_fill_gpu.py::test_grad_kernel_against_an_accurate_derivative, one committed sweep done."""
    rng = np.random.default_rng(11)
    N, p, q = 200, 5, 4
    t = np.sort(rng.uniform(0.0, 60.0, N))
    args = []
    for _ in range(p):
        args += [rng.normal(size=N), rng.uniform(0.1, 0.3, N)]
    g = gpyrn.inference(q, t, *args)
    nodes, weights = _grad_kernels(L, P)
    g.set_components(nodes, weights, [None] * p, [0.2] * p)
    nd, wt, mn, jt = g._get_components()
    ctx = g._setup_device(nd, wt, mn, jt)
    mu0, var0 = g._initMuVar(nd, wt, jt)
    ctx.set_muvar(np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float))
    ctx.keep_sigma(True)
    _, _, info = ctx.sweep(1, commit=True)
    assert info == 0
    mu, _ = ctx.get_muvar()
    m_w = mu[1:].reshape(q, p, N)
    ms = [mu[0, gp] if gp < q else m_w[divmod(gp - q, p)] for gp in range(q + q * p)]
    return g, ctx, t, list(nd) + list(wt), ms


def _entry_errors(dev, G, ops, pars, t, numpy_too=False):
    """Per parameter against the long-double derivative: [(|dev - ref| / sum |G| |dK|, ref, sum |G| |dK|, sum |G| |K|)];
    `numpy_too`: also the error of the plain fp64 NumPy evaluation of the same derivative (tests/_dk_numpy.py) against the
    same reference in the same norm, the worst of the kernel's parameters (else None)."""
    diag = np.eye(t.size, dtype=bool)
    dks = dc.reference(ops, pars, t)
    nps = _dk_numpy.dk_dpars(ops, pars, t) if numpy_too else None
    K = np.asarray(kf.program(kf.np_arith(np, np.longdouble), ops, pars, t[:, None], t[None, :], diag), dtype=float)
    GK = float(np.sum(np.abs(G) * np.abs(K)))
    out, np_err = [], None
    for l, dk in enumerate(dks):
        ref, scale = float(np.sum(G * dk)), float(np.sum(np.abs(G) * np.abs(dk)))
        out.append((abs(dev[l] - ref) / scale, ref, scale, GK))
        if numpy_too:
            np_err = max(np_err or 0.0, abs(float(np.sum(G * nps[l])) - ref) / scale)
    return out, np_err


# The kernels of tests/test_fill_gpu.py's list (+ WhiteNoise) for which a correct derivative misses 1e-12 sum |G| |dK|
# against the reference: the rows of the table above with device > 1e-12, by regime and position in the list.  These alone
# take 4 x the plain NumPy evaluation's error as their bound, and the test asserts that NumPy itself misses 1e-12 there;
# every other kernel, in every regime, is held to 1e-12.
BEYOND_THE_REFERENCE = {
    (8.0, 11.0): {19: 'd Periodic'},
    (0.1, 11.0): {15: 'QuasiNewPeriodic', 16: 'CosPeriodic', 17: 'QuasiCosPeriodic', 18: 'd SquaredExponential',
                  19: 'd Periodic', 20: 'd QuasiPeriodic', 22: 'SquaredExponential(theta=1.0, ell=0.1) * Periodic'},
    (8.0, 0.3): {19: 'd Periodic', 20: 'd QuasiPeriodic'},
}


@pytest.mark.parametrize('L,P', dc.REGIMES)
def test_grad_kernel_exact_meets_the_closed_form_bound(L, P):
    """Option on: EVERY kernel of the existing test's list within the closed forms' 1e-12 sum |G| |dK|, no noise term.  The
    kernels of BEYOND_THE_REFERENCE alone -- where a plain fp64 NumPy evaluation of the same derivative misses 1e-12 too --
    within 4 x that evaluation's error (the table at the top of the file)."""
    g, ctx, t, kernels, ms = _big_problem(L, P)
    try:
        assert ctx.option('grad_exact', 1) == 0
        fails = []
        for gp, k in enumerate(kernels):
            ops, pars = dc.program_of(k)
            dev = ctx.grad_kernel(gp, ms[gp], len(pars))
            Kinv, Pm = ctx.grad_matrices(gp)
            a = Kinv @ ms[gp]
            G = 0.5 * (Pm - Kinv + np.outer(a, a))
            listed = BEYOND_THE_REFERENCE[(L, P)].get(gp)
            assert listed is None or str(k).startswith(listed), (gp, str(k))
            errs, np_err = _entry_errors(dev, G, ops, pars, t, numpy_too=True)
            bound = GRAD_TOL_CLOSED if listed is None else 4.0 * np_err
            print('grad_kernel exact L %-4g P %-4g %-60s device %.2e NumPy %.2e bound %.2e of sum |G||dK|'
                  % (L, P, str(k)[:60], max(e[0] for e in errs), np_err, bound))
            if listed is not None and not np_err > GRAD_TOL_CLOSED:
                fails.append('%s: listed as beyond the reference, but NumPy is within %.2e' % (k, np_err))
            for l, (e, ref, scale, _) in enumerate(errs):
                if not e <= bound:
                    fails.append('%s parameter %d: device %.15g, reference %.15g, off by %.2e of sum |G||dK|'
                                 % (k, l, dev[l], ref, e))
    finally:
        ctx.keep_sigma(False)
    assert not fails, '\n'.join(fails)


def test_grad_kernel_with_the_option_off_returns_todays_bits():
    """Two contexts on one problem: one whose option was never set, one set to 1 and back to 0.  With the option on the
    kernels that are not closed forms move, the three closed forms keep their bits."""
    L, P = dc.REGIMES[0]
    g0, c0, t, kernels, ms0 = _big_problem(L, P)
    g1, c1, _, _, ms1 = _big_problem(L, P)
    try:
        assert c1.option('grad_exact', 1) == 0
        on = [c1.grad_kernel(gp, ms1[gp], len(dc.program_of(k)[1])) for gp, k in enumerate(kernels)]
        assert c1.option('grad_exact', 0) == 1 and c1.option('grad_exact') == 0
        moved = 0
        for gp, k in enumerate(kernels):
            ops, pars = dc.program_of(k)
            assert np.array_equal(ms0[gp], ms1[gp])
            never = c0.grad_kernel(gp, ms0[gp], len(pars))
            back = c1.grad_kernel(gp, ms1[gp], len(pars))
            assert np.array_equal(never, back), str(k)
            if len(ops) == 1 and ops[0][1] in CLOSED:
                assert np.array_equal(never, on[gp]), str(k)
            else:
                moved += not np.array_equal(never, on[gp])
        assert moved >= 15
        with pytest.raises(RuntimeError):
            c1.option('grad_exact', 2)
        assert c1.option('grad_exact') == 0
    finally:
        c0.keep_sigma(False)
        c1.keep_sigma(False)


# ------------------------------------------------------------------ 3. gprn_grad_elbo
def _mixed_kernels():
    """q = 2, p = 2: closed forms alone (SE, QuasiPeriodic), single kernels and composites that take the exact form."""
    c = covfunc
    nodes = [c.Matern52(1.0, 6.0) + c.WhiteNoise(0.3), c.QuasiPeriodic(1.0, 20.0, 7.0, 0.8)]
    weights = [c.RationalQuadratic(0.9, 1.5, 8.0) + c.WhiteNoise(0.3),
               c.SquaredExponential(1.1, 15.0) * c.Periodic(0.9, 9.0, 0.7) + c.WhiteNoise(0.2),
               c.SquaredExponential(0.8, 12.0),
               c.Matern32(0.7, 5.0) + c.Exponential(0.5, 9.0)]
    return nodes, weights


def _mixed_model(N, mask=False, order='reference', kernels=None, **kw):
    rng = np.random.default_rng(100 + N)
    p, q = 2, 2
    t = np.sort(rng.uniform(0.0, 60.0, N))
    args = []
    for i in range(p):
        args += [np.sin(t / (5.0 + i)) + 0.3 * rng.normal(size=N), rng.uniform(0.1, 0.3, N)]
    m = MR.partial_mask(p, N, 3) if mask else None
    g = gpyrn.inference(q, t, *args, mask=m, sweep_order=order, **kw)
    nodes, weights = kernels if kernels is not None else _mixed_kernels()
    g.set_components(nodes, weights, [meanfunc.Constant(0.1), meanfunc.Constant(0.0)], [0.3, 0.4])
    return g, t


def _committed(g, sweeps=1):
    nd, wt, mn, jt = g._get_components()
    ctx = g._setup_device(nd, wt, mn, jt)
    assert g.last_info == 0
    mu0, var0 = g._initMuVar(nd, wt, jt)
    ctx.set_muvar(np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float))
    _, _, info = ctx.sweep(sweeps, commit=True)
    assert info == 0
    return ctx, list(nd) + list(wt)


@pytest.mark.parametrize('N,mask,order', [(45, False, 'reference'), (200, False, 'reference'), (45, True, 'reference'),
                                          (200, True, 'reference'), (45, False, 'sequential'), (200, False, 'sequential')])
def test_grad_elbo_exact(N, mask, order):
    """N = 45 (one tile) and N = 200 on a mixed model, plain, under a partial data mask and in the sequential order: with the
    option on every entry within 1e-12 sum |G| |dK| of sum G dK_ref (G from gprn_grad_matrix); within the difference path's
    documented bound of the option-off result; two calls the same bits; the closed forms' entries the bits of option off.
    Setting the option leaves the committed sweep good (gprn_set_option: nothing on the device changes)."""
    g, t = _mixed_model(N, mask, order)
    ctx, kernels = _committed(g)
    n_k = sum(len(dc.program_of(k)[1]) for k in kernels)
    off = ctx.grad_elbo(n_k)
    assert ctx.option('grad_exact', 1) == 0
    on = ctx.grad_elbo(n_k)                                 # (no new sweep: the option does not end the sweep's validity)
    assert np.array_equal(on, ctx.grad_elbo(n_k))
    assert np.all(np.isfinite(on))
    fails, pos = [], 0
    for gp, k in enumerate(kernels):
        ops, pars = dc.program_of(k)
        G = ctx.grad_matrix(gp)
        errs, _ = _entry_errors(on[pos:pos + pars.size], G, ops, pars, t)
        closed = len(ops) == 1 and ops[0][1] in CLOSED
        print('grad_elbo exact N %d mask %d %s %-60s device %.2e of sum |G||dK|'
              % (N, mask, order, str(k)[:60], max(e[0] for e in errs)))
        for l, (e, ref, scale, GK) in enumerate(errs):
            if not e <= GRAD_TOL_CLOSED:
                fails.append('%s parameter %d: device %.15g, reference %.15g, off by %.2e of sum |G||dK|'
                             % (k, l, on[pos + l], ref, e))
            if closed:
                if on[pos + l] != off[pos + l]:
                    fails.append('%s parameter %d: a closed form moved with the option' % (k, l))
            else:
                noise = GRAD_NOISE * 2.0 ** -53 * GK / (1e-6 * max(1.0, abs(pars[l])))
                if not abs(on[pos + l] - off[pos + l]) <= (GRAD_TOL_FD + GRAD_TOL_CLOSED) * scale + noise:
                    fails.append('%s parameter %d: exact %.15g and differences %.15g apart' % (k, l, on[pos + l], off[pos + l]))
        pos += pars.size
    assert ctx.option('grad_exact', 0) == 1
    assert np.array_equal(off, ctx.grad_elbo(n_k))
    assert ctx.option('fallbacks') == 0
    assert not fails, '\n'.join(fails)


def test_grad_elbo_of_single_closed_forms_keeps_its_bits():
    c = covfunc
    kernels = ([c.SquaredExponential(1.0, 9.0), c.Periodic(0.9, 7.0, 0.8)],
               [c.QuasiPeriodic(1.0, 20.0, 7.0, 0.8), c.SquaredExponential(0.8, 12.0), c.Periodic(0.7, 11.0, 0.9),
                c.QuasiPeriodic(0.6, 15.0, 5.0, 0.7)])
    g, t = _mixed_model(130, kernels=kernels)
    ctx, ks = _committed(g)
    n_k = sum(k.pars.size for k in ks)
    off = ctx.grad_elbo(n_k)
    ctx.option('grad_exact', 1)
    assert np.array_equal(off, ctx.grad_elbo(n_k))


# ------------------------------------------------------------------ 4. the batch
@pytest.mark.parametrize('N,B,budget_mb', [(45, 8, 1), (200, 3, 1)])
def test_batch_slots_are_the_one_by_one_gradient(N, B, budget_mb):
    """nELBO_and_grad_batch(exact_derivatives=True) after forced sweeps, the gradient pass in groups (a small budget: a chunk
    boundary inside the list): every slot's kernel entries are the bits of gprn_grad_elbo with the option on after the
    same forced sweeps on a context of its own."""
    SWEEPS = 2
    g, t = _mixed_model(N, exact_derivatives=True)
    g1, _ = _mixed_model(N, exact_derivatives=True)
    g._backend().option('batch_mem_mb', budget_mb)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(5)
    sets = [x0 * rng.uniform(0.95, 1.05, x0.size) for _ in range(B)]
    assert g._batch_stage([x.copy() for x in sets]) is not None
    vals, grads = g.nELBO_and_grad_batch(sets, sweeps=SWEEPS)
    assert g.last_info == 0 and grads.shape == (B, x0.size) and np.all(np.isfinite(grads))
    assert g._backend().option('grad_exact') == 1
    print('batch exact N %d: %d evaluations per chunk of %d' % (N, g._backend().option('batch_chunk'), B))
    if N > 128:
        assert g._backend().option('batch_chunk') < B              # (a chunk boundary inside the list)
    n_k = sum(k.pars.size for k in chain(g.nodes, g.weights))
    # option off on the same list: the entries of the kernels that are not closed forms move
    g.exact_derivatives = False
    _, grads_off = g.nELBO_and_grad_batch(sets, sweeps=SWEEPS)
    assert g._backend().option('grad_exact') == 0
    assert not np.array_equal(grads[:, :n_k], grads_off[:, :n_k])
    worst = 0.0
    for b, x in enumerate(sets):
        g1.set_parameters(x.copy())
        ctx, _ = _committed(g1, SWEEPS)
        assert ctx.option('grad_exact') == 1
        one = -ctx.grad_elbo(n_k) / g1.q
        worst = max(worst, float(np.abs(grads[b, :n_k] - one).max() / np.abs(one).max()))
        assert np.array_equal(grads[b, :n_k], one), 'slot %d: differs from the one-by-one gradient by %.2e of its largest entry' % (b, worst)
    assert g._backend().option('fallbacks') == 0


# ------------------------------------------------------------------ 5. the fall-back
class _ShortPolynomial(covfunc.covFunction):
    """WhiteNoise + Polynomial whose exponent lies PAST the program's parameters (the device pads with 0: K = w^2 I + 1): the
    sums of the exact form are sized by n_params, so this program keeps the difference path under the option."""
    _param_names = ('w', 'a', 'b')
    _tag = 'SP'

    def __call__(self, r):
        return self.pars[0] ** 2 * (r == 0) + 1.0

    def _device_program(self):
        return ([(covfunc.OP_PUSH, kf.KID['WHITENOISE'], 0), (covfunc.OP_PUSH, kf.KID['POLYNOMIAL'], 1),
                 (covfunc.OP_ADD, 0, 0)], np.asarray(self.pars, dtype=float).ravel())


def test_a_program_past_the_exact_forms_limit_keeps_the_difference_path():
    nodes, weights = _mixed_kernels()
    weights[3] = _ShortPolynomial(0.8, 0.02, 1.5)
    g, t = _mixed_model(130, kernels=(nodes, weights))
    ctx, ks = _committed(g)
    n_k = sum(k.pars.size for k in ks)
    off = ctx.grad_elbo(n_k)
    ctx.option('grad_exact', 1)
    on = ctx.grad_elbo(n_k)
    assert np.array_equal(on[-3:], off[-3:]) and np.all(np.isfinite(on)) and off[-3] != 0
    assert not np.array_equal(on[:2], off[:2])              # (Matern52 + WhiteNoise: the exact form)
    ops, pars = weights[3]._device_program()
    with pytest.raises(RuntimeError):
        ctx.eval_kernel_grad(ops, pars)
    # gprn_grad_kernel makes the same choice (latent GP 5 is the short program, latent GP 0 Matern52 + WhiteNoise)
    ctx.keep_sigma(True)
    try:
        _, _, info = ctx.sweep(1, commit=True)
        assert info == 0
        mu, _ = ctx.get_muvar()
        m5, m0 = mu[1:].reshape(g.q, g.p, g.N)[1, 1], mu[0, 0]
        k_on = ctx.grad_kernel(5, m5, 3), ctx.grad_kernel(0, m0, 3)
        ctx.option('grad_exact', 0)
        k_off = ctx.grad_kernel(5, m5, 3), ctx.grad_kernel(0, m0, 3)
    finally:
        ctx.keep_sigma(False)
    assert np.array_equal(k_on[0], k_off[0]) and k_off[0][0] != 0 and not np.array_equal(k_on[1], k_off[1])
    # ... and the batch pass: the short program's entries of every slot are the same bits with the attribute on and off
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * f for f in (1.0, 1.02, 0.97)]
    grads = {}
    for exact in (True, False):
        g.exact_derivatives = exact
        g._mu = g._var = None
        assert g._batch_stage([x.copy() for x in sets]) is not None
        grads[exact] = g.nELBO_and_grad_batch(sets, sweeps=2)[1]
    assert np.array_equal(grads[True][:, n_k - 3:n_k], grads[False][:, n_k - 3:n_k]) and np.all(grads[True][:, n_k - 3] != 0)
    assert not np.array_equal(grads[True][:, :2], grads[False][:, :2])
