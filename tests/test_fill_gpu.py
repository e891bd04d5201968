"""The covariance fill (csrc/fill.hip) and the device's kernel-parameter gradient (gprn_grad_kernel) against a
high-precision reference: tests/golden/fill_highprec (oracle/gen_fill_highprec.py, mpmath at 40 digits) for every
built-in kernel, the composites and derivatives, over typical, BJD, short-scale, long-scale, many-period and degenerate
regimes; a long-double derivative of the same formulas (oracle/kernel_formulas.py) for the gradient."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc
from oracle import kernel_formulas as kf
from tests import _fill_fixture as ff
from tests import _fill_worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def filled():
    """Every case of the fixture filled once by this process (the symmetric fill, k_fill_sym, where it applies)."""
    cases, d = ff.load()
    return cases, d, _fill_worker.fill_all()


def _report(fails):
    return '\n'.join('%s: %d elements off, e.g. K[%d,%d] = %r, reference %r, allowed %.3g' % (name, len(v), *v[0])
                     for name, v in fails[:20])


def test_fill_within_the_bound_of_the_exact_kernel(filled):
    """|K - K_ref| <= (4 + 2 kappa) 2^-53 |K_ref| + the denormal floor, element by element, in every case and regime
    (NaN where the reference is NaN) -- the same bound NumPy's evaluation meets (tests/test_fill_highprec.py)."""
    cases, d, Ks = filled
    fails = [(c['name'], v) for c in cases for v in [ff.violations(Ks[c['name']], c, d)] if v]
    assert not fails, _report(fails)


def test_fill_follows_numpys_rounding_sequence(filled):
    """SquaredExponential, Periodic and QuasiPeriodic (exp_neg, div_rn, sin_sq_rad): within (4 + 2 kappa) ulp of the
    exact kernel GIVEN NumPy's rounded exponent, phase pi |r| / P and decay -- a few ulp whatever the phase, so that a
    quotient one ulp off or a reduction by pi short of a word shows.  The R5 cases pin sin_sq_rad's range: arguments up
    to 1e12."""
    cases, d, Ks = filled
    seq = [c for c in cases if c['seq']]
    assert {c['regime'] for c in seq} == {'R1', 'R2', 'R3', 'R4', 'R5', 'R6'}
    fails = [(c['name'], v) for c in seq for v in [ff.violations(Ks[c['name']], c, d, seq=True)] if v]
    assert not fails, _report(fails)


def test_degenerate_parameters_give_numpys_zero_one_and_nan(filled):
    """R6: ell^2 subnormal (1 / ell^2 = inf on the host), an overflowing quotient, NaN parameters.  Where the exact
    value is a double (0, theta^2 on the diagonal, NaN), the fill returns that double: the division's correction step
    must not turn NumPy's -0 / ell^2 or -inf into NaN."""
    cases, d, Ks = filled
    r6 = [c for c in cases if c['regime'] == 'R6']
    assert len(r6) >= 10
    for c in r6:
        i, j, hi, lo, _ = ff.case_arrays(c, d)
        exact = lo == 0
        assert exact.sum() >= c['n'] // 2, c['name']
        k = Ks[c['name']][i, j]
        bad = ~((k == hi) | (np.isnan(k) & np.isnan(hi)))
        assert not (bad & exact).any(), '%s: K[%d,%d] = %r, NumPy/exact %r' % (
            c['name'], i[bad & exact][0], j[bad & exact][0], k[bad & exact][0], hi[bad & exact][0])


def test_fill_is_symmetric_to_the_bit(filled):
    cases, d, Ks = filled
    for c in cases:
        K = Ks[c['name']]
        if c['kernel'] != 'Polynomial':
            assert np.array_equal(K, K.T, equal_nan=True), c['name']


def test_specialised_instantiation_equals_the_generic_program(filled):
    """k_fill_sym<KID> (one instantiation per kernel; SE / Periodic / QP with host reciprocals) against the generic
    postfix program k_fill_sym<-1> of k * Constant(1.0): the same bits."""
    cases, d, Ks = filled
    ctxs = {}
    try:
        for c in cases:
            if len(c['ops']) != 1:
                continue
            ctx = ctxs.get(c['tset'])
            if ctx is None:
                t = d['t_' + c['tset']]
                ctx = ctxs[c['tset']] = _hip.Context(0)
                ctx.set_data(t, np.zeros((1, t.size)), np.ones((1, t.size)), 1)
            npar = len(c['pars'])
            ops = c['ops'] + [[0, 0, npar], [2, 0, 0]]
            K = ctx.eval_kernel(ops, list(c['pars']) + [1.0], 0.0)
            assert np.array_equal(K, Ks[c['name']], equal_nan=True), c['name']
    finally:
        for ctx in ctxs.values():
            ctx.close()


def test_full_matrix_fill_equals_symmetric_fill(filled, tmp_path):
    """k_fill (GPRN_FILL_SYM=0, read once per process: a child process) gives the bits of k_fill_sym, case by case --
    and so is itself symmetric to the bit."""
    cases, d, Ks = filled
    out = str(tmp_path / 'full.npz')
    env = dict(os.environ, GPRN_FILL_SYM='0')
    pr = subprocess.run([sys.executable, '-m', 'tests._fill_worker', out], cwd=ROOT, env=env,
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert pr.returncode == 0, pr.stdout.decode(errors='replace')
    full = np.load(out)
    for c in cases:
        assert np.array_equal(full[c['name']], Ks[c['name']], equal_nan=True), c['name']


# ------------------------------------------------------------------ gradient
def _grad_kernels(L, P):
    """The three closed forms alone; every other kernel plus WhiteNoise(0.3), so that the prior stays well conditioned
    (Cosine is of rank two, the derivative kernels are nearly singular, CosPeriodic is indefinite) -- the difference path of the program runs
    over the kernel's own parameters all the same."""
    c = covfunc
    nodes = [c.SquaredExponential(1.0, L), c.Periodic(1.0, P, 0.8), c.QuasiPeriodic(1.0, 2 * L, P, 0.7), c.Constant(0.5)]
    weights = [c.WhiteNoise(0.7), c.RationalQuadratic(0.7, 1.5, L), c.RQP(1.2, 0.9, 2 * L, P, 0.7), c.Cosine(0.8, P),
               c.Exponential(1.1, L), c.Matern32(1.3, L), c.Matern52(0.7, L), c.GammaExp(1.2, 1.5, L),
               c.Piecewise(2 * L), c.Paciorek(1.1, L, 1.5 * L), c.NewPeriodic(1.2, 0.9, P, 0.8),
               c.QuasiNewPeriodic(1.1, 0.7, 2 * L, P, 0.9), c.CosPeriodic(1.3, P, 0.9),
               c.QuasiCosPeriodic(0.9, 2 * L, P, 0.8), c.Derivative(c.SquaredExponential(1.2, L)),
               c.Derivative(c.Periodic(0.9, P, 0.8)), c.Derivative(c.QuasiPeriodic(1.1, 2 * L, P, 0.6)),
               c.SquaredExponential(1.1, L) + c.Matern32(0.4, 0.5 * L),
               c.SquaredExponential(1.0, L) * c.Periodic(1.0, P, 0.5), c.SquaredExponential(0.8, 2 * L)]
    nodes[3] = nodes[3] + c.WhiteNoise(0.3)
    # (exp(-2 cos^2 / ell^2) is largest half a period away from the diagonal: not positive definite, eigenvalues down to -80 here)
    weights = [k + c.WhiteNoise(10.0 if isinstance(k, (c.CosPeriodic, c.QuasiCosPeriodic)) else 0.3) for k in weights]
    return nodes, weights


CLOSED = (kf.KID['SE'], kf.KID['PERIODIC'], kf.KID['QP'])
GRAD_TOL_CLOSED, GRAD_TOL_FD, GRAD_NOISE = 1e-12, 1e-7, 8.0       # include/gprn_hip.h, gprn_grad_kernel


@pytest.mark.parametrize('L,P', [(8.0, 11.0),        # R1
                                 (0.1, 11.0),        # R3-lite: length scales a third of the median spacing
                                 (8.0, 0.3)])        # R5-lite: 200 periods over the span
def test_grad_kernel_against_an_accurate_derivative(L, P):
    """gprn_grad_kernel's < G, dK/dtheta >, G = 1/2 (K^-1 S K^-1 + a a^T - K^-1), a = K^-1 m, after one committed sweep,
    against the same contraction with a long-double Richardson derivative of the kernel formulas (within 1e-11 of
    mpmath: tests/test_fill_highprec.py): closed forms (SE / Periodic / QP) within 1e-12 sum |G| |dK|, the programs'
    differences within 1e-7 sum |G| |dK| + 8 2^-53 sum |G| |K| / h (the rounding of K in a difference of step h).  Every built-in but the three two-argument kernels -- Polynomial,
    (Quasi)HarmonicPeriodic, which _KMatrix leaves without nugget and which would make the prior singular here; their
    gradient takes the same program-difference path -- the three derivatives and two composites."""
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
    try:
        _, _, info = ctx.sweep(1, commit=True)
        assert info == 0
        mu, _ = ctx.get_muvar()
        m_w = mu[1:].reshape(q, p, N)
        diag = np.eye(N, dtype=bool)
        fails = []
        for gp, k in enumerate(list(nd) + list(wt)):
            ops, pars = k._device_program()
            m = mu[0, gp] if gp < q else m_w[divmod(gp - q, p)]
            dev = ctx.grad_kernel(gp, m, len(pars))
            Kinv, Pm = ctx.grad_matrices(gp)
            a = Kinv @ m
            G = 0.5 * (Pm - Kinv + np.outer(a, a))
            dks = kf.dk_dpars_longdouble(np, ops, pars, t[:, None], t[None, :], diag)
            closed = len(ops) == 1 and ops[0][1] in CLOSED
            tol = GRAD_TOL_CLOSED if closed else GRAD_TOL_FD
            # (a difference of the program also carries the rounding of K itself, 2^-53 |K| / h: the floor of any step h)
            GK = float(np.sum(np.abs(G) * np.abs(kf.program(kf.np_arith(np, np.longdouble), ops, pars, t[:, None],
                                                             t[None, :], diag).astype(float))))
            for l, dk in enumerate(dks):
                dk = np.asarray(dk, dtype=float)
                ref, scale = float(np.sum(G * dk)), float(np.sum(np.abs(G) * np.abs(dk)))
                noise = 0.0 if closed else GRAD_NOISE * 2.0 ** -53 * GK / (1e-6 * max(1.0, abs(pars[l])))
                if not abs(dev[l] - ref) <= tol * scale + noise:
                    fails.append('%s parameter %d: device %.15g, reference %.15g, off by %.2e of sum |G||dK|'
                                 % (k, l, dev[l], ref, abs(dev[l] - ref) / scale))
    finally:
        ctx.keep_sigma(False)
    assert not fails, '\n'.join(fails)
