"""The element code of the exact parameter derivatives (gpyrn_amd/csrc/dk_eval.h) without a GPU: the header compiles for the
host (tests/dk_eval_host.cpp), and every formula, limit and the adjoint of a program's leaf is checked against the long-double
derivative of oracle/kernel_formulas.py at the bound the device's test uses."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import kernel_formulas as kf
from tests import _dk_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'gpyrn_amd', 'csrc')
# (the host clang of the ROCm toolchain is there wherever the library itself was built: no compiler is a failure, not a skip)
CXX = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++',
                        os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang++'))
            if c and shutil.which(c)), None)
GOLDEN = os.path.join(HERE, 'golden', 'dk_harmonic_period_mpmath.json')


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    assert CXX is not None, 'no host C++ compiler (CXX, c++, g++, clang++, the ROCm toolchain\'s clang++)'
    so = str(tmp_path_factory.mktemp('dk') / 'dk_eval_host.so')
    # (-ffp-contract=off: the same formulas whatever the host's FMA support; the bound does not need it)
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off', '-shared', '-fPIC', '-I', CSRC,
                    os.path.join(HERE, 'dk_eval_host.cpp'), '-o', so, '-lm'], check=True)
    lib = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    lib.dk_eval_host.argtypes = [ip, ctypes.c_int, dp, ctypes.c_int, dp, ctypes.c_int, dp]
    lib.dk_value_host.argtypes = [ctypes.c_int, dp, dp, ctypes.c_int, dp]

    def grad(ops, pars, t):
        flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 3))
        par = np.ascontiguousarray(pars, dtype=float)
        t = np.ascontiguousarray(t, dtype=float)
        out = np.empty((par.size, t.size, t.size))
        lib.dk_eval_host(flat.ctypes.data_as(ip), flat.shape[0], par.ctypes.data_as(dp), par.size, t.ctypes.data_as(dp),
                         t.size, out.ctypes.data_as(dp))
        return out

    def value(kid, pars, t):
        par = np.ascontiguousarray(pars, dtype=float)
        t = np.ascontiguousarray(t, dtype=float)
        K = np.empty((t.size, t.size))
        lib.dk_value_host(kid, par.ctypes.data_as(dp), t.ctypes.data_as(dp), t.size, K.ctypes.data_as(dp))
        return K
    return grad, value


@pytest.mark.parametrize('L,P', dc.REGIMES)
def test_every_kernel_and_composite_against_the_long_double_derivative(host, L, P):
    """max |dK - ref| <= 2e-11 max |ref| per parameter; symmetric (but Polynomial, whose two products commute only
    mathematically); finite on the diagonal."""
    grad, _ = host
    t = dc.times(130)
    fails = []
    for name, k in dc.kernels(L, P):
        ops, pars = dc.program_of(k)
        dK = grad(ops, pars, t)
        w = dc.worst(dK, dc.reference(ops, pars, t))
        print('%-45s L %-4g P %-4g worst %.2e' % (name, L, P, w))
        if not w <= dc.DK_TOL:
            fails.append('%s: off by %.2e of max |ref|' % (name, w))
        if not np.isfinite(dK[:, np.arange(t.size), np.arange(t.size)]).all():
            fails.append('%s: not finite on the diagonal' % name)
        if name != 'Polynomial' and not np.array_equal(dK, dK.transpose(0, 2, 1)):
            fails.append('%s: not symmetric' % name)
    assert not fails, '\n'.join(fails)


def test_values_against_the_long_double_formulas(host):
    """The header's own k (the sibling values of a MUL)."""
    _, value = host
    t = dc.times(40)
    A = kf.np_arith(np, np.longdouble)
    diag = np.eye(t.size, dtype=bool)
    tl = t.astype(np.longdouble)
    for L, P in dc.REGIMES:
        for name, k in dc.kernels(L, P)[:24]:
            ops, pars = dc.program_of(k)
            ref = np.asarray(kf.kernel(A, ops[0][1], [np.longdouble(v) for v in pars], tl[:, None], tl[None, :], diag), dtype=float)
            K = value(ops[0][1], pars, t)
            assert np.abs(K - ref).max() <= 2e-11 * np.abs(ref).max(), (name, L, P)


def test_the_references_step_for_the_harmonic_period():
    """Why tests/_dk_cases.py takes the reference at a smaller step for the period of the harmonic kernels: between the steps
    1e-6 and 1e-7 the reference itself moves by several times the bound there, between 1e-7 and the step in use no longer --
    and for a parameter of ordinary sensitivity (the amplitude) the default step is converged."""
    t = dc.times(130)
    for L, P in (dc.REGIMES[0], dc.REGIMES[2]):
        for name, k in dc.kernels(L, P)[19:21]:
            ops, pars = dc.program_of(k)
            (l, step), = [(key[1], v) for key, v in dc.REFERENCE_STEP.items() if key[0] == ops[0][1]]
            r6, r7, rs = (dc.reference(ops, pars, t, step=s) for s in (1e-6, 1e-7, step))
            scale = np.abs(rs[l]).max()
            assert np.abs(r6[l] - r7[l]).max() > 5 * dc.DK_TOL * scale, name
            assert np.abs(r7[l] - rs[l]).max() < 5 * dc.DK_TOL * scale, name
            assert np.abs(r6[1] - r7[1]).max() < dc.DK_TOL * np.abs(r6[1]).max(), name


def _mpmath_period_derivatives(points):
    """d k / dP at 40 digits for [(kid, pars, index of P, t_i, t_j)]: mpmath's own differentiation of the formulas of
    oracle/kernel_formulas.py."""
    import mpmath as mp
    out = []
    with mp.workdps(40):
        A = kf.mp_arith(mp)
        for kid, pars, l, ti, tj in points:
            q = [mp.mpf(repr(float(v))) for v in pars]
            f = lambda P: kf.kernel(A, kid, q[:l] + [P] + q[l + 1:], mp.mpf(repr(float(ti))), mp.mpf(repr(float(tj))), False)
            out.append(mp.nstr(mp.diff(f, q[l]), 25))
    return out


def test_the_harmonic_period_against_mpmath(host):
    """The one parameter whose reference takes a step of its own (REFERENCE_STEP), at a handful of elements per kernel and
    regime -- the largest |dK/dP| of the matrix among them -- against mpmath at 40 digits (tests/golden, recomputed here where
    mpmath is installed): the reference at that step AND the header's formula are within the bound of it; the reference at
    its default step is not."""
    import json
    grad, _ = host
    t = dc.times(130)
    golden = json.load(open(GOLDEN))
    seen = 0
    for L, P in (dc.REGIMES[0], dc.REGIMES[2]):
        for name, k in dc.kernels(L, P)[19:21]:
            ops, pars = dc.program_of(k)
            l = [key[1] for key in dc.REFERENCE_STEP if key[0] == ops[0][1]][0]
            ref, dflt, dK = dc.reference(ops, pars, t)[l], dc.reference(ops, pars, t, step=1e-6)[l], grad(ops, pars, t)[l]
            scale = np.abs(ref).max()
            order = np.argsort(-np.abs(np.tril(ref)), axis=None, kind='stable')[[0, 1, 5, 50, 500, 2000]]
            ij = [tuple(int(v) for v in np.unravel_index(o, ref.shape)) for o in order]
            rows = golden['%s L=%g P=%g' % (name, L, P)]
            assert [r['ij'] for r in rows] == [list(p_) for p_ in ij]
            try:
                fresh = _mpmath_period_derivatives([(ops[0][1], pars, l, t[i], t[j]) for i, j in ij])
                assert fresh == [r['dk_dP'] for r in rows], name
            except ImportError:
                pass
            exact = np.array([float(r['dk_dP']) for r in rows])
            at = tuple(np.array(ij).T)
            assert np.abs(ref[at] - exact).max() <= dc.DK_TOL * scale, name
            assert np.abs(dK[at] - exact).max() <= dc.DK_TOL * scale, name
            assert np.abs(dflt[at] - exact).max() > 5 * dc.DK_TOL * scale, name
            seen += 1
    assert seen == 4


def test_limits(host):
    """GammaExp's (a / l)^gamma ln(a / l) is 0 on the diagonal; Piecewise is 0 beyond its support; a NaN parameter gives NaN
    wherever the kernel's value is NaN."""
    grad, value = host
    t = dc.times(30)
    eye = np.eye(t.size, dtype=bool)
    dK = grad([(0, kf.KID['GAMMAEXP'], 0)], [1.2, 1.5, 8.0], t)
    assert (dK[1][eye] == 0).all() and (dK[2][eye] == 0).all() and (dK[0][eye] == 2.4).all()
    dK = grad([(0, kf.KID['PIECEWISE'], 0)], [6.0], t)
    far = np.abs(t[:, None] - t[None, :]) > 3.0
    assert far.any() and (dK[0][far] == 0).all() and (dK[0][~far & ~eye] > 0).all()
    for name, k in dc.kernels(8.0, 11.0)[:24]:
        ops, pars = dc.program_of(k)
        for l in range(pars.size):
            bad = pars.copy()
            bad[l] = np.nan
            K = value(ops[0][1], bad, t)
            dK = grad(ops, bad, t)
            assert np.isnan(dK[:, np.isnan(K)]).all(), (name, l)
            assert np.isnan(K[eye]).all(), (name, l)


def test_shared_and_unused_parameters(host):
    """Two leaves that read the same parameters add up; a parameter no leaf reads has derivative 0."""
    grad, _ = host
    t = dc.times(20)
    se = kf.KID['SE']
    one = grad([(0, se, 0)], [1.1, 8.0], t)
    two = grad([(0, se, 0), (0, se, 0), (1, 0, 0)], [1.1, 8.0, 5.0], t)
    assert np.array_equal(two[:2], one + one) and (two[2] == 0).all()
    # k * k: d/dq = 2 k dk/dq
    sq = grad([(0, se, 0), (0, se, 0), (2, 0, 0)], [1.1, 8.0], t)
    ref = dc.reference([(0, se, 0), (0, se, 0), (2, 0, 0)], [1.1, 8.0], t)
    assert dc.worst(sq, ref) <= dc.DK_TOL
