"""The kernels whose exact parameter derivatives the tests pin (csrc/dk_eval.h), shared by the host-compiled check
(tests/test_dk_eval_host.py) and the device's (tests/test_grad_exact_gpu.py): every built-in id alone, the two-argument
ones and the three derivative kernels included, and four composites; the three regimes of
tests/test_fill_gpu.py::test_grad_kernel_against_an_accurate_derivative."""
import numpy as np

from gpyrn_amd import covfunc as c
from oracle import kernel_formulas as kf

REGIMES = [(8.0, 11.0),        # R1
           (0.1, 11.0),        # R3-lite: length scales a third of the median spacing
           (8.0, 0.3)]         # R5-lite: 200 periods over the span
DK_TOL = 2e-11                 # the reference's own stated accuracy against mpmath (1e-11), doubled


def times(N=130, seed=5):
    """Two 64-blocks of the fill and a ragged third (N = 130): padding and a block edge inside."""
    return np.sort(np.random.default_rng(seed).uniform(0.0, 60.0, N))


def kernels(L, P):
    """(name, kernel): all 24 device ids alone, then the composites."""
    E = 20 * L                 # the decay that multiplies a periodic part: long enough for the period to show (see above)
    alone = [c.Constant(0.5), c.WhiteNoise(0.7), c.SquaredExponential(1.0, L), c.Periodic(1.0, P, 0.8),
             c.QuasiPeriodic(1.0, E, P, 0.7), c.RationalQuadratic(0.7, 1.5, L), c.RQP(1.2, 0.9, E / 4, P, 0.7),
             c.Cosine(0.8, P), c.Exponential(1.1, L), c.Matern32(1.3, L), c.Matern52(0.7, L), c.GammaExp(1.2, 1.5, L),
             c.Piecewise(2 * L), c.Paciorek(1.1, L, 1.5 * L), c.NewPeriodic(1.2, 0.9, P, 0.8),
             c.QuasiNewPeriodic(1.1, 0.7, E, P, 0.9), c.CosPeriodic(1.3, P, 0.9),
             c.QuasiCosPeriodic(0.9, E, P, 0.8), c.Polynomial(1.0, 0.02, 1.5, 2.5), c.HarmonicPeriodic(2, 1.1, P, 0.9),
             c.QuasiHarmonicPeriodic(2, 0.9, E, P, 0.8), c.Derivative(c.SquaredExponential(1.2, L)),
             c.Derivative(c.Periodic(0.9, P, 0.8)), c.Derivative(c.QuasiPeriodic(1.1, E, P, 0.6))]
    se, per, m32 = c.SquaredExponential(1.1, E), c.Periodic(0.9, P, 0.5), c.Matern32(0.9, 2 * L)
    nested = c.Matern32(0.9, 2 * L)
    # (right-nested, six leaves deep, the same class twice: the parameter offsets of a leaf are its own)
    for k in (c.SquaredExponential(1.0, 3 * L), c.Exponential(1.0, L), c.RationalQuadratic(1.2, 0.5, 0.3 * L), c.Matern32(1.1, L),
              c.SquaredExponential(1.2, L)):
        nested = k + nested
    composites = [('SE*Periodic', se * per), ('SE+Matern32', se + m32),
                  ('(SE*Periodic)+Matern32*(RQ+WhiteNoise)',
                   (se * per) + m32 * (c.RationalQuadratic(1.2, 0.5, 0.3 * L) + c.WhiteNoise(0.6))),
                  ('nested sum of six', nested)]
    out = [(type(k).__name__ if not isinstance(k, c.Derivative) else 'd' + type(k.k).__name__, k) for k in alone]
    ids = sorted(k._device_program()[0][0][1] for _, k in out)
    assert ids == list(range(24)), ids
    return out + composites


def program_of(k):
    ops, pars = k._device_program()
    return [tuple(int(v) for v in op) for op in ops], np.asarray(pars, dtype=float)


# The reference is a Richardson difference of relative step 1e-6: its own truncation error is (step x sensitivity)^4, its
# rounding floor 2^-64 max |K| / step.  For the PERIOD of the two harmonic kernels the first is not small: their cotangents
# cot(pi t / P) stand next to poles, the kernel moves through its whole range over dP / P ~ 1e-4, and the reference changes by
# 1.7e-10 (P = 11) to 3.5e-7 (P = 0.3) of max |dK/dP| between the steps 1e-6 and 1e-7 (tests/test_dk_eval_host.py asserts
# this from the reference alone).  That one parameter takes the reference at step 3e-8, where the truncation (1/123 of the
# 3.5e-11 left at 1e-7) and the rounding floor are both below the bound; every other parameter the default.
REFERENCE_STEP = {(kf.KID['HARMONICPERIODIC'], 2): 3e-8, (kf.KID['QUASIHARMONICPERIODIC'], 3): 3e-8}


def reference(ops, pars, t, step=None):
    """[dK/dpars[l]] (N, N) in fp64 from the long-double Richardson reference (`step`: its relative step for every
    parameter; default: 1e-6 but for REFERENCE_STEP's)."""
    diag = np.eye(t.size, dtype=bool)

    def at(rel):
        return [np.asarray(d, dtype=float)
                for d in kf.dk_dpars_longdouble(np, ops, list(pars), t[:, None], t[None, :], diag, rel=rel)]
    if step is not None:
        return at(step)
    out = at(1e-6)
    for op, kid, off in ops:
        for (k, l), rel in REFERENCE_STEP.items():
            if op == kf.OP_PUSH and kid == k:
                out[off + l] = at(rel)[off + l]
    return out


def worst(dK, ref):
    """max over the parameters of max |dK - ref| / max |ref| (the bound's left side over DK_TOL's scale)."""
    w = 0.0
    for l, r in enumerate(ref):
        scale = float(np.abs(r).max())
        err = float(np.abs(dK[l] - r).max())
        w = max(w, err / scale if scale > 0 else (0.0 if err == 0 else np.inf))
    return w
