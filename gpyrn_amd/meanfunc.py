"""Mean functions of the GPRN outputs.

Plugin surface of the reference's ``gpyrn/meanfunc.py`` (base :9-46,
``Sum``/``Product`` :49-117, concrete means :120-273).  Mean functions are
O(p N) host work evaluated once per ``ELBOcalc`` (meanfield.py:382-411,623):
for ONE evaluation per call they are NumPy, and their result, the
mean-subtracted data, is what gets uploaded (``gprn_set_y_resid``).  For many
parameter vectors side by side the built-in means also describe themselves as
a postfix program (``_device_program``, as covfunc's kernels do) that
csrc/mean.hip evaluates and differentiates for every vector in one launch
(``gprn_set_mean``, ``gprn_eval_mean``, ``gprn_eval_mean_grad``, and inside
the side-by-side batches ``gprn_elbocalc_batch_means``).
``Keplerian`` is new: the reference left it a stub (meanfunc.py:276-293).
"""
import numpy as np

from ._utils import Array, _array_input, _take_leading  # noqa: F401

__all__ = [
    'Constant', 'MultiConstant', 'Linear', 'Parabola', 'Cubic', 'Sine', 'Keplerian',
]

# mean ids of csrc/mean_eval.h (include/gprn_hip.h GPRN_M_*) and the postfix opcodes they share with covfunc's programs
MID = {'CONSTANT': 0, 'LINEAR': 1, 'PARABOLA': 2, 'CUBIC': 3, 'SINE': 4, 'KEPLERIAN': 5}
OP_PUSH, OP_ADD, OP_MUL = 0, 1, 2


def _is_builtin(cls):
    # a user subclass of a built-in may override __call__: never trust its id
    return cls.__module__ == __name__


class meanFunction:
    """Base class: ``pars`` vector, chained ``set_parameters``, ``+`` / ``*``."""
    _parsize = 0

    def __init__(self, *pars):
        self.pars = np.array(pars, dtype=float)

    def __repr__(self):
        inner = ', '.join(str(v) for v in self.pars)
        return f'{type(self).__name__}({inner})'

    def get_parameters(self):
        return self.pars

    @_array_input
    def set_parameters(self, p):
        return _take_leading(self, p, 'mean')

    def _dm_dpars(self, t):
        """d mean(t) / d pars, ``(n_pars, N)``: what the gradient of the bound form of the ELBO contracts with the weighted
        residual (``inference(..., elbo='bound')``).  Here Richardson-extrapolated central differences of the function itself
        (steps h and h / 2, h = 1e-4 max(1, |theta|): O(h^4), rounding near 1e-12 of the function's size); the polynomial means,
        ``Sine``, ``MultiConstant``, ``Sum`` and ``Product`` have closed forms.  ``None`` would mean: contributes nothing."""
        t = np.asarray(t, dtype=float)
        pars = np.array(self.pars, dtype=float)
        out = np.zeros((pars.size, t.size))

        def at(k, v):
            x = pars.copy()
            x[k] = v
            self.set_parameters(x)
            return np.asarray(self(t), dtype=float)

        try:
            for k in range(pars.size):
                h = 1e-4 * max(1.0, abs(pars[k]))
                d1 = (at(k, pars[k] + h) - at(k, pars[k] - h)) / (2.0 * h)
                d2 = (at(k, pars[k] + 0.5 * h) - at(k, pars[k] - 0.5 * h)) / h
                out[k] = (4.0 * d2 - d1) / 3.0
        finally:
            self.set_parameters(pars)
        return out

    _device_id = None

    def _device_program(self):
        """Postfix program ``(ops, params)`` of this mean for csrc/mean.hip -- ops are (opcode, mean id, offset of the
        leaf's parameters in ``params``) --, or None where the mean has to be evaluated on the host: ``MultiConstant``
        (it reads the observation ids) and every class not defined in this module."""
        if type(self)._device_id is None or not _is_builtin(type(self)):
            return None
        return [(OP_PUSH, type(self)._device_id, 0)], np.asarray(self.pars, dtype=float).ravel()

    def __add__(self, other):
        return Sum(self, other)

    __radd__ = __add__

    def __mul__(self, other):
        return Product(self, other)

    __rmul__ = __mul__


class _pair(meanFunction):
    """Two means combined; parameters are the concatenation of both."""

    def __init__(self, m1, m2):
        self.m1, self.m2 = m1, m2
        self._param_names = tuple(self._names(m1, m2))
        self._parsize = m1._parsize + m2._parsize
        self.pars = np.r_[m1.pars, m2.pars]

    @staticmethod
    def _names(m1, m2):
        return list(m1._param_names) + list(m2._param_names)

    @_array_input
    def set_parameters(self, p):
        n = self.pars.size
        assert len(p) >= n, f'too few parameters for mean {type(self).__name__}'
        self.pars = np.array(p[:n], dtype=float) if len(p) > n else p
        rest = self.m1.set_parameters(p)
        rest = self.m2.set_parameters(rest)
        return rest if len(p) > n else None

    _opcode = None

    def _device_program(self):
        if self._opcode is None or not _is_builtin(type(self)):
            return None
        sides = [m._device_program() if isinstance(m, meanFunction) else None for m in (self.m1, self.m2)]
        if sides[0] is None or sides[1] is None:
            return None
        (ops_l, par_l), (ops_r, par_r) = sides
        shifted = [(op, mid, off + par_l.size if op == OP_PUSH else 0) for op, mid, off in ops_r]
        return ops_l + shifted + [(self._opcode, 0, 0)], np.r_[par_l, par_r]


class Sum(_pair):
    """m1 + m2; equal classes get numbered parameter names (meanfunc.py:49-82)."""
    _opcode = OP_ADD

    @staticmethod
    def _names(m1, m2):
        if m1.__class__ == m2.__class__:
            return [f'{n}1' for n in m1._param_names] + \
                   [f'{n}2' for n in m2._param_names]
        return list(m1._param_names) + list(m2._param_names)

    def __repr__(self):
        return f'{self.m1} + {self.m2}'

    @_array_input
    def __call__(self, t):
        return self.m1(t) + self.m2(t)

    def _dm_dpars(self, t):
        return np.concatenate((self.m1._dm_dpars(t), self.m2._dm_dpars(t)))


class Product(_pair):
    """m1 * m2 (meanfunc.py:85-117)."""
    _opcode = OP_MUL

    def __repr__(self):
        return f'{self.m1} * {self.m2}'

    @_array_input
    def __call__(self, t):
        return self.m1(t) * self.m2(t)

    def _dm_dpars(self, t):
        return np.concatenate((self.m1._dm_dpars(t) * self.m2(t)[None], self.m2._dm_dpars(t) * self.m1(t)[None]))


class Constant(meanFunction):
    """m(t) = c (meanfunc.py:120-135)."""
    _param_names = 'c',
    _parsize = 1
    _device_id = MID['CONSTANT']

    def __init__(self, c: float):
        super().__init__(c)

    @_array_input
    def __call__(self, t):
        return np.full(t.shape, self.pars[0])

    def _dm_dpars(self, t):
        return np.ones((1, np.size(t)))


class MultiConstant(meanFunction):
    """Per-instrument offsets relative to the last instrument, whose average
    is the final parameter (meanfunc.py:138-187).

    Args:
        offsets: [off_1, ..., off_{n-1}, mean_n]
        obsid: one-based instrument index of every observation
        time: observation times, same size as ``obsid``
    """
    _parsize = 0

    def __init__(self, offsets: np.ndarray, obsid: np.ndarray, time: np.ndarray):
        self.obsid, self.time = obsid, time
        self._parsize = (np.ediff1d(obsid) == 1).sum() + 1
        self.ii = obsid.astype(int) - 1
        if isinstance(offsets, float):
            offsets = [offsets]
        assert len(offsets) == self._parsize, \
            f'wrong number of parameters, expected {self._parsize} got {len(offsets)}'
        super().__init__(*offsets)
        self._param_names = [f'off{i}' for i in range(1, self._parsize)] + ['mean']

    def time_bins(self):
        """Edges between instruments: midpoints of the gaps, plus the start."""
        last_of_block = self.time[np.ediff1d(self.obsid, 0, None) != 0]
        first_of_next = self.time[np.ediff1d(self.obsid, None, 0) != 0]
        mid = np.mean((last_of_block, first_of_next), axis=0)
        return np.sort(np.r_[self.time[0], mid])

    @_array_input
    def __call__(self, t):
        offsets = np.pad(self.pars[:-1], (0, 1))
        if t.size == self.time.size:
            which = self.ii
        else:
            which = np.digitize(t, self.time_bins()) - 1
        return np.full_like(t, self.pars[-1]) + np.take(offsets, which)

    def _dm_dpars(self, t):
        t = np.asarray(t, dtype=float)
        which = self.ii if t.size == self.time.size else np.digitize(t, self.time_bins()) - 1
        out = np.zeros((self.pars.size, t.size))
        for k in range(self.pars.size - 1):
            out[k] = which == k
        out[-1] = 1.0
        return out


class Linear(meanFunction):
    """m(t) = slope (t - mean(t)) + intercept (meanfunc.py:190-208)."""
    _param_names = ('slope', 'intercept')
    _parsize = 2
    _device_id = MID['LINEAR']

    def __init__(self, slope: float, intercept: float):
        super().__init__(slope, intercept)

    @_array_input
    def __call__(self, t):
        return self.pars[0] * (t - t.mean()) + self.pars[1]

    def _dm_dpars(self, t):
        t = np.asarray(t, dtype=float)
        return np.array([t - t.mean(), np.ones(t.size)])


class Parabola(meanFunction):
    """m(t) = quad t^2 + slope t + intercept (meanfunc.py:211-229; the names
    tuple is ordered as in the reference)."""
    _param_names = ('slope', 'intercept', 'quadratic')
    _parsize = 3
    _device_id = MID['PARABOLA']

    def __init__(self, quad: float, slope: float, intercept: float):
        super().__init__(quad, slope, intercept)

    @_array_input
    def __call__(self, t):
        return np.polyval(self.pars, t)

    def _dm_dpars(self, t):
        t = np.asarray(t, dtype=float)
        return np.array([t ** k for k in range(self.pars.size - 1, -1, -1)])


class Cubic(meanFunction):
    """m(t) = cub t^3 + quad t^2 + slope t + intercept (meanfunc.py:232-251)."""
    _param_names = ('cub', 'quad', 'slope', 'intercept')
    _parsize = 4
    _device_id = MID['CUBIC']

    def __init__(self, cub: float, quad: float, slope: float, intercept: float):
        super().__init__(cub, quad, slope, intercept)

    @_array_input
    def __call__(self, t):
        return np.polyval(self.pars, t)

    def _dm_dpars(self, t):
        t = np.asarray(t, dtype=float)
        return np.array([t ** k for k in range(self.pars.size - 1, -1, -1)])


class Sine(meanFunction):
    """m(t) = amplitude sin(2 pi t / period + phase) (meanfunc.py:254-273)."""
    _param_names = ('amplitude', 'period', 'phase')
    _parsize = 3
    _device_id = MID['SINE']

    def __init__(self, amplitude: float, period: float, phase: float):
        super().__init__(amplitude, period, phase)

    @_array_input
    def __call__(self, t):
        amplitude, period, phase = self.pars
        return amplitude * np.sin((2 * np.pi * t / period) + phase)

    def _dm_dpars(self, t):
        t = np.asarray(t, dtype=float)
        amplitude, period, phase = self.pars
        arg = (2 * np.pi * t / period) + phase
        return np.array([np.sin(arg), -amplitude * np.cos(arg) * 2 * np.pi * t / period**2, amplitude * np.cos(arg)])


# Newton steps of the Kepler solver (host and csrc/mean_eval.h alike): the smallest count at which one more step changes
# no bit of E on tests/golden/mean_highprec's grid of (e, M) AND on a dense grid out to e = 1 - 2^-53 (the fixture's grid
# alone would allow one fewer: the seventh step still moves four of the dense grid's 30 000 points by an ulp) --
# tests/test_mean_keplerian.py holds it to that
KEPLER_STEPS = 7


def _e_minus_sin(E):
    """E - sin E without the cancellation at small E (the series below |E| = 1, 1 / 21! < 2^-53 / 3!)."""
    x = E * E
    s = 1.0 / 6.0
    poly = np.zeros_like(E)
    for k in range(20, 2, -2):                       # E^3 / 3! (1 - x / (4 5) (1 - x / (6 7) (1 - ... x / (20 21))))
        poly = (1.0 - poly) * (x / (k * (k + 1)))
    series = E * x * s * (1.0 - poly)
    return np.where(np.abs(E) < 1.0, series, E - np.sin(E))


def _kepler_E(Ma, e):
    """E in [0, pi] with E - e sin E = Ma, 0 <= Ma <= pi, 0 <= e < 1.  f(E) = E - e sin E - Ma is increasing and convex
    there and the root lies in [Ma, min(Ma + e, pi)]: from any start in that bracket one Newton step lands right of the
    root (clamped to the bracket it stays right of it), and from the right Newton descends monotonically -- no divergence
    at any e < 1, no data-dependent loop: KEPLER_STEPS steps.  The residual is formed as (1 - e) E + e (E - sin E) - Ma, which does not cancel
    near E = 0, e = 1."""
    hi = np.minimum(Ma + e, np.pi)
    # starter: the root of the cubic f has at E = 0, (1 - e) E + e E^3 / 6 = Ma, where that model holds (small Ma, large e);
    # else Ma + e sin Ma / (1 - sin(Ma + e) + sin Ma), which is exact at both ends of [0, pi]
    with np.errstate(all='ignore'):
        a = 2.0 * (1.0 - e) / np.maximum(e, 0.25)
        b = 3.0 * Ma / np.maximum(e, 0.25)
        w = np.cbrt(b + np.sqrt(b * b + a * a * a))
        cubic = w - a / w
        sm = np.sin(Ma)
        smooth = Ma + e * sm / (1.0 - np.sin(Ma + e) + sm)
    E = np.where((e > 0.5) & (Ma < 0.25), cubic, smooth)
    E = np.minimum(np.maximum(E, Ma), hi)
    om = 1.0 - e
    lo = np.full_like(E, -1.0)                         # the largest iterate known to lie left of the root (f < 0)
    for _ in range(KEPLER_STEPS):
        f = (om * E + e * _e_minus_sin(E)) - Ma
        En = E - f / (1.0 - e * np.cos(E))
        En = np.minimum(np.maximum(En, Ma), hi)
        # left of the root: up, wherever Newton lands.  Right of it: only down, and never back onto a point already known to
        # lie left -- rounding in f can then set up no cycle between neighbours, and a step that rounding threw left of the
        # root (where f is nearly linear Newton lands ON it, give or take the subtraction) is made good by the next
        left = f < 0
        lo = np.where(left, np.maximum(lo, E), lo)
        E = np.where(left, En, np.where(En <= lo, E, np.minimum(E, En)))
    return E


class Keplerian(meanFunction):
    """m(t) = K [cos(nu + w) + e cos w], the radial velocity of a Keplerian orbit: period P, semi-amplitude K,
    eccentricity e, argument of periastron w, time of periastron Tp; M = 2 pi (t - Tp) / P, E - e sin E = M, and the true
    anomaly nu from cos nu = (cos E - e) / D, sin nu = sqrt(1 - e^2) sin E / D, D = 1 - e cos E.  (The reference left
    this class a stub, meanfunc.py:276-293, over _utils.keplerian, _utils.py:62-118, whose iteration does not converge
    for e > 0; neither is restated here.)  e outside [0, 1), P <= 0 or a non-finite parameter: NaN at every time."""
    _param_names = ('P', 'K', 'e', 'w', 'Tp')
    _parsize = 5
    _device_id = MID['KEPLERIAN']

    def __init__(self, P: float, K: float, e: float, w: float, Tp: float):
        super().__init__(P, K, e, w, Tp)

    def _orbit(self, t):
        """(m, dm / d(P, K, e, w, Tp)) at the times t; the formulas of csrc/mean_eval.h, operation by operation."""
        t = np.asarray(t, dtype=float)
        P, K, e, w, Tp = (float(v) for v in self.pars)
        if not (np.isfinite([P, K, e, w, Tp]).all() and 0.0 <= e < 1.0 and P > 0.0):
            nan = np.full(t.shape, np.nan)
            return nan, np.full((5,) + t.shape, np.nan)
        x = (t - Tp) / P
        fr = x - np.rint(x)                            # M reduced to [-pi, pi] through the fraction of a period
        Ma = 2 * np.pi * np.abs(fr)
        sg = np.where(fr < 0, -1.0, 1.0)               # E(-M) = -E(M)
        E = _kepler_E(Ma, e)
        cE, sE = np.cos(E), sg * np.sin(E)
        D = 1.0 - e * cE
        q = np.sqrt((1.0 - e) * (1.0 + e))
        cn, sn = (cE - e) / D, q * sE / D
        cw, sw = np.cos(w), np.sin(w)
        c, s = cn * cw - sn * sw, sn * cw + cn * sw    # cos(nu + w), sin(nu + w)
        m = K * c + K * e * cw
        nuM = q / (D * D)
        nue = sn * (2.0 + e * cn) / ((1.0 - e) * (1.0 + e))
        ks = K * s
        return m, np.array([ks * nuM * (2 * np.pi * x) / P, c + e * cw, -ks * nue + K * cw, -(ks + K * e * sw),
                            ks * nuM * (2 * np.pi / P)])

    @_array_input
    def __call__(self, t):
        return self._orbit(t)[0]

    def _dm_dpars(self, t):
        return self._orbit(np.asarray(t, dtype=float).ravel())[1]
