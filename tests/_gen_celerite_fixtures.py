"""High-precision reference of the celerite kernels: tests/golden/celerite_highprec.{npz,json}
(python -m tests._gen_celerite_fixtures [--only NAME ...]).

mpmath at 40 digits over tests/_celerite_formulas.py, no GPU.  The time sets are oracle/gen_fill_highprec.time_sets():
``R1`` 200 times over a span of 60, ``R2`` 200 BJD stamps (2.45e6 + [0, 3000]) with repeated ones, ``R3`` 120 times a day
apart.  Per case -- a kernel of gpyrn_amd.covfunc written as the expression that builds it -- three records:

* the SQUARE sample, in the layout tests/_fill_fixture.violations takes (``i``, ``j``, ``hi`` + ``lo`` the exact value as a
  double-double, ``kappa`` the element's condition number sum_u |u dk/du| / |k| over u in {r, every parameter}; per case
  ``off``, ``n``, ``expr``, ``tset``): the lower triangle of the 12 x 12 corner, eight elements of the diagonal (both ends,
  the 128-row tile's edge), every pair of equal stamps, seeded random pairs -- 280 elements.  NO rounded intermediate of a
  formula enters kappa: kernel_formulas.N_INTERMEDIATES has no counterpart here, the value code is held to r and the
  parameters alone;
* ``dk``: at the same elements and per parameter of the program the derivative d k / d par[l] -- mpmath's own
  differentiation (mp.diff) of the value formula, rounded to double; (n_par, n) per case from ``dk_off``.  A case with a NaN
  parameter has none (``dk_off`` null), and neither have the three cases at 1e6 radians (DK_DROPPED): no formula in
  r = fl(t_i - t_j) meets the norm-wise bound of the derivatives there -- r is itself half an ulp of 60 off, 3.5e-15, which
  1.7e4 radians a day turn into 6e-11 of phase, three times the bound.  Their values stay, under the value bound, whose
  kappa covers r;
* the RECTANGULAR sample as oracle/gen_rect_highprec.py lays it out, its keys under the prefix ``rect_``: N = 129 data times
  (the first 129 of the set) against ns = 130 prediction times (a tenth beyond either end of the data, eight bit-equal to a
  data time -- the first and the last among them, and the pairs (t*_3, t_5), (t*_5, t_3) --, two equal to each other);
  ``i``, ``j``, ``hi``, ``lo``, ``kappa`` the reference form at 180 elements of K* (the 8 x 8 corner, every coincident pair,
  the ends of the last row and column, random ones), ``co_*`` the posterior form where it differs (nugget 1e-6 and WhiteNoise
  as delta(t, t')), ``kss_*`` all of k** in the reference form (+ 1.25e-12), then in the posterior form.

Cases (the issue's list): SHO typical at six Q, BJD, the critical neighbourhood Q = 1/2 +- {2^-52, 1e-12, 1e-9, 1e-6, 1e-3},
the over-damped far tail (a to 3e4 and 1e5 with k above 1e-3 theta^2), Q = 1e4, phases of 1e3 and 1e6 radians at Q = 3 and
1e5, deep underflow, NaN in each parameter; Rotation typical, BJD, Q0 = 1e-8, dQ = 0, f in {0, 1e6}, far phases, NaN;
CeleriteTerm typical, BJD, the real term, d tau to 1e6 at c = 1e-9, underflow, NaN; two composites."""
import argparse
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from gpyrn_amd import covfunc  # noqa: E402
from oracle import gen_fill_highprec as sq  # noqa: E402
from oracle import kernel_formulas as kf  # noqa: E402
from tests import _celerite_formulas as cf  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
DPS = sq.DPS
SPAN = sq.SPAN
CORNER, N_DIAG, MAX_SAMPLES = 12, 8, 280
N_RECT, NS, RECT_CORNER, RECT_SAMPLES = 129, 130, 8, 180
TINY_NUGGET, SETUP_NUGGET = 1.25e-12, 1e-6
COINCIDE = ((3, 5), (5, 3), (9, 12), (40, 0), (41, 60), (77, 127), (100, 64), (129, 128))
TWINS = (20, 88)
DK_DROPPED = ('SHO_phase_3', 'Rotation_phase_1', 'CeleriteTerm_phase_0')
nan = float('nan')


def _phase_period(x):
    """P0 (P) such that 2 pi span / P0 = x"""
    return float(2 * np.pi * SPAN / x)


def case_list():
    out = []

    def add(name, kernel, tset, expr):
        out.append(dict(name=name, kernel=kernel, tset=tset, expr=expr))

    def sho(name, tset, theta, P0, Q):
        add(name, 'SHO', tset, 'c.SHO(%s, %s, %s)' % tuple(sq._fmt(v) for v in (theta, P0, Q)))

    for k, Q in enumerate((0.05, 0.3, 0.5, float(1 / np.sqrt(2)), 3.0, 40.0)):
        sho('SHO_typical_%d' % k, 'R1', 1.3, 11.0, Q)
    for k, Q in enumerate((0.3, 3.0)):
        sho('SHO_bjd_%d' % k, 'R2', 1.3, 450.0, Q)
    for k, e in enumerate((2.0 ** -52, 1e-12, 1e-9, 1e-6, 1e-3)):
        sho('SHO_critical_above_%d' % k, 'R1', 1.3, 11.0, 0.5 + e)
        sho('SHO_critical_below_%d' % k, 'R1', 1.3, 11.0, 0.5 - e)
    # a = pi r / (P0 Q) reaches 3e4 (1e5) over the span; the exponent a (1 - h) ~ 2 a Q^2 stays at 6 (0.2)
    sho('SHO_tail_0', 'R1', 1.3, float(np.pi * SPAN / (3e4 * 1e-2)), 1e-2)
    sho('SHO_tail_1', 'R1', 1.3, float(np.pi * SPAN / (1e5 * 1e-3)), 1e-3)
    sho('SHO_highQ_0', 'R1', 1.3, 11.0, 1e4)
    for k, (x, Q) in enumerate(((1e3, 3.0), (1e6, 3.0), (1e3, 1e5), (1e6, 1e5))):
        sho('SHO_phase_%d' % k, 'R1', 1.3, _phase_period(x), Q)
    sho('SHO_underflow_0', 'R3', 1.3, 1e-3, 0.3)
    sho('SHO_underflow_1', 'R3', 1.3, 1e-3, 3.0)
    for k, pars in enumerate(((nan, 11.0, 3.0), (1.3, nan, 3.0), (1.3, 11.0, nan))):
        sho('SHO_nan_%d' % k, 'R1', *pars)

    def rot(name, tset, *pars):
        add(name, 'Rotation', tset, 'c.Rotation(%s)' % ', '.join(sq._fmt(v) for v in pars))

    typical = (1.1, 9.0, 1.2, 0.3, 0.4)
    rot('Rotation_typical_0', 'R1', *typical)
    rot('Rotation_bjd_0', 'R2', 1.1, 25.0, 1.2, 0.3, 0.4)
    rot('Rotation_smallQ0_0', 'R1', 1.1, 9.0, 1e-8, 0.3, 0.4)
    rot('Rotation_dQ0_0', 'R1', 1.1, 9.0, 1.2, 0.0, 0.4)
    rot('Rotation_f_0', 'R1', 1.1, 9.0, 1.2, 0.3, 0.0)
    rot('Rotation_f_1', 'R1', 1.1, 9.0, 1.2, 0.3, 1e6)
    rot('Rotation_phase_0', 'R1', 1.1, _phase_period(1e3), 30.0, 0.3, 0.4)
    rot('Rotation_phase_1', 'R1', 1.1, _phase_period(1e6), 1e5, 0.3, 0.4)
    for k in range(5):
        rot('Rotation_nan_%d' % k, 'R1', *[nan if l == k else v for l, v in enumerate(typical)])

    def cel(name, tset, *pars):
        add(name, 'CeleriteTerm', tset, 'c.CeleriteTerm(%s)' % ', '.join(sq._fmt(v) for v in pars))

    cel('CeleriteTerm_typical_0', 'R1', 1.2, 0.3, 0.1, 0.7)
    cel('CeleriteTerm_bjd_0', 'R2', 1.2, 0.3, 0.002, 0.014)
    cel('CeleriteTerm_real_0', 'R1', 1.2, 0.0, 0.1, 0.0)
    cel('CeleriteTerm_phase_0', 'R1', 1.2, 0.3, 1e-9, float(1e6 / SPAN))
    cel('CeleriteTerm_underflow_0', 'R3', 1.2, 0.3, 1e3, 0.7)
    for k in range(4):
        cel('CeleriteTerm_nan_%d' % k, 'R1', *[nan if l == k else v for l, v in enumerate((1.2, 0.3, 0.1, 0.7))])

    add('SHO_times_SE_plus_WN_0', 'composite', 'R1', 'c.SHO(1.3, 11.0, 3.0) * c.SquaredExponential(1.0, 30.0) + c.WhiteNoise(0.4)')
    add('SHO_times_SE_plus_WN_1', 'composite', 'R2', 'c.SHO(1.3, 450.0, 0.3) * c.SquaredExponential(1.0, 1500.0) + c.WhiteNoise(0.4)')
    add('Rotation_plus_Celerite_0', 'composite', 'R1', 'c.Rotation(1.1, 9.0, 1.2, 0.3, 0.4) + c.CeleriteTerm(0.5, 0.1, 0.05, 0.9)')
    add('Rotation_plus_Celerite_1', 'composite', 'R2', 'c.Rotation(1.1, 25.0, 1.2, 0.3, 0.4) + c.CeleriteTerm(0.5, 0.1, 0.002, 0.02)')
    return out


def build_kernel(expr):
    return eval(expr, {'c': covfunc, 'nan': nan})


def square_sample(t, seed):
    rng = np.random.default_rng(seed)
    N = t.size
    seen, out = set(), []

    def add(i, j):
        if (i, j) not in seen:
            seen.add((i, j))
            out.append((i, j))
    for i in range(CORNER):
        for j in range(i + 1):
            add(i, j)
    for i in [0, 127 % N, 128 % N, N - 1] + [int(v) for v in rng.integers(0, N, N_DIAG - 4)]:
        add(i, i)
    for i, j in zip(*np.nonzero((t[:, None] == t[None, :]) & ~np.eye(N, dtype=bool))):
        add(int(i), int(j))
    while len(out) < MAX_SAMPLES:
        i, j = (int(v) for v in rng.integers(0, N, 2))
        add(i, j)
    return np.array(out[:MAX_SAMPLES], dtype=np.int64)


def rect_time_sets():
    """{set: (t, t*)}: the first 129 times of the square set (R3: 129 of its rule) and 130 prediction times of a draw of
    their own"""
    rng = np.random.default_rng(20261021)
    out = {}
    for reg, full in sq.time_sets().items():
        if reg not in ('R1', 'R2', 'R3'):
            continue
        # (R3 has 120 times: 129 by the same rule, a day apart)
        t = full[:N_RECT].copy() if full.size >= N_RECT else np.cumsum(rng.uniform(0.9, 1.1, N_RECT))
        lo, hi = float(t[0]), float(t[-1])
        beyond = NS // 10
        ts = np.concatenate([lo - rng.uniform(0.0, 0.1 * (hi - lo), beyond), hi + rng.uniform(0.0, 0.1 * (hi - lo), beyond),
                             rng.uniform(lo, hi, NS - 2 * beyond)])
        ts = rng.permutation(ts)
        for i, n in COINCIDE:
            ts[i] = t[n]
        ts[TWINS[1]] = ts[TWINS[0]]
        out[reg] = (t, ts)
    return out


def rect_sample(t, ts, seed):
    rng = np.random.default_rng(seed)
    seen, out = set(), []

    def add(i, j):
        if (i, j) not in seen:
            seen.add((i, j))
            out.append((i, j))
    for i in range(RECT_CORNER):
        for j in range(RECT_CORNER):
            add(i, j)
    for i, j in zip(*np.nonzero(ts[:, None] == t[None, :])):
        add(int(i), int(j))
    for j in (0, t.size - 1, int(rng.integers(0, t.size))):
        add(ts.size - 1, j)
    for i in (0, ts.size - 1, int(rng.integers(0, ts.size))):
        add(i, t.size - 1)
    while len(out) < RECT_SAMPLES:
        add(int(rng.integers(0, ts.size)), int(rng.integers(0, t.size)))
    return np.array(out[:RECT_SAMPLES], dtype=np.int64)


class _Evaluator:
    """Values, condition numbers and parameter derivatives of one case's program, cached per (r, diag, nugget)."""

    def __init__(self, expr):
        import mpmath
        self.mp = mp = mpmath.mp
        mp.dps = DPS
        self.A = kf.mp_arith(mp)
        ops, pars = build_kernel(expr)._device_program()
        self.ops = [tuple(int(v) for v in o) for o in ops]
        self.pars = [float(v) for v in pars]
        self.P = [mp.mpf(v) for v in self.pars]
        self.has_nan = any(v != v for v in self.pars)
        self._value, self._dk = {}, {}

    def _f(self, diag, nug):
        c = self.mp.mpf(nug)
        return lambda xs: cf.program(self.A, self.ops, xs[1:], xs[0], 0, diag) + c

    def value(self, a, b, diag, nug=0.0):
        """(hi, lo, kappa) of k(a, b) + nug"""
        mp = self.mp
        r = mp.mpf(float(a)) - mp.mpf(float(b))
        key = (r, diag, nug)
        if key not in self._value:
            f, xs = self._f(diag, nug), [r] + self.P
            v = f(xs)
            self._value[key] = sq._split(mp, v) + (sq._kappa(mp, f, xs, v),)
        return self._value[key]

    def dk(self, a, b, diag):
        """[d k / d par[l]] rounded to double"""
        mp = self.mp
        r = mp.mpf(float(a)) - mp.mpf(float(b))
        key = (r, diag)
        if key not in self._dk:
            out = []
            for l in range(len(self.P)):
                g = lambda p: cf.program(self.A, self.ops, self.P[:l] + [p] + self.P[l + 1:], r, 0, diag)   # noqa: E731
                out.append(float(mp.diff(g, self.P[l])))
            self._dk[key] = out
        return self._dk[key]


def evaluate_case(case, t, rect):
    ev = _Evaluator(case['expr'])
    seed = zlib.crc32(case['name'].encode())
    idx = square_sample(t, seed)
    val = [ev.value(t[i], t[j], bool(i == j)) for i, j in idx]
    col = lambda rows, c, dt: np.array([r[c] for r in rows], dtype=dt)              # noqa: E731
    res = dict(ops=ev.ops, pars=ev.pars, i=idx[:, 0], j=idx[:, 1], hi=col(val, 0, float), lo=col(val, 1, np.float32),
               kappa=col(val, 2, np.float32))
    if not ev.has_nan and case['name'] not in DK_DROPPED:
        res['dk'] = np.array([ev.dk(t[i], t[j], bool(i == j)) for i, j in idx]).T.copy()
    tr, ts = rect
    ridx = rect_sample(tr, ts, seed + 1)
    ref = [ev.value(ts[i], tr[j], False) for i, j in ridx]
    co_k = [k for k, (i, j) in enumerate(ridx) if ts[i] == tr[j]]
    co = [ev.value(ts[ridx[k][0]], tr[ridx[k][1]], True, SETUP_NUGGET) for k in co_k]
    kss = [ev.value(v, v, True, TINY_NUGGET) for v in ts] + [ev.value(v, v, True, SETUP_NUGGET) for v in ts]
    res.update(rect_i=ridx[:, 0], rect_j=ridx[:, 1], rect_hi=col(ref, 0, float), rect_lo=col(ref, 1, np.float32),
               rect_kappa=col(ref, 2, np.float32), rect_co_k=np.array(co_k, dtype=np.int64),
               rect_co_hi=col(co, 0, float), rect_co_lo=col(co, 1, np.float32), rect_co_kappa=col(co, 2, np.float32),
               rect_kss_hi=col(kss, 0, float), rect_kss_lo=col(kss, 1, np.float32), rect_kss_kappa=col(kss, 2, np.float32))
    return res


SQUARE_KEYS = ('i', 'j', 'hi', 'lo', 'kappa')
RECT_KEYS = tuple('rect_' + k for k in SQUARE_KEYS)
CO_KEYS = ('rect_co_k', 'rect_co_hi', 'rect_co_lo', 'rect_co_kappa')
KSS_KEYS = ('rect_kss_hi', 'rect_kss_lo', 'rect_kss_kappa')


def generate(only=None):
    """(meta, arrays) of the fixture, or of the cases named in `only`."""
    sets, rsets = sq.time_sets(), rect_time_sets()
    meta, cols = [], {}
    off = dk_off = rect_off = co_off = kss_off = 0
    for case in case_list():
        if only is not None and case['name'] not in only:
            continue
        res = evaluate_case(case, sets[case['tset']], rsets[case['tset']])
        n, rn, co_n = res['hi'].size, res['rect_hi'].size, res['rect_co_hi'].size
        has_dk = 'dk' in res
        meta.append(dict(case, ops=res['ops'], pars=res['pars'], nugget=True, off=off, n=n,
                         dk_off=dk_off if has_dk else None,
                         rect=dict(off=rect_off, n=rn, co_off=co_off, co_n=co_n, kss_off=kss_off)))
        for key in SQUARE_KEYS + RECT_KEYS + CO_KEYS + KSS_KEYS:
            cols.setdefault(key, []).append(res[key])
        if has_dk:
            cols.setdefault('dk', []).append(res['dk'].ravel())
            dk_off += res['dk'].size
        off, rect_off, co_off, kss_off = off + n, rect_off + rn, co_off + co_n, kss_off + 2 * NS
        print('%-28s %3d + %3d elements' % (case['name'], n, rn), flush=True)
    arrays = {}
    for reg in ('R1', 'R2', 'R3'):
        arrays['t_' + reg] = sets[reg]
        arrays['rect_t_' + reg], arrays['rect_ts_' + reg] = rsets[reg]
    for key, parts in cols.items():
        a = np.concatenate(parts)
        arrays[key] = a.astype(np.uint8) if key in ('i', 'j', 'rect_i', 'rect_j', 'rect_co_k') else a
    return meta, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*')
    ap.add_argument('--out', default=GOLDEN)
    a = ap.parse_args()
    meta, arrays = generate(a.only)
    os.makedirs(a.out, exist_ok=True)
    sq._write_npz(os.path.join(a.out, 'celerite_highprec.npz'), arrays)
    with open(os.path.join(a.out, 'celerite_highprec.json'), 'w') as f:
        json.dump({'dps': DPS, 'max_samples': MAX_SAMPLES, 'n_rect': N_RECT, 'ns': NS, 'tiny_nugget': TINY_NUGGET,
                   'setup_nugget': SETUP_NUGGET, 'cases': meta}, f, indent=0)
    print('%d cases, %d + %d elements -> %s' % (len(meta), arrays['hi'].size, arrays['rect_hi'].size, a.out))


if __name__ == '__main__':
    main()
