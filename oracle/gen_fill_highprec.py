"""High-precision reference of the covariance fill: tests/golden/fill_highprec.{npz,json}.

Every built-in kernel, the composites and derivatives of kernels.json and one composite seven stack slots deep, each
over the regimes that apply to it (R1 typical, R2 absolute times in BJD with repeated stamps, R3 length scales far
below the sampling -- exponents through -700 ... -800 and past them --, R4 length scales far above the span and
RationalQuadratic at alpha = 1e8, R5 periods so short that pi |r| / P reaches 1e3, 1e6, 1e9 and 1e12, R6 degenerate
parameters: ell^2 subnormal, an overflowing quotient, NaN).  For a fixed sample of each case's elements (the lower
triangle of the 16 x 16 corner, the diagonal, seeded random pairs; 500 at most, the fixture stays below 1 MiB):

* ``hi`` + ``lo``: the exact kernel value at the (double) inputs as a double-double (lo in float32: 2^-77 from exact);
* ``kappa``: its elementwise condition number sum_u |u dk/du| / |k| over u in {r (t_i and t_j for the kernels that
  read them), every parameter} -- and, for the rational-quadratic and harmonic forms, the intermediates their formula
  rounds and then raises to the power alpha or lets cancel (kernel_formulas.N_INTERMEDIATES) --, float32;
* for the one-kernel SquaredExponential, Periodic and QuasiPeriodic cases -- the kernels whose fill follows NumPy's
  rounding sequence (csrc/fill.hip: div_rn, sin_sq_rad, exp_neg) -- also ``seq_hi``/``seq_lo``/``seq_kappa``: the exact
  value once NumPy's own rounded intermediates are given, i.e. exp of NumPy's rounded exponent (SE), of
  -2 sin^2(Phi) / ell^2 with NumPy's rounded phase Phi = pi |r| / P (Periodic), of -2 sin^2(Phi) / lp^2 - D with the
  rounded phase and NumPy's rounded decay D = r^2 / (2 le^2) (QP); its condition number is taken with those
  intermediates held (theta, ell or lp, and D), so the bound is a few ulp at any phase.

mpmath at 40 digits; needs neither the reference project nor a GPU.  Usage: python oracle/gen_fill_highprec.py
[--only NAME ...] [--out DIR]."""
import argparse
import io
import json
import os
import sys
import zipfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gpyrn_amd import covfunc  # noqa: E402
from oracle import kernel_formulas as kf  # noqa: E402

DPS = 40
DELTA = '1e-15'                      # relative step of the condition numbers' differences (at 40 digits: ~25 digits)
CORNER = 16
MAX_SAMPLES = 500
SPAN = 60.0


def time_sets():
    rng = np.random.default_rng(20261016)
    t1 = np.sort(rng.uniform(0.0, SPAN, 200))
    t2 = 2.45e6 + np.sort(rng.uniform(0.0, 3000.0, 200))
    for k in (17, 60, 61, 133, 170):                      # repeated time stamps: r = 0 off the diagonal
        t2[k + 1] = t2[k]
    t3 = np.cumsum(rng.uniform(0.9, 1.1, 120))            # median spacing ~1
    t5 = np.sort(rng.uniform(0.0, SPAN, 48))
    t6 = 2.45e6 + np.sort(rng.uniform(0.0, 3000.0, 64))
    t6[11] = t6[10]
    return {'R1': t1, 'R2': t2, 'R3': t3, 'R5': t5, 'R6': t6}


def _period(x):
    """P such that pi |r| / P reaches x over the span."""
    return float(np.pi * SPAN / x)


PHASES = (1e3, 1e6, 1e9, 1e12)
nan = float('nan')

# kernel -> {regime: [parameter tuples]}; R5 entries are functions of the period
TABLE = [
    ('Constant', {'R1': [(1.3,)], 'R2': [(1.3,)]}),
    ('WhiteNoise', {'R1': [(0.7,)], 'R2': [(0.7,)]}),
    ('SquaredExponential', {'R1': [(1.2, 7.5)], 'R2': [(1.2, 300.0)], 'R3': [(1.2, 0.026)],
                            'R4': [(1.2, 6e4), (1.2, 6e7)],
                            'R6': [(1.0, 1e-160), (2.0, 1e-152), (nan, 7.5), (1.0, nan)]}),
    ('Periodic', {'R1': [(0.9, 11.0, 0.8)], 'R2': [(0.9, 400.0, 0.8)], 'R3': [(0.9, 11.0, 0.05)],
                  'R4': [(0.9, 6e4, 0.8), (0.9, 11.0, 1e5)], 'R5': lambda P: (0.9, P, 0.8),
                  'R6': [(1.0, 11.0, 1e-160), (1.0, nan, 0.8)]}),
    ('QuasiPeriodic', {'R1': [(1.1, 30.0, 12.5, 0.6)], 'R2': [(1.1, 1500.0, 400.0, 0.6)],
                       'R3': [(1.1, 0.026, 12.5, 0.05)], 'R4': [(1.1, 6e4, 12.5, 0.6)],
                       'R5': lambda P: (1.1, 30.0, P, 0.6),
                       'R6': [(1.0, 1e-160, 11.0, 1e-160), (2.0, 1e-152, 11.0, 0.6), (1.0, 30.0, 12.5, nan)]}),
    ('RationalQuadratic', {'R1': [(1.4, 0.8, 9.0)], 'R2': [(1.4, 0.8, 400.0)], 'R3': [(1.4, 0.8, 0.026)],
                           'R4': [(1.4, 1e8, 9.0), (1.4, 0.8, 6e4)], 'R6': [(1.0, nan, 9.0)]}),
    ('RQP', {'R1': [(1.2, 0.9, 20.0, 13.0, 0.7)], 'R2': [(1.2, 0.9, 1000.0, 450.0, 0.7)],
             'R3': [(1.2, 0.9, 0.026, 13.0, 0.05)], 'R4': [(1.2, 1e8, 20.0, 13.0, 0.7)],
             'R5': lambda P: (1.2, 0.9, 20.0, P, 0.7)}),
    ('Cosine', {'R1': [(0.8, 9.5)], 'R2': [(0.8, 450.0)], 'R4': [(0.8, 6e4)], 'R5': lambda P: (0.8, P)}),
    ('Exponential', {'R1': [(1.1, 6.0)], 'R2': [(1.1, 300.0)], 'R3': [(1.1, 0.0013)], 'R4': [(1.1, 6e4)]}),
    ('Matern32', {'R1': [(1.3, 8.0)], 'R2': [(1.3, 400.0)], 'R3': [(1.3, 0.0023)], 'R4': [(1.3, 6e4)],
                  'R6': [(1.0, nan)]}),
    ('Matern52', {'R1': [(0.7, 5.0)], 'R2': [(0.7, 250.0)], 'R3': [(0.7, 0.003)], 'R4': [(0.7, 6e4)]}),
    ('GammaExp', {'R1': [(1.2, 1.5, 6.0)], 'R2': [(1.2, 1.5, 300.0)], 'R3': [(1.2, 1.5, 0.012)],
                  'R4': [(1.2, 1.5, 6e4)]}),
    ('Piecewise', {'R1': [(14.0,)], 'R2': [(700.0,)], 'R3': [(2.2,)], 'R4': [(6e4,)]}),
    ('Paciorek', {'R1': [(1.1, 5.0, 9.0)], 'R2': [(1.1, 250.0, 450.0)], 'R3': [(1.1, 0.03, 0.05)],
                  'R4': [(1.1, 6e4, 9e4)]}),
    ('NewPeriodic', {'R1': [(1.2, 0.9, 10.0, 0.8)], 'R2': [(1.2, 0.9, 450.0, 0.8)], 'R3': [(1.2, 0.9, 10.0, 0.01)],
                     'R4': [(1.2, 0.9, 6e4, 0.8)], 'R5': lambda P: (1.2, 0.9, P, 0.8)}),
    ('QuasiNewPeriodic', {'R1': [(1.1, 0.7, 25.0, 10.0, 0.9)], 'R2': [(1.1, 0.7, 1250.0, 450.0, 0.9)],
                          'R3': [(1.1, 0.7, 0.026, 10.0, 0.01)], 'R4': [(1.1, 0.7, 6e4, 10.0, 0.9)],
                          'R5': lambda P: (1.1, 0.7, 25.0, P, 0.9)}),
    ('CosPeriodic', {'R1': [(1.3, 11.0, 0.9)], 'R2': [(1.3, 450.0, 0.9)], 'R3': [(1.3, 11.0, 0.05)],
                     'R4': [(1.3, 6e4, 0.9)], 'R5': lambda P: (1.3, P, 0.9)}),
    ('QuasiCosPeriodic', {'R1': [(0.9, 22.0, 9.0, 0.8)], 'R2': [(0.9, 1100.0, 450.0, 0.8)],
                          'R3': [(0.9, 0.026, 9.0, 0.05)], 'R4': [(0.9, 6e4, 9.0, 0.8)],
                          'R5': lambda P: (0.9, 22.0, P, 0.8)}),
    ('Polynomial', {'R1': [(1.0, 0.01, 1.5, 2.0)], 'R2': [(1.0, 0.01, 1.5, 2.0)]}),
    ('HarmonicPeriodic', {'R1': [(2, 1.1, 13.0, 0.9)], 'R2': [(2, 1.1, 450.0, 0.9)], 'R3': [(2, 1.1, 13.0, 0.02)],
                          'R5': lambda P: (2, 1.1, P, 0.9)}),
    ('QuasiHarmonicPeriodic', {'R1': [(2, 1.2, 25.0, 11.0, 0.8)], 'R2': [(2, 1.2, 1250.0, 450.0, 0.8)],
                               'R3': [(2, 1.2, 0.026, 11.0, 0.02)], 'R5': lambda P: (2, 1.2, 25.0, P, 0.8)}),
]

# expressions over c = covfunc; '{P}' is the R5 period
EXPRS = [
    ('dSE', {'R1': 'c.Derivative(c.SquaredExponential(1.2, 6.0))', 'R2': 'c.Derivative(c.SquaredExponential(1.2, 300.0))',
             'R3': 'c.Derivative(c.SquaredExponential(1.2, 0.026))', 'R4': 'c.Derivative(c.SquaredExponential(1.2, 6e4))'}),
    ('dP', {'R1': 'c.Derivative(c.Periodic(0.9, 11.0, 0.8))', 'R2': 'c.Derivative(c.Periodic(0.9, 450.0, 0.8))',
            'R3': 'c.Derivative(c.Periodic(0.9, 11.0, 0.05))', 'R5': 'c.Derivative(c.Periodic(0.9, {P}, 0.8))'}),
    ('dQP', {'R1': 'c.Derivative(c.QuasiPeriodic(1.1, 30.0, 12.5, 0.6))',
             'R2': 'c.Derivative(c.QuasiPeriodic(1.1, 1500.0, 450.0, 0.6))',
             'R3': 'c.Derivative(c.QuasiPeriodic(1.1, 0.026, 12.5, 0.05))',
             'R4': 'c.Derivative(c.QuasiPeriodic(1.1, 6e4, 12.5, 0.6))',
             'R5': 'c.Derivative(c.QuasiPeriodic(1.1, 30.0, {P}, 0.6))'}),
    ('SE_plus_M32', {'R1': 'c.SquaredExponential(1.1, 8.0) + c.Matern32(0.4, 3.0)',
                     'R2': 'c.SquaredExponential(1.1, 400.0) + c.Matern32(0.4, 150.0)'}),
    ('SE_times_P', {'R1': 'c.SquaredExponential(1.0, 10.0) * c.Periodic(1.0, 20.0, 0.5)',
                    'R2': 'c.SquaredExponential(1.0, 500.0) * c.Periodic(1.0, 1000.0, 0.5)',
                    'R5': 'c.SquaredExponential(1.0, 10.0) * c.Periodic(1.0, {P}, 0.5)'}),
    ('sum_of_prod', {'R1': 'c.SquaredExponential(0.9, 12.0) * c.Periodic(1.0, 7.0, 0.9) + c.Exponential(0.3, 4.0)',
                     'R2': 'c.SquaredExponential(0.9, 600.0) * c.Periodic(1.0, 350.0, 0.9) + c.Exponential(0.3, 200.0)'}),
    # right-nested: seven values on the program's stack at once
    ('deep7', {'R1': 'c.Constant(0.5) + c.SquaredExponential(1.1, 8.0) * (c.Periodic(0.9, 11.0, 0.8) + '
                     'c.Matern52(0.8, 5.0) * (c.Exponential(0.6, 9.0) + c.RationalQuadratic(1.2, 0.8, 9.0) * '
                     'c.Cosine(0.7, 13.0)))',
               'R2': 'c.Constant(0.5) + c.SquaredExponential(1.1, 400.0) * (c.Periodic(0.9, 450.0, 0.8) + '
                     'c.Matern52(0.8, 250.0) * (c.Exponential(0.6, 450.0) + c.RationalQuadratic(1.2, 0.8, 450.0) * '
                     'c.Cosine(0.7, 650.0)))'}),
]
SEQ_KERNELS = ('SquaredExponential', 'Periodic', 'QuasiPeriodic')


def _fmt(v):
    return 'nan' if v != v else repr(float(v))


def cases():
    out = []
    for name, regs in TABLE:
        for reg in ('R1', 'R2', 'R3', 'R4', 'R5', 'R6'):
            if reg not in regs:
                continue
            sets = [regs[reg](_period(x)) for x in PHASES] if reg == 'R5' else regs[reg]
            for k, pars in enumerate(sets):
                expr = 'c.%s(%s)' % (name, ', '.join(_fmt(v) for v in pars))
                out.append(dict(name='%s_%s_%d' % (name, reg, k), kernel=name, regime=reg,
                                tset='R1' if reg == 'R4' else reg, expr=expr, seq=name in SEQ_KERNELS))
    for name, regs in EXPRS:
        for reg in ('R1', 'R2', 'R3', 'R4', 'R5'):
            if reg not in regs:
                continue
            exprs = [regs[reg].replace('{P}', repr(_period(x))) for x in PHASES[:3]] if reg == 'R5' else [regs[reg]]
            for k, expr in enumerate(exprs):
                out.append(dict(name='%s_%s_%d' % (name, reg, k), kernel=name, regime=reg,
                                tset='R1' if reg == 'R4' else reg, expr=expr, seq=False))
    return out


def build_kernel(expr):
    return eval(expr, {'c': covfunc, 'nan': float('nan')})


def sample(N, seed):
    rng = np.random.default_rng(seed)
    seen, out = set(), []

    def add(i, j):
        if (i, j) not in seen:
            seen.add((i, j))
            out.append((i, j))
    for i in range(min(CORNER, N)):
        for j in range(i + 1):
            add(i, j)
    for i in range(N):
        add(i, i)
    while len(out) < MAX_SAMPLES and len(seen) < N * N:
        i, j = (int(v) for v in rng.integers(0, N, 2))
        add(i, j)
    return np.array(out[:MAX_SAMPLES], dtype=np.int64)


def _split(mp, v):
    """double-double (hi, lo as float32) of an mpf; NaN -> (nan, 0)."""
    if mp.isnan(v):
        return float('nan'), 0.0
    hi = float(v)
    if not np.isfinite(hi):
        return hi, 0.0
    return hi, float(np.float32(float(v - mp.mpf(hi))))


def _kappa(mp, f, xs, f0):
    """sum_u |u df/du| / |f| by central differences of relative step DELTA."""
    if mp.isnan(f0):
        return float('nan')
    if f0 == 0:
        return 0.0
    d = mp.mpf(DELTA)
    tot = mp.mpf(0)
    for k, x in enumerate(xs):
        if x == 0 or mp.isnan(x):
            continue
        up, dn = list(xs), list(xs)
        up[k], dn[k] = x * (1 + d), x * (1 - d)
        tot += abs(f(up) - f(dn)) / (2 * d)
    v = float(tot / abs(f0))
    return float(np.float32(v)) if np.isfinite(v) else float('inf')


def evaluate_case(case, t):
    import mpmath
    mp = mpmath.mp
    mp.dps = DPS
    A = kf.mp_arith(mp)
    k = build_kernel(case['expr'])
    ops, pars = k._device_program()
    ops = [tuple(int(v) for v in o) for o in ops]
    pars = [float(v) for v in pars]
    two = kf.uses_t(ops)
    idx = sample(t.size, zlib.crc32(case['name'].encode()))
    P = [mp.mpf(v) for v in pars]
    npar = len(P)
    nint = kf.N_INTERMEDIATES.get(ops[0][1], 0) if len(ops) == 1 else 0
    ones = [mp.mpf(1)] * 10
    hi, lo, kap = [], [], []
    shi, slo, skap = [], [], []
    for i, j in idx:
        ti, tj = mp.mpf(float(t[i])), mp.mpf(float(t[j]))
        diag = bool(i == j)
        # variables of the condition number: r (or t_i, t_j), the parameters, a one-kernel formula's intermediates
        if two:
            f = lambda xs: kf.program(A, ops, xs[2:2 + npar], xs[0], xs[1], diag, xs[2 + npar:] + ones)  # noqa: E731
            xs = [ti, tj] + P + [mp.mpf(1)] * nint
        else:
            f = lambda xs: kf.program(A, ops, xs[1:1 + npar], xs[0], 0, diag, xs[1 + npar:] + ones)      # noqa: E731
            xs = [ti - tj] + P + [mp.mpf(1)] * nint
        v = f(xs)
        h, l_ = _split(mp, v)
        hi.append(h)
        lo.append(l_)
        kap.append(_kappa(mp, f, xs, v))
        if case['seq']:
            v, g, ys = _seq(mp, A, case['kernel'], pars, float(t[i]) - float(t[j]))
            h, l_ = _split(mp, v)
            shi.append(h)
            slo.append(l_)
            skap.append(_kappa(mp, g, ys, v))
    res = dict(i=idx[:, 0], j=idx[:, 1], hi=np.array(hi), lo=np.array(lo, dtype=np.float32),
               kappa=np.array(kap, dtype=np.float32), ops=ops, pars=pars)
    if case['seq']:
        res.update(seq_hi=np.array(shi), seq_lo=np.array(slo, dtype=np.float32),
                   seq_kappa=np.array(skap, dtype=np.float32))
    return res


def _seq(mp, A, name, q, r):
    """The exact value given NumPy's rounded intermediates (module docstring); returns (value, f, variables)."""
    r = np.float64(r)
    with np.errstate(all='ignore'):                         # (R6: NumPy's quotient overflows as the fill's does)
        return _seq_at(mp, name, q, r)


def _seq_at(mp, name, q, r):
    if name == 'SquaredExponential':
        X = mp.mpf(float(-0.5 * r**2 / np.float64(q[1])**2))
        f = lambda xs: xs[0] ** 2 * mp.exp(X)                                   # noqa: E731
        ys = [mp.mpf(q[0])]
    elif name == 'Periodic':
        s2 = mp.sin(mp.mpf(float(np.pi * np.abs(r) / np.float64(q[1])))) ** 2
        f = lambda xs: xs[0] ** 2 * mp.exp(-2 * s2 / xs[1] ** 2)                # noqa: E731
        ys = [mp.mpf(q[0]), mp.mpf(q[2])]
    else:
        s2 = mp.sin(mp.mpf(float(np.pi * np.abs(r) / np.float64(q[2])))) ** 2
        D = mp.mpf(float(r**2 / (2 * np.float64(q[1])**2)))
        f = lambda xs: xs[0] ** 2 * mp.exp(-2 * s2 / xs[1] ** 2 - xs[2])       # noqa: E731
        ys = [mp.mpf(q[0]), mp.mpf(q[3]), D]
    return f(ys), f, ys


def _write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            zi = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def generate(only=None):
    """(meta, arrays) of the fixture, or of the cases named in `only`."""
    ts = time_sets()
    meta, cols = [], {}
    off = soff = 0
    for case in cases():
        if only is not None and case['name'] not in only:
            continue
        res = evaluate_case(case, ts[case['tset']])
        n = res['hi'].size
        entry = dict(case, ops=res['ops'], pars=res['pars'], off=off, n=n, seq_off=soff if case['seq'] else None)
        meta.append(entry)
        for key in ('i', 'j', 'hi', 'lo', 'kappa', 'seq_hi', 'seq_lo', 'seq_kappa'):
            if key in res:
                cols.setdefault(key, []).append(res[key])
        off += n
        soff += n if case['seq'] else 0
    arrays = {'t_' + k: v for k, v in ts.items()}
    for key, parts in cols.items():
        a = np.concatenate(parts)
        arrays[key] = a.astype(np.uint8) if key in ('i', 'j') else a
    return meta, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    meta, arrays = generate(a.only)
    os.makedirs(a.out, exist_ok=True)
    _write_npz(os.path.join(a.out, 'fill_highprec.npz'), arrays)
    with open(os.path.join(a.out, 'fill_highprec.json'), 'w') as f:
        json.dump({'dps': DPS, 'corner': CORNER, 'max_samples': MAX_SAMPLES, 'cases': meta}, f, indent=0)
    print('%d cases, %d elements -> %s' % (len(meta), arrays['hi'].size, a.out))


if __name__ == '__main__':
    main()
