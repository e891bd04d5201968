"""High-precision reference of the rectangular fills of prediction, K* and k**: tests/golden/rect_highprec.{npz,json}.

The kernels, regimes and parameters are those of the square fixture (gen_fill_highprec: TABLE, EXPRS, R1 ... R6), so both
cover the same cases.  Per time set one data set t (N = 200) and, a draw of its own, ns = 137 prediction times t* in no
order: a tenth below the data's span, a tenth above it, the rest inside; ten of them bit-equal to data times (among
them the first and the last data time, and the pairs (t*_3, t_5), (t*_5, t_3) inside the corner: a transposed index
shows), two equal to each other.  R2 and R6 are absolute times in BJD; R2's data carry one repeated stamp, which a t*
coincides with.

What the two forms of prediction compute (include/gprn_hip.h "predict_form", DESIGN.md 9 f-2, csrc/fill.hip k_fill_rect):

* reference form: K*[i][n] = k(t*_i, t_n) evaluated OFF the diagonal everywhere -- no nugget and no WhiteNoise, also where
  t*_i == t_n --, k**[i] = k(t*_i, t*_i) on the diagonal + 1.25e-12, the nugget left out for the kernels that take none
  (Polynomial, HarmonicPeriodic, QuasiHarmonicPeriodic);
* posterior form: the nugget (the set-up's 1e-6, with the same exceptions) and WhiteNoise are delta(t, t'): in K* exactly where
  t*_i == t_n as doubles, in k** always.  Elsewhere K* is the reference form's.

Recorded per case, in the encoding of the square fixture (``hi`` + ``lo`` the exact value as a double-double, ``kappa`` the
element's condition number over r or (t_i, t_j), the parameters and kernel_formulas.N_INTERMEDIATES; a nugget is a constant
of the sum):

* ``i``, ``j``, ``hi``, ``lo``, ``kappa``: the reference form at a sample of at most 300 elements of K* -- the 16 x 16 corner,
  every coincident pair, a dozen elements each of the last row and the last column (both ends among them), seeded random ones;
* ``co_k``, ``co_hi``, ``co_lo``, ``co_kappa``: the posterior form where it differs, at the coincident pairs (co_k: the
  element's position in the case's sample);
* ``kss_hi``, ``kss_lo``, ``kss_kappa``: all of k**, the reference form's ns values, then the posterior form's.

mpmath at 40 digits; needs neither the reference project nor a GPU.  Usage: python oracle/gen_rect_highprec.py
[--only NAME ...] [--out DIR]."""
import argparse
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gen_fill_highprec as sq  # noqa: E402
from oracle import kernel_formulas as kf  # noqa: E402

DPS = sq.DPS
CORNER = 16
MAX_SAMPLES = 300
EDGE = 12                            # elements of the last row, and of the last column
N, NS = 200, 137
TINY_NUGGET = 1.25e-12               # _gp.py:47, the reference form's k**
SETUP_NUGGET = 1e-6                  # csrc/gprn_internal.h GPRN_SETUP_NUGGET, the posterior form
NO_NUGGET = ('Polynomial', 'HarmonicPeriodic', 'QuasiHarmonicPeriodic')
# (row of t*, column of t) made bit-equal; and the two rows of t* made equal to each other
COINCIDE = ((3, 5), (5, 3), (9, 12), (40, 0), (41, 60), (77, 128), (100, 127), (120, 150), (130, 64), (136, 199))
TWINS = (20, 88)


def _tstar(rng, t):
    lo, hi = float(t[0]), float(t[-1])
    out = NS // 10 + 1
    ts = np.concatenate([lo - rng.uniform(0.0, 0.1 * (hi - lo), out), hi + rng.uniform(0.0, 0.1 * (hi - lo), out),
                         rng.uniform(lo, hi, NS - 2 * out)])
    ts = rng.permutation(ts)
    # (the rows rewritten below give up times inside the span: the tenths beyond its ends stay whole)
    special = [i for i, _ in COINCIDE] + [TWINS[1]]
    free = [i for i in range(NS) if i not in special and i != TWINS[0] and lo < ts[i] < hi]
    for i in special:
        if not lo < ts[i] < hi:
            k = free.pop(0)
            ts[i], ts[k] = ts[k], ts[i]
    for i, n in COINCIDE:
        ts[i] = t[n]
    ts[TWINS[1]] = ts[TWINS[0]]
    return ts


def time_sets():
    """{regime: (t, t*)}"""
    rng = np.random.default_rng(20261020)
    out = {}
    for reg in ('R1', 'R2', 'R3', 'R5', 'R6'):
        if reg in ('R2', 'R6'):
            t = 2.45e6 + np.sort(rng.uniform(0.0, 3000.0, N))
        elif reg == 'R3':
            t = np.cumsum(rng.uniform(0.9, 1.1, N))       # median spacing ~1
        else:
            t = np.sort(rng.uniform(0.0, sq.SPAN, N))
        if reg == 'R2':
            t[61] = t[60]                                 # a repeated stamp: t*_41 coincides with two columns
        out[reg] = (t, _tstar(rng, t))
    return out


def coincident(t, ts):
    """the pairs (i, n) with t*_i == t_n, in row-major order"""
    return [(int(i), int(n)) for i, n in zip(*np.nonzero(ts[:, None] == t[None, :]))]


def sample(t, ts, seed):
    rng = np.random.default_rng(seed)
    seen, out = set(), []

    def add(i, j):
        if (i, j) not in seen:
            seen.add((i, j))
            out.append((i, j))
    for i in range(CORNER):
        for j in range(CORNER):
            add(i, j)
    for i, j in coincident(t, ts):
        add(i, j)
    for j in [0, t.size - 1] + [int(v) for v in rng.integers(0, t.size, EDGE - 2)]:
        add(ts.size - 1, j)
    for i in [0, ts.size - 1] + [int(v) for v in rng.integers(0, ts.size, EDGE - 2)]:
        add(i, t.size - 1)
    while len(out) < MAX_SAMPLES:
        add(int(rng.integers(0, ts.size)), int(rng.integers(0, t.size)))
    return np.array(out[:MAX_SAMPLES], dtype=np.int64)


def evaluate_case(case, t, ts):
    import mpmath
    mp = mpmath.mp
    mp.dps = DPS
    A = kf.mp_arith(mp)
    k = sq.build_kernel(case['expr'])
    ops, pars = k._device_program()
    ops = [tuple(int(v) for v in o) for o in ops]
    pars = [float(v) for v in pars]
    two = kf.uses_t(ops)
    nugget = case['kernel'] not in NO_NUGGET
    P = [mp.mpf(v) for v in pars]
    npar = len(P)
    nint = kf.N_INTERMEDIATES.get(ops[0][1], 0) if len(ops) == 1 else 0
    ones = [mp.mpf(1)] * 10
    at_zero = {}                         # a kernel in r alone between equal times: one evaluation per (diag, nugget)

    def element(a, b, diag, nug):
        """(hi, lo, kappa) of k(a, b) + nug"""
        key = (diag, nug)
        if not two and a == b and key in at_zero:
            return at_zero[key]
        ti, tj, c = mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(nug)
        if two:
            f = lambda xs: kf.program(A, ops, xs[2:2 + npar], xs[0], xs[1], diag, xs[2 + npar:] + ones) + c  # noqa: E731
            xs = [ti, tj] + P + [mp.mpf(1)] * nint
        else:
            f = lambda xs: kf.program(A, ops, xs[1:1 + npar], xs[0], 0, diag, xs[1 + npar:] + ones) + c      # noqa: E731
            xs = [ti - tj] + P + [mp.mpf(1)] * nint
        v = f(xs)
        res = sq._split(mp, v) + (sq._kappa(mp, f, xs, v),)
        if not two and a == b:
            at_zero[key] = res
        return res

    idx = sample(t, ts, zlib.crc32(case['name'].encode()))
    ref = [element(ts[i], t[j], False, 0.0) for i, j in idx]
    post_nug = SETUP_NUGGET if nugget else 0.0
    co_k = [k_ for k_, (i, j) in enumerate(idx) if ts[i] == t[j]]
    co = [element(ts[idx[k_][0]], t[idx[k_][1]], True, post_nug) for k_ in co_k]
    kss = [element(v, v, True, TINY_NUGGET if nugget else 0.0) for v in ts]
    kss += [element(v, v, True, post_nug) for v in ts]
    col = lambda rows, c, dt: np.array([r[c] for r in rows], dtype=dt)              # noqa: E731
    return dict(ops=ops, pars=pars, nugget=nugget, i=idx[:, 0], j=idx[:, 1],
                hi=col(ref, 0, float), lo=col(ref, 1, np.float32), kappa=col(ref, 2, np.float32),
                co_k=np.array(co_k, dtype=np.int64), co_hi=col(co, 0, float), co_lo=col(co, 1, np.float32),
                co_kappa=col(co, 2, np.float32),
                kss_hi=col(kss, 0, float), kss_lo=col(kss, 1, np.float32), kss_kappa=col(kss, 2, np.float32))


KEYS = ('i', 'j', 'hi', 'lo', 'kappa')
CO_KEYS = ('co_k', 'co_hi', 'co_lo', 'co_kappa')
KSS_KEYS = ('kss_hi', 'kss_lo', 'kss_kappa')


def generate(only=None):
    """(meta, arrays) of the fixture, or of the cases named in `only`."""
    sets = time_sets()
    meta, cols = [], {}
    off = co_off = kss_off = 0
    for case in sq.cases():
        if only is not None and case['name'] not in only:
            continue
        case = {k: v for k, v in case.items() if k != 'seq'}
        res = evaluate_case(case, *sets[case['tset']])
        n, co_n = res['hi'].size, res['co_hi'].size
        meta.append(dict(case, ops=res['ops'], pars=res['pars'], nugget=res['nugget'], off=off, n=n, co_off=co_off,
                         co_n=co_n, kss_off=kss_off))
        for key in KEYS + CO_KEYS + KSS_KEYS:
            cols.setdefault(key, []).append(res[key])
        off, co_off, kss_off = off + n, co_off + co_n, kss_off + 2 * NS
    arrays = {}
    for reg, (t, ts) in sets.items():
        arrays['t_' + reg], arrays['ts_' + reg] = t, ts
    for key, parts in cols.items():
        a = np.concatenate(parts)
        arrays[key] = a.astype(np.uint8) if key in ('i', 'j') else a.astype(np.uint16) if key == 'co_k' else a
    return meta, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', nargs='*')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    meta, arrays = generate(a.only)
    os.makedirs(a.out, exist_ok=True)
    sq._write_npz(os.path.join(a.out, 'rect_highprec.npz'), arrays)
    with open(os.path.join(a.out, 'rect_highprec.json'), 'w') as f:
        json.dump({'dps': DPS, 'corner': CORNER, 'max_samples': MAX_SAMPLES, 'ns': NS, 'tiny_nugget': TINY_NUGGET,
                   'setup_nugget': SETUP_NUGGET, 'cases': meta}, f, indent=0)
    print('%d cases, %d + %d + %d elements -> %s' % (len(meta), arrays['hi'].size, arrays['co_hi'].size,
                                                      arrays['kss_hi'].size, a.out))


if __name__ == '__main__':
    main()
