"""High-precision reference of the mean functions: tests/golden/mean_highprec.{npz,json}  (python -m tests._gen_mean_fixtures).

mpmath at 40 digits, no GPU.  Per case -- a mean of gpyrn_amd.meanfunc, written as the expression that builds it, on one of
the time sets below -- and per time:

* ``hi`` + ``lo``: the exact value at the (double) inputs as a double-double (lo in float32: 2^-77 from exact);
* ``dhi`` + ``dlo``: every d / d theta_k the same way, (n_par, n) per case.  They are the closed forms of meanfunc's
  ``_dm_dpars`` evaluated exactly; the generator first holds each against mpmath's numerical derivative of the VALUE at three
  times of every case (1e-12 of its size), so the fixture judges the formulas and not their transcription;
* ``kappa``, ``dkappa``: sum_u |u df/du| of the value / of each derivative over u in {t, every parameter, the intermediates
  the formula rounds and then cancels or divides by} (the rule of oracle/kernel_formulas.N_INTERMEDIATES: a multiplier of 1 on
  the intermediate).  Keplerian: E, the two terms of D = 1 - e cos E, and the terms K cos(nu + w), K e cos w; the polynomials:
  their monomials (Linear: mean(t) and the product); Sine: the two terms of its argument; every Sum: its two operands.
  Taken by central differences at a relative step of 1e-15 in 40-digit arithmetic.

The bound every evaluation is held to (tests/_mean_fixture.py): |m - m_ref| <= (C0 |m_ref| + C1 kappa) 2^-53 with
tests/_fill_fixture's C0, C1 = 4, 2; NaN where the reference is NaN.

Time sets (45 points each): ``A`` in [0, 60]; ``B`` BJD, 2.45e6 + [0, 3000], one stamp repeated; ``C`` around P = 0.37 and
Tp = 7.25: t = Tp exactly, M a hair on either side of +-pi, and times out to 1500 (four thousand periods).  ``mix1``,
``mix45``, ``mix257``: the first 1 / 45 / 257 of 257 times in [0, 60] (Linear subtracts the mean of the times it is given).

Cases: every leaf on A and B; Sum and Product three deep; Keplerian at e in {0, 1e-12, 0.1, 0.5, 0.9, 0.97, 0.99} x
w in {0, 0.8, pi} x {A, B, C}; the degenerate rows e = 1, e = -0.1, P = 0 and a NaN parameter (reference NaN); and the two
programs tests/test_mean_gpu.py mixes, at three parameter sets and the three mix lengths.

The one record taken from the reference: ``ref_e0`` -- _utils.keplerian (_utils.py:62-118) at e = 0, P = 11.3, K = 3.7,
w = 0.8 on the 45 times of A, imported through the stand-ins as oracle/gen_golden.py arranges them.  Its worst error against
the 40-digit value, in units of 2^-53 K (1 + |M|), is written into the json (``ref_e0_measured``).  For e > 0 its iteration
does not converge (it updates M from the lagged E) and nothing of it is recorded.  Without the reference on the import path the
record already in the fixture is kept."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from gpyrn_amd import meanfunc as mf  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
DPS = 40
H = '1e-15'


def time_sets():
    r = np.random.RandomState(20261)
    A = np.sort(r.uniform(0.0, 60.0, 45))
    B = 2.45e6 + np.sort(r.uniform(0.0, 3000.0, 45))
    B[17] = B[16]                                        # a repeated stamp
    P, Tp = 0.37, 7.25
    C = [Tp, Tp + 1e-9, Tp - 1e-9]
    for k in (0, 3, 40, 1000, 4000):                     # M a hair from +-pi, on either side
        half = Tp + P * (k + 0.5)
        C += [half, np.nextafter(half, 0.0), np.nextafter(half, 1e9), half - 1e-7, half + 1e-7]
    C += list(r.uniform(0.0, 1500.0, 45 - len(C)))
    C = np.sort(np.array(C))
    mix = np.sort(r.uniform(0.0, 60.0, 257))
    r.shuffle(mix)                                       # (a prefix is then no initial stretch of the span)
    return {'A': A, 'B': B, 'C': C, 'mix1': mix[:1].copy(), 'mix45': mix[:45].copy(), 'mix257': mix}


KEP = {'A': (11.3, 3.7, 2.1), 'B': (11.3, 3.7, 2450017.4), 'C': (0.37, 3.7, 7.25)}      # P, K, Tp per time set
MIX_PARS = [
    ('m.Keplerian(11.3, 3.7, 0.5, 0.8, 2.1) + m.Constant(1.7)', 'm.Sine(2.5, 7.7, 0.4) * m.Linear(0.03, -2.0) + m.Cubic(2e-5, -1e-3, 0.02, 1.0)'),
    ('m.Keplerian(3.21, 12.0, 0.97, 3.9, -4.4) + m.Constant(-30.0)', 'm.Sine(0.3, 1.37, 2.0) * m.Linear(-1.5, 0.25) + m.Cubic(-1e-4, 3e-3, 0.5, -7.0)'),
    ('m.Keplerian(47.0, 0.8, 0.0, 0.0, 30.0) + m.Constant(0.0)', 'm.Sine(11.0, 60.0, 0.0) * m.Linear(0.0, 1.0) + m.Cubic(0.0, 0.0, 0.0, 2.0)'),
]


def case_list():
    cases = []
    leaves = ['m.Constant(1.7)', 'm.Linear(0.03, -2.0)', 'm.Parabola(1e-3, -0.02, 0.5)', 'm.Cubic(2e-5, -1e-3, 0.02, 1.0)',
              'm.Sine(2.5, 7.7, 0.4)']
    for ts in 'AB':
        for expr in leaves:
            cases.append({'name': f'{expr[2:expr.index("(")]}_{ts}', 'expr': expr, 'tset': ts})
    cases.append({'name': 'Sum3_A', 'tset': 'A',
                  'expr': 'm.Keplerian(11.3, 3.7, 0.5, 0.8, 2.1) + m.Constant(1.7) + m.Linear(0.03, -2.0) + m.Sine(2.5, 7.7, 0.4)'})
    cases.append({'name': 'Product3_A', 'tset': 'A',
                  'expr': 'm.Sine(2.5, 7.7, 0.4) * m.Linear(0.03, -2.0) * m.Parabola(1e-3, -0.02, 0.5) * m.Constant(1.7)'})
    for ts in 'ABC':
        P, K, Tp = KEP[ts]
        for e in (0.0, 1e-12, 0.1, 0.5, 0.9, 0.97, 0.99):
            for wn, w in (('0', 0.0), ('0.8', 0.8), ('pi', float(np.pi))):
                cases.append({'name': f'Keplerian_{ts}_e{e:g}_w{wn}', 'tset': ts, 'e': e,
                              'expr': f'm.Keplerian({P!r}, {K!r}, {e!r}, {w!r}, {Tp!r})'})
    P, K, Tp = KEP['A']
    for tag, expr in (('e1', f'm.Keplerian({P}, {K}, 1.0, 0.8, {Tp})'), ('eneg', f'm.Keplerian({P}, {K}, -0.1, 0.8, {Tp})'),
                      ('P0', f'm.Keplerian(0.0, {K}, 0.5, 0.8, {Tp})'), ('nan', f'm.Keplerian({P}, nan, 0.5, 0.8, {Tp})')):
        cases.append({'name': f'Keplerian_A_{tag}', 'tset': 'A', 'expr': expr, 'nan': True})
    for s, pair in enumerate(MIX_PARS):
        for o, expr in zip((0, 2), pair):
            for nt in (1, 45, 257):
                cases.append({'name': f'mix_set{s}_out{o}_nt{nt}', 'tset': f'mix{nt}', 'expr': expr})
    return cases


def build(expr):
    return eval(expr, {'m': mf, 'nan': float('nan')})


N_MULT = {'Constant': 0, 'Linear': 2, 'Parabola': 2, 'Cubic': 3, 'Sine': 2, 'Keplerian': 5}


def count_mult(node):
    if isinstance(node, mf.Sum):
        return 2 + count_mult(node.m1) + count_mult(node.m2)
    if isinstance(node, mf.Product):
        return count_mult(node.m1) + count_mult(node.m2)
    return N_MULT[type(node).__name__]


def kepler_E(mp, Ma, e):
    """E - e sin E = Ma at working precision: Newton from the upper end of the bracket [Ma, min(Ma + e, pi)], from where it
    descends monotonically (f is convex) -- nothing of the code under test enters -- until the step is below 1e-38, the
    residual then asserted"""
    E = min(Ma + abs(e), mp.pi)
    for _ in range(200):
        step = (E - e * mp.sin(E) - Ma) / (1 - e * mp.cos(E))
        E = E - step
        if abs(step) < mp.mpf('1e-38'):
            break
    assert abs(E - e * mp.sin(E) - Ma) < mp.mpf('1e-35'), (Ma, e, E)
    return E


def leaf(mp, node, th, t, tmean, mu):
    """(value, [d value / d theta_k]) of one leaf at parameters th (mpf), multipliers mu on its intermediates"""
    name = type(node).__name__
    one = mp.mpf(1)
    if name == 'Constant':
        return th[0], [one]
    if name == 'Linear':
        dt = t - tmean * mu[0]
        return th[0] * dt * mu[1] + th[1], [dt, one]
    if name in ('Parabola', 'Cubic'):
        n = len(th)
        v = sum(th[k] * t ** (n - 1 - k) * mu[k] for k in range(n - 1)) + th[n - 1]
        return v, [t ** (n - 1 - k) for k in range(n)]
    if name == 'Sine':
        A, P, ph = th
        arg = (2 * mp.pi * t / P) * mu[0] + ph * mu[1]
        return A * mp.sin(arg), [mp.sin(arg), -A * mp.cos(arg) * 2 * mp.pi * t / P ** 2, A * mp.cos(arg)]
    P, K, e, w, Tp = th
    x = (t - Tp) / P
    fr = x - mp.nint(x)
    Ma = 2 * mp.pi * abs(fr)
    sg = -1 if fr < 0 else 1
    E = kepler_E(mp, Ma, e) * mu[0]
    cE, sE = mp.cos(E), sg * mp.sin(E)
    D = one * mu[1] - e * cE * mu[2]
    q = mp.sqrt(1 - e * e)
    cn, sn = (cE - e) / D, q * sE / D
    cw, sw = mp.cos(w), mp.sin(w)
    c, s = cn * cw - sn * sw, sn * cw + cn * sw
    v = K * c * mu[3] + K * e * cw * mu[4]
    nuM, nue = q / D ** 2, sn * (2 + e * cn) / (1 - e * e)
    return v, [K * s * nuM * 2 * mp.pi * x / P, c + e * cw, -K * s * nue + K * cw, -K * (s + e * sw), K * s * nuM * 2 * mp.pi / P]


def tree(mp, node, th, t, tmean, mu):
    """(value, derivatives in every parameter) of the expression; th and mu are consumed left to right"""
    if isinstance(node, (mf.Sum, mf.Product)):
        own = [mu.pop(0), mu.pop(0)] if isinstance(node, mf.Sum) else None
        a, da = tree(mp, node.m1, th, t, tmean, mu)
        b, db = tree(mp, node.m2, th, t, tmean, mu)
        if own:
            return a * own[0] + b * own[1], da + db
        return a * b, [d * b for d in da] + [a * d for d in db]
    n = node.pars.size
    mine, k = [th.pop(0) for _ in range(n)], N_MULT[type(node).__name__]
    return leaf(mp, node, mine, t, tmean, [mu.pop(0) for _ in range(k)])


def evaluate(mp, node, pars, t, tmean, nmult, check):
    """value, derivatives and their kappas at one time"""
    h = mp.mpf(H)
    base = [t, tmean] + list(pars) + [mp.mpf(1)] * nmult        # t, then mean(t) as an intermediate of its own, ...
    npar = len(pars)

    def f(u):
        v, d = tree(mp, node, list(u[2:2 + npar]), u[0], u[1], list(u[2 + npar:]))
        return [v] + d

    f0 = f(base)
    kap = [mp.mpf(0)] * len(f0)
    for i, u in enumerate(base):
        if u == 0:
            continue
        up, dn = list(base), list(base)
        up[i], dn[i] = u * (1 + h), u * (1 - h)
        fu, fd = f(up), f(dn)
        kap = [k + abs(a - b) / (2 * h) for k, a, b in zip(kap, fu, fd)]
    if check:                                            # the closed forms against the value's own numerical derivative
        for k in range(npar):
            if pars[k] == 0:
                step = mp.mpf('1e-12')
            else:
                step = abs(pars[k]) * mp.mpf('1e-12')
            def g(s, k=k):
                u = list(base)
                u[2 + k] = pars[k] + s
                return f(u)[0]
            num = (8 * (g(step) - g(-step)) - (g(2 * step) - g(-2 * step))) / (12 * step)
            scale = max(abs(f0[1 + k]), kap[1 + k] * mp.mpf('1e-6'), mp.mpf('1e-30'))
            assert abs(num - f0[1 + k]) <= mp.mpf('1e-12') * scale + mp.mpf('1e-20'), (type(node).__name__, k, num, f0[1 + k])
    return f0, kap


def split(v):
    hi = float(v)
    return hi, float(v - hi)


def reference_e0(t):
    """_utils.keplerian of the reference at e = 0 (the one regime in which it converges), or None without the reference"""
    try:
        sys.path.insert(0, os.path.join(REPO, 'oracle', 'standins'))
        from oracle import gen_golden  # noqa: F401  (puts the reference and the stand-ins on the import path)
        from gpyrn import _utils as rutils
    except Exception as exc:                             # noqa: BLE001
        print('reference not importable (%s): keeping the recorded ref_e0' % exc)
        return None
    return np.array(rutils.keplerian(P=11.3, K=3.7, e=0, w=0.8, T=2.1, t=t)[1], dtype=float)


def main():
    import mpmath
    mp = mpmath.mp
    mp.dps = DPS
    sets = time_sets()
    cases = case_list()
    out = {f't_{k}': v for k, v in sets.items()}
    hi, lo, kap, dhi, dlo, dkap = [], [], [], [], [], []
    off = doff = 0
    for case in cases:
        node = build(case['expr'])
        t = sets[case['tset']]
        pars = [mp.mpf(float(v)) for v in node.pars]
        nmult = count_mult(node)
        tmean = sum(mp.mpf(float(x)) for x in t) / t.size
        case.update(off=off, doff=doff, n=int(t.size), npar=len(pars))
        D = [[None] * t.size for _ in pars]
        for n, tn in enumerate(t):
            if case.get('nan'):
                hi.append(np.nan), lo.append(0.0), kap.append(0.0)
                for k in range(len(pars)):
                    D[k][n] = (np.nan, 0.0, 0.0)
                continue
            f0, kp = evaluate(mp, node, pars, mp.mpf(float(tn)), tmean, nmult, check=n in (0, t.size // 2, t.size - 1))
            a, b = split(f0[0])
            hi.append(a), lo.append(b), kap.append(float(kp[0]))
            for k in range(len(pars)):
                a, b = split(f0[1 + k])
                D[k][n] = (a, b, float(kp[1 + k]))
        for row in D:
            for a, b, c in row:
                dhi.append(a), dlo.append(b), dkap.append(c)
        off += t.size
        doff += t.size * len(pars)
        print(case['name'], flush=True)
    out.update(hi=np.array(hi), lo=np.array(lo, dtype=np.float32), kappa=np.array(kap, dtype=np.float32),
               dhi=np.array(dhi), dlo=np.array(dlo, dtype=np.float32), dkappa=np.array(dkap, dtype=np.float32))
    # kappa is rounded up: a float32 below the double would tighten the bound
    for k in ('kappa', 'dkappa'):
        out[k] = np.nextafter(out[k], np.float32(np.inf))

    meta = {'dps': DPS, 'cases': cases, 'kepler_sets': KEP}
    path = os.path.join(GOLDEN, 'mean_highprec')
    rec = reference_e0(sets['A'])
    if rec is None and os.path.exists(path + '.npz'):
        old = np.load(path + '.npz')
        rec = old['ref_e0'] if 'ref_e0' in old.files else None
    if rec is not None:
        c0 = next(c for c in cases if c['name'] == 'Keplerian_A_e0_w0.8')
        s = slice(c0['off'], c0['off'] + c0['n'])
        M = 2 * np.pi * (sets['A'] - KEP['A'][2]) / KEP['A'][0]
        unit = 2.0 ** -53 * KEP['A'][1] * (1 + np.abs(M))
        err = np.abs((rec - out['hi'][s]) - out['lo'][s].astype(float))
        out['ref_e0'] = rec
        meta['ref_e0_case'] = c0['name']
        meta['ref_e0_measured'] = float((err / unit).max())
        print('ref_e0: worst error %.3f x 2^-53 K (1 + |M|)' % meta['ref_e0_measured'])
    np.savez_compressed(path + '.npz', **out)
    with open(path + '.json', 'w') as fjs:
        json.dump(meta, fjs, indent=1)
    print('wrote', path, os.path.getsize(path + '.npz'), 'bytes')


if __name__ == '__main__':
    main()
