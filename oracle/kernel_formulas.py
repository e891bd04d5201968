"""The covariance fill's kernel formulas (csrc/fill.hip, eval_kernel) written once over an arithmetic of the caller's
choice: mpmath at 40+ digits for the high-precision reference of the fill (oracle/gen_fill_highprec.py), NumPy long
double for the derivative reference of the gradient tests.  The parameters are in the device layout
(covFunction._device_pars); a program is the postfix list of covfunc._device_program.  pi is the caller's (the exact
number for mpmath): the device's rounded pi is a relative perturbation of r below 2^-53, which the condition number
of every element covers."""

KID = dict(
    CONSTANT=0, WHITENOISE=1, SE=2, PERIODIC=3, QP=4, RQ=5, RQP=6, COSINE=7,
    EXPONENTIAL=8, MATERN32=9, MATERN52=10, GAMMAEXP=11, PIECEWISE=12,
    PACIOREK=13, NEWPERIODIC=14, QUASINEWPERIODIC=15, COSPERIODIC=16,
    QUASICOSPERIODIC=17, POLYNOMIAL=18, HARMONICPERIODIC=19,
    QUASIHARMONICPERIODIC=20, DSE=21, DPERIODIC=22, DQP=23,
)
# kernels that read t_i and t_j themselves, not r
TWO_ARGUMENT = (KID['POLYNOMIAL'], KID['HARMONICPERIODIC'], KID['QUASIHARMONICPERIODIC'])
OP_PUSH, OP_ADD, OP_MUL = 0, 1, 2


class Arith:
    """sin, cos, tan, exp, sqrt, abs, power, where(c, a, b) and pi of one arithmetic."""

    def __init__(self, sin, cos, tan, exp, sqrt, fabs, power, where, pi):
        self.sin, self.cos, self.tan, self.exp, self.sqrt = sin, cos, tan, exp, sqrt
        self.fabs, self.power, self.where, self.pi = fabs, power, where, pi


def mp_arith(mp):
    return Arith(mp.sin, mp.cos, mp.tan, mp.exp, mp.sqrt, abs, lambda a, b: a ** b,
                 lambda c, a, b: a if c else b, +mp.pi)


def np_arith(np, dtype):
    pi = dtype('3.14159265358979323846264338327950288')
    return Arith(np.sin, np.cos, np.tan, np.exp, np.sqrt, np.abs, np.power, np.where, pi)


def _harmonic(A, Nh, P, t, m):
    phase = (Nh + 0.5) * 2 * A.pi * t / P * m[3]
    half = A.pi * t / P * m[4]
    s = A.sin(phase) / 2 * A.sin(half) * m[0]
    u = 0.5 / A.tan(half) * m[1] - A.cos(phase) / 2 * A.sin(half) * m[2]
    return s, u


# how many intermediates of each formula the condition number also runs over (multipliers m, 1 at the value): the
# rounded base 1 + ... of the rational quadratic forms, whose rounding alone moves k by alpha ulp (RationalQuadratic at
# alpha = 1e8: 1e-8), and the terms s, cot, cos sin of both time stamps of the harmonic kernels, which cancel, and their
# phases, rounded four times from t
N_INTERMEDIATES = {5: 1, 6: 1, 14: 1, 15: 1, 19: 10, 20: 10}


def kernel(A, kid, q, ti, tj, diag, m=(1,) * 10):
    """k(t_i, t_j) of built-in `kid`, device parameters q; `diag`: the element is on the diagonal (WhiteNoise); `m`: the
    multipliers of the intermediates (N_INTERMEDIATES)."""
    r = ti - tj
    a = A.fabs(r)
    pi = A.pi
    if kid == KID['CONSTANT']:
        return q[0] * q[0] + 0 * r
    if kid == KID['WHITENOISE']:
        return A.where(diag, q[0] * q[0] + 0 * r, 0 * r)
    if kid == KID['SE']:
        return q[0] ** 2 * A.exp(-r * r / (2 * q[1] ** 2))
    if kid == KID['PERIODIC']:
        s = A.sin(pi * a / q[1])
        return q[0] ** 2 * A.exp(-2 * s * s / q[2] ** 2)
    if kid == KID['QP']:
        s = A.sin(pi * a / q[2])
        return q[0] ** 2 * A.exp(-2 * s * s / q[3] ** 2 - r * r / (2 * q[1] ** 2))
    if kid == KID['RQ']:
        return q[0] ** 2 * A.power((1 + r * r / (2 * q[1] * q[2] ** 2)) * m[0], -q[1])
    if kid == KID['RQP']:
        s = A.sin(pi * a / q[3])
        return q[0] ** 2 * A.exp(-2 * s * s / q[4] ** 2) * A.power((1 + r * r / (2 * q[1] * q[2] ** 2)) * m[0], -q[1])
    if kid == KID['COSINE']:
        return q[0] ** 2 * A.cos(2 * pi * a / q[1])
    if kid == KID['EXPONENTIAL']:
        return q[0] ** 2 * A.exp(-a / q[1])
    if kid == KID['MATERN32']:
        x = A.sqrt(3 + 0 * r) * a / q[1]
        return q[0] ** 2 * (1 + x) * A.exp(-x)
    if kid == KID['MATERN52']:
        s5 = A.sqrt(5 + 0 * r)
        return q[0] ** 2 * (1 + (3 * s5 * q[1] * a + 5 * a * a) / (3 * q[1] ** 2)) * A.exp(-s5 * a / q[1])
    if kid == KID['GAMMAEXP']:
        return q[0] ** 2 * A.exp(-A.power(a / q[2], q[1]))
    if kid == KID['PIECEWISE']:
        x = a / (q[0] / 2)
        return A.where(x > 1, 0 * r, (3 * x + 1) * (1 - x) ** 3)
    if kid == KID['PACIOREK']:
        s = q[1] ** 2 + q[2] ** 2
        return q[0] ** 2 * A.sqrt(2 * q[1] * q[2] / s) * A.exp(-2 * r * r / s)
    if kid == KID['NEWPERIODIC']:
        s = A.sin(pi * a / q[2])
        return q[0] ** 2 * A.power((1 + 2 * s * s / (q[1] * q[3] ** 2)) * m[0], -q[1])
    if kid == KID['QUASINEWPERIODIC']:
        s = A.sin(pi * a / q[3])
        return q[0] ** 2 * A.power((1 + 2 * s * s / (q[1] * q[4] ** 2)) * m[0], -q[1]) * A.exp(-r * r / (2 * q[2] ** 2))
    if kid == KID['COSPERIODIC']:
        c = A.cos(pi * a / q[1])
        return q[0] ** 2 * A.exp(-2 * c * c / q[2] ** 2)
    if kid == KID['QUASICOSPERIODIC']:
        c = A.cos(pi * a / q[2])
        return q[0] ** 2 * A.exp(-2 * c * c / q[3] ** 2 - r * r / (2 * q[1] ** 2))
    if kid == KID['POLYNOMIAL']:
        return A.power(q[0] * ti * tj + q[1], q[2])
    if kid in (KID['HARMONICPERIODIC'], KID['QUASIHARMONICPERIODIC']):
        P = q[2] if kid == KID['HARMONICPERIODIC'] else q[3]
        s1, u1 = _harmonic(A, q[0], P, ti, m[:5])
        s2, u2 = _harmonic(A, q[0], P, tj, m[5:])
        d2 = (s1 - s2) ** 2 + (u1 - u2) ** 2
        if kid == KID['HARMONICPERIODIC']:
            return q[1] ** 2 * A.exp(-d2 / (2 * q[3] ** 2))
        return q[1] ** 2 * A.exp(-d2 / (2 * q[4] ** 2)) * A.exp(-r * r / (2 * q[2] ** 2))
    if kid == KID['DSE']:
        e2 = q[1] ** 2
        return q[0] ** 2 / e2 ** 2 * (e2 - r * r) * A.exp(-r * r / (2 * e2))
    if kid == KID['DPERIODIC']:
        x = pi * r / q[1]
        sx, cx = A.sin(x), A.cos(x)
        poly = q[2] ** 2 * A.cos(2 * x) - 4 * sx * sx * cx * cx
        return 4 * pi * pi * q[0] ** 2 * poly * A.exp(-2 * sx * sx / q[2] ** 2)
    if kid == KID['DQP']:
        th, le, P, lp = q[0], q[1], q[2], q[3]
        sx, cx = A.sin(pi * r / P), A.cos(pi * r / P)
        scale = 2 * th ** 2 / (P ** 2 * lp ** 4 * le ** 4)
        poly = (P ** 2 * lp ** 4 * le ** 2 - 2 * P ** 2 * lp ** 4 * r * r
                - 4 * pi * P * lp ** 2 * le ** 2 * r * A.sin(2 * pi * r / P)
                + 2 * pi * pi * lp ** 2 * le ** 4 * A.cos(2 * pi * r / P)
                - 8 * pi * pi * le ** 4 * sx * sx * cx * cx)
        return scale * poly * A.exp(-(lp ** 2 * r * r + 2 * le ** 2 * sx * sx) / (lp ** 2 * le ** 2))
    raise ValueError('unknown kernel id %d' % kid)


def program(A, ops, pars, ti, tj, diag, m=(1,) * 10):
    """The postfix program (ops: rows (op, kid, parameter offset)) at (t_i, t_j); `m`: the intermediates' multipliers of
    a one-kernel program."""
    st = []
    for op, kid, off in ops:
        if op == OP_PUSH:
            st.append(kernel(A, int(kid), pars[int(off):], ti, tj, diag, m))
        else:
            b, a = st.pop(), st.pop()
            st.append(a + b if op == OP_ADD else a * b)
    return st[0]


def uses_t(ops):
    """True when the program reads t_i, t_j themselves (its condition number is taken over them, not over r)."""
    return any(op == OP_PUSH and int(kid) in TWO_ARGUMENT for op, kid, _ in ops)


def dk_dpars_longdouble(np, ops, pars, ti, tj, diag, rel=1e-6):
    """[dk/dpars[l]] of the program at arrays (t_i, t_j) in NumPy long double: Richardson's extrapolation
    (4 D(h/2) - D(h)) / 3 of central differences, h = rel |pars[l]| (rel where the parameter is 0).  The reference
    derivative of the gradient tests (within 1e-11 of mpmath: tests/test_fill_highprec.py)."""
    ld = np.longdouble
    A = np_arith(np, ld)
    ti, tj = np.asarray(ti, dtype=ld), np.asarray(tj, dtype=ld)
    base = [ld(v) for v in pars]
    out = []
    for l, v in enumerate(base):
        h = ld(rel) * (abs(v) if v != 0 else ld(1))
        d = []
        for s in (h, h / 2):
            up, dn = list(base), list(base)
            up[l], dn[l] = v + s, v - s
            d.append((program(A, ops, up, ti, tj, diag) - program(A, ops, dn, ti, tj, diag)) / (2 * s))
        out.append((4 * d[1] - d[0]) / 3)
    return out
