"""The celerite kernels' formulas (csrc/fill_eval.h: GPRN_K_SHO, GPRN_K_ROTATION, GPRN_K_CELERITE) written once over an
arithmetic of the caller's choice, as oracle/kernel_formulas.py writes the reference's: mpmath at 40 digits for
tests/_gen_celerite_fixtures.py.  The parameters are in the device layout (covFunction._device_pars); every other id of
a program goes to oracle/kernel_formulas.kernel.  The formulas are the DEFINITIONS (the issue's model section), not the
device's arrangement of them: at 40 digits the textbook forms lose nothing that matters -- e^-a cosh(h a) is a product of
two representable numbers there, and sin(s) / s is exact to the working precision down to s = 0, which alone is branched
on.  Scalars only (the branches are Python's)."""
from oracle import kernel_formulas as kf

KID = dict(kf.KID, SHO=24, ROTATION=25, CELERITE=26)
OWN = (KID['SHO'], KID['ROTATION'], KID['CELERITE'])
OP_PUSH, OP_ADD, OP_MUL = kf.OP_PUSH, kf.OP_ADD, kf.OP_MUL


def sho_shape(A, a, w):
    """e^-a [C(x) + a S(x)], x = w a^2: C = cos sqrt(x), S = sin sqrt(x) / sqrt(x) for x >= 0, cosh and sinh of sqrt(-x)
    below; S(0) = 1."""
    x = w * a * a
    if x != x:
        return x
    if x == 0:
        return A.exp(-a) * (1 + a)
    s = A.sqrt(A.fabs(x))
    if x > 0:
        return A.exp(-a) * (A.cos(s) + a * A.sin(s) / s)
    # (the exponents combined: e^-a cosh(s) overflows a double's range, not mpmath's, but the sum of two exponentials is
    # the cheaper one to differentiate numerically as well)
    return (A.exp(s - a) * (1 + a / s) + A.exp(-s - a) * (1 - a / s)) / 2


def kernel(A, kid, q, ti, tj, diag, m=(1,) * 10):
    """k(t_i, t_j) of `kid` with device parameters q, one of OWN or an id of oracle/kernel_formulas."""
    if kid not in OWN:
        return kf.kernel(A, kid, q, ti, tj, diag, m)
    tau = A.fabs(ti - tj)
    pi = A.pi
    if kid == KID['SHO']:
        theta, P0, Q = q[0], q[1], q[2]
        return theta ** 2 * sho_shape(A, pi * tau / (P0 * Q), (2 * Q - 1) * (2 * Q + 1))
    if kid == KID['ROTATION']:
        theta, P, Q0, dQ, f = q[0], q[1], q[2], q[3], q[4]
        g1 = 2 * A.sqrt((Q0 + dQ) * (Q0 + dQ + 1))
        g2 = 2 * A.sqrt(Q0 * (Q0 + 1))
        p1, p2 = 2 * pi * tau / P, 4 * pi * tau / P
        k1 = A.exp(-p1 / g1) * (A.cos(p1) + A.sin(p1) / g1)
        k2 = A.exp(-p2 / g2) * (A.cos(p2) + A.sin(p2) / g2)
        return theta ** 2 / (1 + f) * (k1 + f * k2)
    a, b, c, d = q[0], q[1], q[2], q[3]
    return A.exp(-c * tau) * (a * A.cos(d * tau) + b * A.sin(d * tau))


def program(A, ops, pars, ti, tj, diag):
    """The postfix program (ops: rows (op, kid, parameter offset)) at (t_i, t_j)."""
    st = []
    for op, kid, off in ops:
        if op == OP_PUSH:
            st.append(kernel(A, int(kid), pars[int(off):], ti, tj, diag))
        else:
            b, a = st.pop(), st.pop()
            st.append(a + b if op == OP_ADD else a * b)
    return st[0]
