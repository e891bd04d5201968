"""Plain fp64 NumPy evaluation of the parameter derivatives of the kernels of the gradient tests (every built-in that is a
function of r, Sum and Multiplication trees of them), written here and not taken from the library: what an fp64 evaluation
of the textbook formulas gives against the long-double reference.  tests/test_grad_exact_gpu.py sets a kernel's bound to
4 x this evaluation's error where 1e-12 is below what fp64 (or the reference itself) resolves."""
import numpy as np

from oracle.kernel_formulas import KID, OP_ADD, OP_PUSH

pi = np.pi


def _leaf(kid, q, r, diag):
    """(k, [dk/dq_l]) of one built-in on the array r of time differences."""
    a, r2 = np.abs(r), r * r
    one = np.ones_like(r)
    if kid == KID['CONSTANT']:
        return q[0] ** 2 * one, [2 * q[0] * one]
    if kid == KID['WHITENOISE']:
        return np.where(diag, q[0] ** 2, 0.0), [np.where(diag, 2 * q[0], 0.0)]
    if kid == KID['SE']:
        k = q[0] ** 2 * np.exp(-0.5 * r2 / q[1] ** 2)
        return k, [2 * k / q[0], k * r2 / q[1] ** 3]
    if kid in (KID['PERIODIC'], KID['QP'], KID['COSPERIODIC'], KID['QUASICOSPERIODIC']):
        quasi = kid in (KID['QP'], KID['QUASICOSPERIODIC'])
        cosine = kid in (KID['COSPERIODIC'], KID['QUASICOSPERIODIC'])
        P, l = (q[2], q[3]) if quasi else (q[1], q[2])
        x = pi * a / P
        f = np.cos(x) ** 2 if cosine else np.sin(x) ** 2
        k = q[0] ** 2 * np.exp(-2 * f / l ** 2 - (r2 / (2 * q[1] ** 2) if quasi else 0.0))
        dP = k * 2 * x * np.sin(2 * x) / (P * l ** 2) * (-1.0 if cosine else 1.0)
        dl = k * 4 * f / l ** 3
        return k, ([2 * k / q[0], k * r2 / q[1] ** 3, dP, dl] if quasi else [2 * k / q[0], dP, dl])
    if kid in (KID['RQ'], KID['RQP']):
        u = r2 / (2 * q[1] * q[2] ** 2)
        k = q[0] ** 2 * (1 + u) ** (-q[1])
        d = [None, k * (u / (1 + u) - np.log(1 + u)), k * r2 / (q[2] ** 3 * (1 + u))]
        if kid == KID['RQP']:
            x = pi * a / q[3]
            per = np.exp(-2 * np.sin(x) ** 2 / q[4] ** 2)
            k = k * per
            d = [None, d[1] * per, d[2] * per, k * 2 * x * np.sin(2 * x) / (q[3] * q[4] ** 2), k * 4 * np.sin(x) ** 2 / q[4] ** 3]
        d[0] = 2 * k / q[0]
        return k, d
    if kid == KID['COSINE']:
        y = 2 * pi * a / q[1]
        return q[0] ** 2 * np.cos(y), [2 * q[0] * np.cos(y), q[0] ** 2 * np.sin(y) * y / q[1]]
    if kid == KID['EXPONENTIAL']:
        k = q[0] ** 2 * np.exp(-a / q[1])
        return k, [2 * k / q[0], k * a / q[1] ** 2]
    if kid == KID['MATERN32']:
        x = np.sqrt(3.0) * a / q[1]
        k = q[0] ** 2 * (1 + x) * np.exp(-x)
        return k, [2 * k / q[0], q[0] ** 2 * x ** 2 * np.exp(-x) / q[1]]
    if kid == KID['MATERN52']:
        x = np.sqrt(5.0) * a / q[1]
        k = q[0] ** 2 * (1 + x + x ** 2 / 3) * np.exp(-x)
        return k, [2 * k / q[0], q[0] ** 2 * x ** 2 * (1 + x) * np.exp(-x) / (3 * q[1])]
    if kid == KID['GAMMAEXP']:
        b = a / q[2]
        w = b ** q[1]
        k = q[0] ** 2 * np.exp(-w)
        with np.errstate(divide='ignore', invalid='ignore'):
            wl = np.where(a == 0, 0.0, w * np.log(b))
        return k, [2 * k / q[0], -k * wl, k * w * q[1] / q[2]]
    if kid == KID['PIECEWISE']:
        x = a / (0.5 * q[0])
        return (np.where(x > 1, 0.0, (3 * x + 1) * (1 - x) ** 3),
                [np.where(x > 1, 0.0, 12 * x ** 2 * (1 - x) ** 2 / q[0])])
    if kid == KID['PACIOREK']:
        s = q[1] ** 2 + q[2] ** 2
        k = q[0] ** 2 * np.sqrt(2 * q[1] * q[2] / s) * np.exp(-2 * r2 / s)
        return k, [2 * k / q[0], k * (0.5 / q[1] - q[1] / s + 4 * r2 * q[1] / s ** 2),
                   k * (0.5 / q[2] - q[2] / s + 4 * r2 * q[2] / s ** 2)]
    if kid in (KID['NEWPERIODIC'], KID['QUASINEWPERIODIC']):
        quasi = kid == KID['QUASINEWPERIODIC']
        P, l = (q[3], q[4]) if quasi else (q[2], q[3])
        x = pi * a / P
        u = 2 * np.sin(x) ** 2 / (q[1] * l ** 2)
        k = q[0] ** 2 * (1 + u) ** (-q[1]) * (np.exp(-0.5 * r2 / q[2] ** 2) if quasi else 1.0)
        dal = k * (u / (1 + u) - np.log(1 + u))
        dP = k * 2 * x * np.sin(2 * x) / (P * l ** 2 * (1 + u))
        dl = k * 4 * np.sin(x) ** 2 / (l ** 3 * (1 + u))
        return k, ([2 * k / q[0], dal, k * r2 / q[2] ** 3, dP, dl] if quasi else [2 * k / q[0], dal, dP, dl])
    if kid == KID['DSE']:
        z = r2 / q[1] ** 2
        e = np.exp(-0.5 * z)
        k = q[0] ** 2 / q[1] ** 4 * (q[1] ** 2 - r2) * e
        return k, [2 * k / q[0], q[0] ** 2 * e * (-2 + 5 * z - z ** 2) / q[1] ** 3]
    if kid == KID['DPERIODIC']:
        x = pi * r / q[1]
        S, C, s2, l2 = np.sin(2 * x), np.cos(2 * x), np.sin(x) ** 2, q[2] ** 2
        poly, e = l2 * C - S ** 2, np.exp(-2 * s2 / l2)
        f = 4 * pi ** 2 * q[0] ** 2 * e
        return f * poly, [2 * f * poly / q[0], f * (-2 * S * (l2 + 2 * C) - poly * 2 * S / l2) * (-x / q[1]),
                          f * (2 * q[2] * C + poly * 4 * s2 / q[2] ** 3)]
    if kid == KID['DQP']:
        th, le, P, lp = q[0], q[1], q[2], q[3]
        x = pi * r / P
        S, C, s2 = np.sin(2 * x), np.cos(2 * x), np.sin(x) ** 2
        poly = (P ** 2 * lp ** 4 * (le ** 2 - 2 * r2) - 4 * pi * P * lp ** 2 * le ** 2 * r * S + 2 * pi ** 2 * lp ** 2 * le ** 4 * C
                - 2 * pi ** 2 * le ** 4 * S ** 2)
        se = 2 * th ** 2 / (P ** 2 * lp ** 4 * le ** 4) * np.exp(-r2 / le ** 2 - 2 * s2 / lp ** 2)
        p_le = 2 * P ** 2 * lp ** 4 * le - 8 * pi * P * lp ** 2 * le * r * S + 8 * pi ** 2 * lp ** 2 * le ** 3 * C - 8 * pi ** 2 * le ** 3 * S ** 2
        p_lp = 4 * P ** 2 * lp ** 3 * (le ** 2 - 2 * r2) - 8 * pi * P * lp * le ** 2 * r * S + 4 * pi ** 2 * lp * le ** 4 * C
        p_P = (2 * P * lp ** 4 * (le ** 2 - 2 * r2) - 4 * pi * lp ** 2 * le ** 2 * r * S
               + (8 * pi * lp ** 2 * le ** 2 * r * C + (4 * pi ** 2 * lp ** 2 * le ** 4 * S + 8 * pi ** 2 * le ** 4 * S * C) / P) * x)
        return se * poly, [2 * se * poly / th, se * (p_le + poly * (-4 / le + 2 * r2 / le ** 3)),
                           se * (p_P + poly * (-2 / P + 2 * x * S / (P * lp ** 2))),
                           se * (p_lp + poly * (-4 / lp + 4 * s2 / lp ** 3))]
    raise ValueError('no NumPy derivative for kernel id %d' % kid)


def dk_dpars(ops, pars, t):
    """[dK/dpars[l]] (N, N) of the postfix program by the product rule, fp64 throughout."""
    r = t[:, None] - t[None, :]
    diag = np.eye(t.size, dtype=bool)
    pars = np.asarray(pars, dtype=float)
    st = []                                  # (value, {parameter index: derivative})
    for op, kid, off in ops:
        if op == OP_PUSH:
            k, d = _leaf(int(kid), pars[int(off):], r, diag)
            st.append((k, {int(off) + l: np.asarray(dl, dtype=float) for l, dl in enumerate(d)}))
            continue
        (b, db), (a, da) = st.pop(), st.pop()
        if op == OP_ADD:
            d = dict(da)
            for l, v in db.items():
                d[l] = d[l] + v if l in d else v
            st.append((a + b, d))
        else:
            d = {l: v * b for l, v in da.items()}
            for l, v in db.items():
                d[l] = d[l] + a * v if l in d else a * v
            st.append((a * b, d))
    zero = np.zeros_like(r)
    return [st[0][1].get(l, zero) for l in range(pars.size)]
