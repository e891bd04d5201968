"""NumPy / SciPy restatement of the BOUND form of the ELBO (inference(..., elbo='bound'), option "elbo_form"), built from
oracle/cpu_ref.py's helpers, tests/_order_ref.py's sequential rule and tests/_mask_ref.py's masked precisions.

The sweep's UPDATES are the reference's (cpu_ref._node_d_and_pred / _weight_d_and_pred / _gp_update_B; under a mask the
selections of _mask_ref.sweep); only the reported value changes.  With variance = jitter^2 + yerr^2, sums over observed
entries only, m_g / Sigma_g the latent GP's OWN mean and covariance (weight (j, i): mu_w[i, j]):

    LogL = -1/2 sum_{i,n} [ log(2 pi v_in) + ((y - mean)_in - sum_j mu_w,ij mu_f,j)^2 / v_in + cross_in / v_in ]
    LogP = sum_g [ -1/2 log det K_g - 1/2 (m_g^T K_g^-1 m_g + tr K_g^-1 Sigma_g) ] - 1/2 N q (p + 1) log 2 pi
    Ent  = sum_g 1/2 log det Sigma_g + 1/2 q (p + 1) N (1 + log 2 pi)
    ELBO = LogL + LogP + Ent

i.e. the reference's value without quirks Q1 (cumulative node covariance), Q2 (raw-reshape pairing), Q3 (raw y) and Q5
(division by q).  Two routes:

* route='dense': the explicit Sigma = K - K (D^-1 + K)^-1 K (under a mask K - K S (I + S K S)^-1 S K, _mask_ref._gp, which
  needs no division by d), tr K^-1 Sigma by cho_solve, the entropy from the Cholesky factor of Sigma.
* route='B': the algebra of the device: B = I + S K S, diag Sigma and Sigma pred from X = chol(B)^-1, tr K^-1 Sigma =
  tr B^-1, log det Sigma = log det K - log det B.

Each route runs masked and unmasked, in both sweep orders.  gradient() is the fixed-state gradient of the bound for every
parameter class; at a converged state it is the total derivative (the bound is what the updates maximise).
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import cpu_ref
from tests import _mask_ref, _order_ref

LOG2PI = cpu_ref.LOG2PI
ORDERS = _order_ref.ORDERS


def _gp_dense(K, L, d, pred, masked):
    """One latent GP with the explicit covariance: diag Sigma, Sigma pred, log det Sigma, tr K^-1 Sigma."""
    if masked:
        sigma = _mask_ref._gp(K, d, pred)[0]
    else:
        sigma = _order_ref._sigma(K, d)
    sigma = 0.5 * (sigma + sigma.T)
    ld_sigma = 2.0 * np.sum(np.log(np.diag(np.linalg.cholesky(sigma))))
    return np.diag(sigma).copy(), sigma @ pred, ld_sigma, np.trace(cho_solve((L, True), sigma))


def _gp_B(K, L, d, pred, masked):
    """The same four numbers in the B-form.  Where d_n = 0 (a masked entry) nothing is divided by s:
    diag Sigma = diag K - colnorm2(X S K), Sigma pred = K pred - (X S K)^T (X S K) pred."""
    ldK = 2.0 * np.sum(np.log(np.diag(L)))
    if not masked:
        ds, m, ldB, trB, _, _ = cpu_ref._gp_update_B(K, d, pred)
        return ds, m, ldK - ldB, trB
    s = np.sqrt(d)
    N = K.shape[0]
    B = np.eye(N) + s[:, None] * K * s[None, :]
    Lb = np.linalg.cholesky(B)
    X = solve_triangular(Lb, np.eye(N), lower=True)
    W = X @ (s[:, None] * K)
    return (np.diag(K) - np.sum(W * W, axis=0), K @ pred - W.T @ (W @ pred), ldK - 2.0 * np.sum(np.log(np.diag(Lb))),
            np.sum(X * X))


def sweep(Kf, Kw, Lf, Lw, y, yerr2, jitt2, mu, var, mask=None, order='reference', route='B'):
    """One sweep from (mu, var): (ELBO, new_mu (p+1, q, N), new_var, (LogL, LogP, Ent)) in the bound form.  y (p, N) is
    y - mean; under `mask` (p, N bool) masked entries of y / yerr2 are never read."""
    assert order in ORDERS and route in ('B', 'dense')
    seq = order == 'sequential'
    gp = _gp_B if route == 'B' else _gp_dense
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    Kw4, Lw4 = Kw.reshape(q, p, N, N), Lw.reshape(q, p, N, N)
    muF, muW = cpu_ref.split_u(mu, p, q, N)
    varF, varW = cpu_ref.split_u(var, p, q, N)
    masked = mask is not None
    if masked:
        mask = np.asarray(mask, dtype=bool)
        y = np.where(mask, y, 0.0)
        variance = np.where(mask, jitt2[:, None] + np.where(mask, yerr2, 1.0), 1.0)
        prec = np.where(mask, 1.0 / variance, 0.0)
    else:
        variance = jitt2[:, None] + yerr2

    def node_rhs(cur, j):
        if not masked:
            return cpu_ref._node_d_and_pred(y, variance, cur, muW, varW, j)
        others = [k for k in range(q) if k != j]
        resid = y - np.sum(muW[:, others] * cur[others][None], axis=1)
        return np.sum((muW[:, j] ** 2 + varW[:, j]) * prec, axis=0), np.sum(resid * muW[:, j] * prec, axis=0)

    def weight_rhs(mu_f, dsf, cur, j, i):
        if not masked:
            return cpu_ref._weight_d_and_pred(y, variance, mu_f, dsf, cur, j, i)
        others = [k for k in range(q) if k != j]
        resid = y[i] - np.sum(mu_f[others] * cur[i, others], axis=0)
        return (mu_f[j] ** 2 + dsf[j]) * prec[i], resid * mu_f[j] * prec[i]

    ent = 0.5 * q * (p + 1) * N * (1 + LOG2PI)
    logp = -0.5 * N * q * (p + 1) * LOG2PI
    mu_f, dsf = np.empty((q, N)), np.empty((q, N))
    cur = np.array(muF, dtype=float)                 # what a node's right-hand side reads of the other nodes
    for j in range(q):
        d, pred = node_rhs(cur, j)
        dsf[j], mu_f[j], ld_sigma, tr = gp(Kf[j], Lf[j], d, pred, masked)
        if seq:
            cur[j] = mu_f[j]
        ent += 0.5 * ld_sigma
        logp += -np.sum(np.log(np.diag(Lf[j]))) - 0.5 * tr
    mu_w, dsw = np.empty((p, q, N)), np.empty((q, p, N))
    curw = np.array(muW, dtype=float)                # ... and a weight's of the other nodes' weights of its output
    for j in range(q):
        for i in range(p):
            d, pred = weight_rhs(mu_f, dsf, curw, j, i)
            dsw[j, i], mu_w[i, j], ld_sigma, tr = gp(Kw4[j, i], Lw4[j, i], d, pred, masked)
            ent += 0.5 * ld_sigma
            logp += -np.sum(np.log(np.diag(Lw4[j, i]))) - 0.5 * tr
        if seq:
            curw[:, j] = mu_w[:, j]
    # the means' prior terms, every latent GP with its OWN final mean
    for j in range(q):
        a = solve_triangular(Lf[j], mu_f[j], lower=True)
        logp += -0.5 * (a @ a)
        for i in range(p):
            a = solve_triangular(Lw4[j, i], mu_w[i, j], lower=True)
            logp += -0.5 * (a @ a)
    if masked:
        logl = _mask_ref.expected_loglike(y, variance, mask, mu_f, mu_w, dsf, dsw)
    else:
        logl = cpu_ref.expected_loglike(y, variance, mu_f, mu_w, dsf, dsw)
    new_mu = np.concatenate((mu_f[None], mu_w))
    new_var = np.concatenate((dsf[None], np.transpose(dsw, (1, 0, 2))))
    return logl + logp + ent, new_mu, new_var, (logl, logp, ent)


def sweeps(Kf, Kw, Lf, Lw, y, yerr2, jitt2, mu, var, n, **kw):
    """n forced sweeps from (mu, var): per-sweep ELBO (n,), parts (n, 3), final state."""
    E, P = [], []
    for _ in range(n):
        e, mu, var, parts = sweep(Kf, Kw, Lf, Lw, y, yerr2, jitt2, mu, var, **kw)
        E.append(e)
        P.append(parts)
    return np.array(E), np.array(P), mu, var


def elbo_calc(Kf, Kw, Lf, Lw, y, yerr2, jitt2, mu, var, max_iter=10000, snapshot=None, **kw):
    """cpu_ref.elbo_calc's loop and stop rule (quirk Q7 included) over the bound's values.  Returns (ELBO, mu, var,
    iterNumber, elboArray, crit, parts, snap): crit[k] the rule's criterion after trip k + 4, parts[k] = (LogL, LogP, Ent) of
    trip k + 1, snap the state (mu, var) after trip `snapshot` (None: not kept) -- trips 1 .. n ARE n forced sweeps from the
    start, so one loop serves both."""
    E, *_ = sweep(Kf, Kw, Lf, Lw, y, yerr2, jitt2, mu, var, **kw)
    hist, crits, parts, snap, it = [E], [], [], None, 0
    while it < max_iter:
        E, mu, var, pt = sweep(Kf, Kw, Lf, Lw, y, yerr2, jitt2, mu, var, **kw)
        hist.append(E)
        parts.append(pt)
        it += 1
        if it == snapshot:
            snap = (mu, var)
        if it > 3:
            last = np.array(hist[-3:])
            crit = np.abs(np.std(last) / np.mean(last))
            crits.append(crit)
            if crit < 1e-3 and crit != 0:
                break
    return E, mu, var, it, np.array(hist), np.array(crits), np.array(parts), snap


def problem(tag):
    """_order_ref.problem with the bound form's argument list: args = (Kf, Kw, Lf, Lw, y - mean, yerr2, jitt2)."""
    pr = _order_ref.problem(tag)
    Kf, Kw, Lf, Lw, yres, y_raw, yerr2, jitt2 = pr['args']
    pr['args'] = (Kf, Kw, Lf, Lw, yres, yerr2, jitt2)
    pr['y_raw'], pr['yerr2'] = y_raw, yerr2
    return pr


def setup_args(pr):
    """The argument list again from the problem's CURRENT parameters (pr['nodes'], ['weights'], ['means'], ['jitters'])."""
    Kf, Kw, Lf, Lw, yres, jitt2 = cpu_ref.setup(pr['time'], pr['nodes'], pr['weights'], pr['means'], pr['jitters'], pr['y_raw'])
    return Kf, Kw, Lf, Lw, yres, pr['yerr2'], jitt2


# ------------------------------------------------------------------ the fixed-state gradient
def precisions(args, mu_prev, var_prev, mu, var, mask=None):
    """The precisions the sweep from (mu_prev, var_prev) to (mu, var) factored with: d_f (q, N), d_w (q, p, N)."""
    Kf, Kw, Lf, Lw, y, yerr2, jitt2 = args
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    variance = jitt2[:, None] + (yerr2 if mask is None else np.where(mask, yerr2, 1.0))
    prec = 1.0 / variance if mask is None else np.where(mask, 1.0 / variance, 0.0)
    _, muW = cpu_ref.split_u(mu_prev, p, q, N)
    _, varW = cpu_ref.split_u(var_prev, p, q, N)
    d_f = np.array([np.sum((muW[:, j] ** 2 + varW[:, j]) * prec, axis=0) for j in range(q)])
    d_w = np.array([[(mu[0, j] ** 2 + var[0, j]) * prec[i] for i in range(p)] for j in range(q)])
    return d_f, d_w


def G_matrices(args, d_f, d_w, mu, route='chol'):
    """G_g = 1/2 (a a^T - S B^-1 S), a = K_g^-1 m_g with the latent GP's own mean: what meets dK_g / dtheta.  No cross term.
    Two LAPACK routes as in tests/_grad_ref.G_matrices, whose spread is the restatement's own error: 'chol' (Cholesky
    factors, triangular solves) and 'inv' (the explicit inverse of B, the LU solve for a)."""
    Kf, Kw, Lf, Lw = args[:4]
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    Ks = [Kf[j] for j in range(q)] + [Kw[g] for g in range(q * p)]
    Ls = [Lf[j] for j in range(q)] + [Lw[g] for g in range(q * p)]
    ds = [d_f[j] for j in range(q)] + [d_w[j, i] for j in range(q) for i in range(p)]
    ms = [mu[0, j] for j in range(q)] + [mu[1 + i, j] for j in range(q) for i in range(p)]
    out = []
    for K, L, d, m in zip(Ks, Ls, ds, ms):
        s = np.sqrt(d)
        B = np.eye(N) + s[:, None] * K * s[None, :]
        if route == 'inv':
            a, Binv = np.linalg.solve(K, m), np.linalg.inv(B)
        else:
            a = cho_solve((L, True), m)
            X = solve_triangular(np.linalg.cholesky(B), np.eye(N), lower=True)
            Binv = X.T @ X
        out.append(0.5 * (np.outer(a, a) - s[:, None] * Binv * s[None, :]))
    return out


def gradient(pr, args, mu_prev, var_prev, mu, var, mask=None, dk=None, route='chol'):
    """d bound / d (nodes, weights, means, jitters) at the fixed state (mu, var) that one sweep from (mu_prev, var_prev)
    left -- the layout of inference.grad_ELBO.  Returns (gradient, norm): norm[l] = sum |G| |dK/dtheta_l| for the kernel
    entries (the scale their error is measured in), NaN elsewhere.  dk(kernel, t): the kernel's parameter derivatives
    (default tests/_grad_ref.dk_dpars)."""
    if dk is None:
        from tests import _grad_ref
        dk = _grad_ref.dk_dpars
    Kf, Kw, Lf, Lw, y, yerr2, jitt2 = args
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    t = np.asarray(pr['time'], dtype=float)
    d_f, d_w = precisions(args, mu_prev, var_prev, mu, var, mask)
    grad, norm = [], []
    for G, kernel in zip(G_matrices(args, d_f, d_w, mu, route), list(pr['nodes']) + list(pr['weights'])):
        for dK in dk(kernel, t):
            grad.append(np.sum(G * dK))
            norm.append(np.sum(np.abs(G) * np.abs(dK)))
    obs = np.ones((p, N), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    variance = np.where(obs, jitt2[:, None] + np.where(obs, yerr2, 1.0), 1.0)
    fit = np.einsum('iqn,qn->in', mu[1:], mu[0])
    resid = np.where(obs, y, 0.0) - fit
    w = np.where(obs, resid / variance, 0.0)
    for i, m in enumerate(pr['means']):
        if m is None:
            continue
        pars = np.array(m.pars, dtype=float)
        for k in range(pars.size):                   # five-point differences of the mean function itself: O(h^4)
            h = 1e-5 * max(1.0, abs(pars[k]))

            def at(v):
                x = pars.copy()
                x[k] = v
                m.set_parameters(x)
                return np.asarray(m(t), dtype=float)
            dm = (8.0 * (at(pars[k] + h) - at(pars[k] - h)) - (at(pars[k] + 2 * h) - at(pars[k] - 2 * h))) / (12.0 * h)
            m.set_parameters(pars)
            grad.append(np.sum(w[i] * dm))
            norm.append(np.nan)
    A = np.zeros((p, N))
    for i in range(p):
        for j in range(q):
            A[i] += var[0, j] * mu[1 + i, j] ** 2 + var[1 + i, j] * mu[0, j] ** 2 + var[0, j] * var[1 + i, j]
    dv = np.where(obs, -0.5 * (1.0 / variance - (resid ** 2 + A) / variance ** 2), 0.0)
    for i in range(p):
        grad.append(np.sum(dv[i]) * 2.0 * float(np.asarray(pr['jitters'], dtype=float)[i]))
        norm.append(np.nan)
    return np.array(grad), np.array(norm)
