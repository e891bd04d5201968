"""Dense NumPy / SciPy restatement of one sweep under a data mask WITH a choice of the order of the mean updates
(inference(..., mask=, sweep_order=, sequential_under_mask=True)).

It is tests/_mask_ref.py's sweep -- the explicit Sigma = K - K S (I + S K S)^-1 S K of _mask_ref._gp, the masked
precisions and right-hand sides, _mask_ref.expected_loglike -- with tests/_order_ref.py's rule:

order='reference':  every mean from the means the sweep started from (quirk Q6): _mask_ref.sweep, operation by operation.
order='sequential': node j reads the NEW means of the nodes k < j and the starting means of the nodes k > j; weight (j, i)
                    the NEW weight means (k, i), k < j, and the starting ones for k > j.

The precision d of a latent GP reads none of the means the order is about, so Sigma, its diagonal, log det B and the Q1
traces are the same in both orders inside a half-sweep; only pred, and with it mu = Sigma pred, changes.  mu = Sigma pred
covers the rows of zero precision too (there mu_n = sum_m K_nm s_m c_m: what the device takes from the phase's ct).
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import cpu_ref
from tests._mask_ref import LOG2PI, _gp, expected_loglike

ORDERS = ('reference', 'sequential')


def sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, order='reference', return_sigma=False):
    """One ELBOaux under `mask` (p, N bool) in `order`.  Same contract as _mask_ref.sweep: (ELBO, new_mu, new_var,
    (LogL, LogP, Ent)) and, with return_sigma, the explicit covariances sig_f (q, N, N), sig_w (q, p, N, N) behind it.
    Masked entries of y / y_raw / yerr2 are never read."""
    assert order in ORDERS
    seq = order == 'sequential'
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    Kw4 = Kw.reshape(q, p, N, N)
    mask = np.asarray(mask, dtype=bool)
    y = np.where(mask, y, 0.0)
    y_raw = np.where(mask, y_raw, 0.0)
    variance = np.where(mask, jitt2[:, None] + np.where(mask, yerr2, 1.0), 1.0)
    prec = np.where(mask, 1.0 / variance, 0.0)        # zero precision where masked
    muF, muW = cpu_ref.split_u(mu, p, q, N)
    varF, varW = cpu_ref.split_u(var, p, q, N)

    ent = 0.5 * q * (p + 1) * N * (1 + LOG2PI)
    logp = -0.5 * N * q * (p + 1) * LOG2PI
    sig_f = np.empty((q, N, N))
    mu_f = np.empty((q, N))
    cum = np.zeros((N, N))
    muF_cur = np.array(muF, dtype=float)               # what a node's right-hand side reads of the other nodes
    for j in range(q):
        d = np.sum((muW[:, j] ** 2 + varW[:, j]) * prec, axis=0)
        others = [k for k in range(q) if k != j]
        resid = y - np.sum(muW[:, others] * muF_cur[others][None], axis=1)
        pred = np.sum(resid * muW[:, j] * prec, axis=0)
        sig_f[j], mu_f[j], ldB = _gp(Kf[j], d, pred)
        if seq:
            muF_cur[j] = mu_f[j]
        Lk = np.linalg.cholesky(Kf[j])
        ldK = 2.0 * np.sum(np.log(np.diag(Lk)))
        ent += 0.5 * (ldK - ldB)
        cum = cum + sig_f[j]                           # Q1: the cumulative sumSigmaF
        a = solve_triangular(Lk, mu_f[j], lower=True)
        logp += -0.5 * ldK - 0.5 * (a @ a + np.trace(cho_solve((Lk, True), cum)))
    dsf = np.einsum('jnn->jn', sig_f)

    sig_w = np.empty((q, p, N, N))
    mu_w = np.empty((p, q, N))
    muW_cur = np.array(muW, dtype=float)               # ... and a weight's of the other nodes' weights of its output
    for j in range(q):
        for i in range(p):
            d = (mu_f[j] ** 2 + dsf[j]) * prec[i]
            others = [k for k in range(q) if k != j]
            resid = y[i] - np.sum(mu_f[others] * muW_cur[i, others], axis=0)
            pred = resid * mu_f[j] * prec[i]
            sig_w[j, i], mu_w[i, j], ldB = _gp(Kw4[j, i], d, pred)
            ent += 0.5 * (2.0 * np.sum(np.log(np.diag(np.linalg.cholesky(Kw4[j, i])))) - ldB)
        if seq:
            muW_cur[:, j] = mu_w[:, j]
    dsw = np.einsum('jinn->jin', sig_w)
    m_scr = mu_w.reshape(q, p, N)                      # Q2
    for j in range(q):
        for i in range(p):
            Lk = np.linalg.cholesky(Kw4[j, i])
            a = solve_triangular(Lk, m_scr[j, i], lower=True)
            logp += -np.sum(np.log(np.diag(Lk))) - 0.5 * (a @ a + np.trace(cho_solve((Lk, True), sig_w[j, i])))

    logl = expected_loglike(y_raw, variance, mask, mu_f, mu_w, dsf, dsw)
    new_mu = np.concatenate((mu_f[None], mu_w))
    new_var = np.concatenate((dsf[None], np.transpose(dsw, (1, 0, 2))))
    out = ((logl + logp + ent) / q, new_mu, new_var, (logl, logp, ent))
    return out + (sig_f, sig_w) if return_sigma else out


def sweeps(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, n, order='reference'):
    """n forced sweeps from (mu, var): per-sweep ELBO (n,), parts (n, 3), final state."""
    E, P = [], []
    for _ in range(n):
        e, mu, var, parts = sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, order)
        E.append(e)
        P.append(parts)
    return np.array(E), np.array(P), mu, var


def elbo_calc(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, max_iter=10000, order='reference'):
    """ELBOcalc's loop and stop rule (cpu_ref.elbo_calc) over the sweep above.  Returns (ELBO, mu, var, iterNumber,
    elboArray, crit) with crit[k] the rule's criterion after trip k + 4 (the first trip that evaluates it)."""
    E, *_ = sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, order)   # Q7
    hist = [E]
    crits = []
    it = 0
    while it < max_iter:
        E, mu, var, _ = sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, order)
        hist.append(E)
        it += 1
        if it > 3:
            last = np.array(hist[-3:])
            crit = np.abs(np.std(last) / np.mean(last))
            crits.append(crit)
            if crit < 1e-3 and crit != 0:
                break
    return E, mu, var, it, np.array(hist), np.array(crits)


def args(pr):
    """The arguments of sweep / sweeps / elbo_calc up to the state, from a _mask_ref.problem."""
    return pr['Kf'], pr['Kw'], pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2']
