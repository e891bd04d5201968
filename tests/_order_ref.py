"""NumPy restatement of one sweep and of ELBOcalc's loop with a choice of the ORDER of the mean updates
(inference(..., sweep_order=)), built from oracle/cpu_ref.py's own helpers.

order='reference': cpu_ref.sweep_B, operation by operation (quirk Q6, Jacobi: every mean from the OLD means of the others).
order='sequential': node j reads the NEW means of the nodes k < j and the sweep's starting means of the nodes k > j; weight
(j, i) the NEW weight means (k, i), k < j, and the starting ones for k > j.  Inside a half-sweep the precisions d -- and
with them the variances, log det B, tr B^-1 and the Q1 traces -- read none of those means; a weight's d reads the mean of
its node as the node phase left it, so between the two orders the weight variances of the nodes j >= 1 differ.  Prior
terms, likelihood, ELBO, stop rule and quirk Q7 are cpu_ref's, on the final state of the sweep.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import cpu_ref

ORDERS = ('reference', 'sequential')


def _sigma(K, d):
    """The explicit covariance of one latent GP in the reference's own form (meanfield.py:771, 850)."""
    return K - K @ np.linalg.solve(np.diag(1.0 / d) + K, K)


def sweep(Kf, Kw, Lf, Lw, y, y_raw, yerr2, jitt2, mu, var, order='reference', Kf_inv=None, return_sigma=False):
    """One ELBOaux in the algebra of the HIP path; same contract as cpu_ref.sweep_B (return_sigma: the explicit
    covariances sig_f (q, N, N), sig_w (q, p, N, N) behind the result, as cpu_ref.sweep_ref returns them)."""
    assert order in ORDERS
    seq = order == 'sequential'
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    Kw4 = Kw.reshape(q, p, N, N)
    Lw4 = Lw.reshape(q, p, N, N)
    muF, muW = cpu_ref.split_u(mu, p, q, N)
    varF, varW = cpu_ref.split_u(var, p, q, N)
    variance = jitt2[:, None] + yerr2
    if Kf_inv is None and q > 1:
        Kf_inv = [None] + [cho_solve((Lf[j], True), np.eye(N)) for j in range(1, q)]

    ent = 0.5 * q * (p + 1) * N * (1 + cpu_ref.LOG2PI)
    logp = -0.5 * N * q * (p + 1) * cpu_ref.LOG2PI
    mu_f = np.empty((q, N))
    dsf = np.empty((q, N))
    sig_f, sig_w = np.empty((q, N, N)), np.empty((q, p, N, N))
    sig_parts = []
    muF_cur = np.array(muF, dtype=float)             # what a node's right-hand side reads of the other nodes
    for j in range(q):
        d, pred = cpu_ref._node_d_and_pred(y, variance, muF_cur, muW, varW, j)
        dsf[j], mu_f[j], ldB, trBinv, Binv, s = cpu_ref._gp_update_B(Kf[j], d, pred, need_inverse=(j < q - 1))
        if seq:
            muF_cur[j] = mu_f[j]
        if return_sigma:
            sig_f[j] = _sigma(Kf[j], d)
        ldK = 2.0 * np.sum(np.log(np.diag(Lf[j])))
        ent += 0.5 * (ldK - ldB)
        tr = trBinv
        for (Bk, sk) in sig_parts:                   # Q1
            Sk = (np.eye(N) - Bk) / (sk[:, None] * sk[None, :])
            tr += np.sum(Kf_inv[j] * Sk)
        if Binv is not None:
            sig_parts.append((Binv, s))
        a = solve_triangular(Lf[j], mu_f[j], lower=True)
        logp += -0.5 * ldK - 0.5 * (a @ a + tr)

    mu_w = np.empty((p, q, N))
    dsw = np.empty((q, p, N))
    ldKw = np.empty((q, p))
    trw = np.empty((q, p))
    muW_cur = np.array(muW, dtype=float)             # ... and a weight's of the other nodes' weights of its output
    for j in range(q):
        for i in range(p):
            d, pred = cpu_ref._weight_d_and_pred(y, variance, mu_f, dsf, muW_cur, j, i)
            dsw[j, i], mu_w[i, j], ldB, trw[j, i], _, _ = cpu_ref._gp_update_B(Kw4[j, i], d, pred)
            ldKw[j, i] = 2.0 * np.sum(np.log(np.diag(Lw4[j, i])))
            if return_sigma:
                sig_w[j, i] = _sigma(Kw4[j, i], d)
            ent += 0.5 * (ldKw[j, i] - ldB)
        if seq:
            muW_cur[:, j] = mu_w[:, j]
    m_scr = mu_w.reshape(q, p, N)                    # Q2
    for j in range(q):
        for i in range(p):
            a = solve_triangular(Lw4[j, i], m_scr[j, i], lower=True)
            logp += -0.5 * ldKw[j, i] - 0.5 * (a @ a + trw[j, i])

    logl = cpu_ref.expected_loglike(y_raw, variance, mu_f, mu_w, dsf, dsw)
    new_mu = np.concatenate((mu_f[None], mu_w))
    new_var = np.concatenate((dsf[None], np.transpose(dsw, (1, 0, 2))))
    out = ((logl + logp + ent) / q, new_mu, new_var, (logl, logp, ent))
    return out + (sig_f, sig_w) if return_sigma else out


def _kf_inv(Lf):
    q, N = Lf.shape[0], Lf.shape[-1]
    return [None] + [cho_solve((Lf[j], True), np.eye(N)) for j in range(1, q)] if q > 1 else None


def sweeps(Kf, Kw, Lf, Lw, y, y_raw, yerr2, jitt2, mu, var, n, order='reference'):
    """n forced sweeps from (mu, var): per-sweep ELBO (n,), parts (n, 3), final state."""
    inv = _kf_inv(Lf)
    E, P = [], []
    for _ in range(n):
        e, mu, var, parts = sweep(Kf, Kw, Lf, Lw, y, y_raw, yerr2, jitt2, mu, var, order, Kf_inv=inv)
        E.append(e)
        P.append(parts)
    return np.array(E), np.array(P), mu, var


def elbo_calc(Kf, Kw, Lf, Lw, y, y_raw, yerr2, jitt2, mu, var, max_iter=10000, order='reference'):
    """cpu_ref.elbo_calc's loop and stop rule over the sweep above.  Returns (ELBO, mu, var, iterNumber, elboArray, crit)
    with crit[k] the rule's criterion after trip k + 4 (the first trip that evaluates it)."""
    inv = _kf_inv(Lf)
    E, *_ = sweep(Kf, Kw, Lf, Lw, y, y_raw, yerr2, jitt2, mu, var, order, Kf_inv=inv)   # Q7
    hist = [E]
    crits = []
    it = 0
    while it < max_iter:
        E, mu, var, _ = sweep(Kf, Kw, Lf, Lw, y, y_raw, yerr2, jitt2, mu, var, order, Kf_inv=inv)
        hist.append(E)
        it += 1
        if it > 3:
            last = np.array(hist[-3:])
            crit = np.abs(np.std(last) / np.mean(last))
            crits.append(crit)
            if crit < 1e-3 and crit != 0:
                break
    return E, mu, var, it, np.array(hist), np.array(crits)


def problem(tag):
    """The fixture's model and matrices: dict with meta, d, nodes, weights, means, jitters, time, the arguments `args` of
    sweep / elbo_calc up to the state, and the _initMuVar state (mu0, var0)."""
    from gpyrn_amd import covfunc, meanfunc
    from tests import _cases
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    t, y, yerr = np.array(d['time']), np.array(d['y']), np.array(d['yerr'])
    Kf, Kw, Lf, Lw, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, y)
    mu0, var0 = cpu_ref.init_mu_var(y, [n.pars[0] for n in nodes], [w.pars[0] for w in weights], jit)
    return dict(meta=meta, d=d, nodes=nodes, weights=weights, means=means, jitters=jit, time=t,
                args=(Kf, Kw, Lf, Lw, yres, y, yerr ** 2, jitt2), mu0=mu0, var0=var0)
