"""Dense NumPy / LAPACK restatement of the B-form ELBO gradient (gprn_grad_elbo / gprn_grad_matrix), data masks included.

At a fixed variational state only the expected log prior (meanfield.py:992-1067) depends on the kernel of latent GP g:

    d/dtheta = 1/(2 q) < a a^T + M_g , dK_g/dtheta >,   a = K_g^-1 m_g,

with, for B = I + S K S, S = diag(sqrt(d)) (zero where d = 0: a masked entry),

    weight g:  M = - S B^-1 S                      ( = K^-1 Sigma K^-1 - K^-1, Sigma = K - K S B^-1 S K )
    node j:    M = - S B^-1 S + sum_{k<j} K_j^-1 Sigma_fk K_j^-1        (quirk Q1)

and m_g the state row of latent GP g as it lies in memory (quirk Q2).  The precisions d are formed as oracle/cpu_ref.py
(_node_d_and_pred, _weight_d_and_pred) and tests/_mask_ref.py (sweep) form them; the sweep itself is _mask_ref.sweep (an
all-True mask is the reference's sweep).  G comes out by two LAPACK routes -- inv(B) with LU solves for what meets K, and
Cholesky factors with triangular solves -- whose spread is the reference's own error (G_matrices).  The fixed-state ELBO
whose central differences the gradient is checked against is _mask_ref.expected_loglike plus the prior part of
cpu_ref.fixed_state_elbo.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import cpu_ref, kernel_formulas
from tests import _mask_ref


def sweep_state(pr, mu_prev, var_prev, mask=None):
    """One sweep of problem `pr` (_mask_ref.problem) from (mu_prev, var_prev): dict with the ELBO, the new state
    (mu, var: (p+1, q, N)), the explicit covariances (sig_f (q, N, N), sig_w (q, p, N, N)) and the precisions the sweep
    factored with (d_f (q, N), d_w (q, p, N))."""
    Kf, Kw = pr['Kf'], pr['Kw']
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    mask = np.ones((p, N), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    y_raw = np.where(mask, pr['y_raw'], 0.0)
    y = np.where(mask, pr['y_resid'], 0.0)
    yerr2 = np.where(mask, pr['yerr2'], 1.0)
    E, mu, var, parts, sig_f, sig_w = _mask_ref.sweep(Kf, Kw, y, y_raw, yerr2, pr['jitt2'], mu_prev, var_prev, mask,
                                                      return_sigma=True)
    variance = pr['jitt2'][:, None] + yerr2
    prec = np.where(mask, 1.0 / variance, 0.0)
    muF, muW = cpu_ref.split_u(mu_prev, p, q, N)
    varF, varW = cpu_ref.split_u(var_prev, p, q, N)
    d_f = np.array([np.sum((muW[:, j] ** 2 + varW[:, j]) * prec, axis=0) for j in range(q)])
    d_w = np.array([[(mu[0, j] ** 2 + var[0, j]) * prec[i] for i in range(p)] for j in range(q)])
    if mask.all():                                      # the oracle's own expressions, where they apply
        for j in range(q):
            np.testing.assert_allclose(d_f[j], cpu_ref._node_d_and_pred(y, variance, muF, muW, varW, j)[0], rtol=1e-13)
            for i in range(p):
                np.testing.assert_allclose(d_w[j, i], cpu_ref._weight_d_and_pred(y, variance, mu[0], var[0], muW, j, i)[0],
                                           rtol=1e-13)
    return dict(elbo=E, mu=mu, var=var, sig_f=sig_f, sig_w=sig_w, d_f=d_f, d_w=d_w, mask=mask, variance=variance,
                y_raw=y_raw, p=p, q=q, N=N)


def state_rows(st):
    """m_g for g = 0 .. G-1: nodes mu_f[j], weights the raw-reshape rows of mu_w (quirk Q2)."""
    q, p, N = st['q'], st['p'], st['N']
    m_scr = st['mu'][1:].reshape(q, p, N)
    return [st['mu'][0, j] for j in range(q)] + [m_scr[j, i] for j in range(q) for i in range(p)]


def _minus_SBinvS(K, d, route):
    s = np.sqrt(d)
    N = K.shape[0]
    B = np.eye(N) + s[:, None] * K * s[None, :]
    if route == 'inv':
        Binv = np.linalg.inv(B)
    else:
        X = solve_triangular(np.linalg.cholesky(B), np.eye(N), lower=True)
        Binv = X.T @ X
    return -(s[:, None] * Binv * s[None, :])


def _sigma(K, d):
    """Sigma = K - K S B^-1 S K as _mask_ref._gp forms it (no division by s)."""
    s = np.sqrt(d)
    B = np.eye(K.shape[0]) + s[:, None] * K * s[None, :]
    W = solve_triangular(np.linalg.cholesky(B), s[:, None] * K, lower=True)
    return K - W.T @ W


def G_matrices(pr, st, route='chol'):
    """G_g = 1/2 (a a^T + M_g), g = 0 .. G-1 (NOT divided by q), by LAPACK, in two routes.  'chol': Cholesky factors of B
    and of K with triangular solves.  'inv': the explicit inverse of B, and for what meets K -- a = K^-1 m and the Q1 cross
    term -- the LU solve (gesv), NOT an explicit inverse of K: at cond(K) ~ 1e8 inv(K) costs three digits that neither the
    B-form nor the device spends, and the spread of the routes would measure those.  The two solves with K are both
    backward stable and share no rounding, so the spread is the restatement's own error: on step_p3q2, step_p2q3,
    mid_N300_p3q2, illc_N100_p2q3 it is 5.2e-13, 3.6e-13, 1.3e-15, 5.0e-12 of the norm sum |G| |dK/dtheta|, where the
    'chol' route is 3.5e-13, 1.7e-14, 1.4e-15, 3.5e-12 from the same G with a solved in long double.  (With ONE solve for a
    in both routes the spread is 2e-17: G is a a^T / 2 to many digits, and the error of a would cancel out of it.)"""
    Kf, Kw = pr['Kf'], pr['Kw']
    q, p = st['q'], st['p']
    Ks = [Kf[j] for j in range(q)] + [Kw[g] for g in range(q * p)]
    ds = [st['d_f'][j] for j in range(q)] + [st['d_w'][j, i] for j in range(q) for i in range(p)]
    ms = state_rows(st)
    sig_f = [_sigma(Kf[k], st['d_f'][k]) for k in range(q - 1)]
    out = []
    for g, (K, d, m) in enumerate(zip(Ks, ds, ms)):
        if route == 'inv':
            solve = lambda A: np.linalg.solve(K, A)
        else:
            L = np.linalg.cholesky(K)
            solve = lambda A: cho_solve((L, True), A)
        a = solve(m)
        M = _minus_SBinvS(K, d, route)
        if 0 < g < q:
            S = np.sum(sig_f[:g], axis=0)
            M = M + solve(solve(S).T).T
        out.append(0.5 * (np.outer(a, a) + M))
    return out


def dk_dpars(kernel, t):
    """[dK/dtheta_l] at the data times: oracle.kernel_formulas.dk_dpars_longdouble where it covers the kernel (a device
    program), else the kernel's own _dk_dpars."""
    t = np.asarray(t, dtype=float)
    program = kernel._device_program() if hasattr(kernel, '_device_program') else None
    if program is None:
        return [np.asarray(dk, dtype=float) for dk in kernel._dk_dpars(t[:, None] - t[None, :])]
    ops, params = program
    ops = np.asarray(ops).reshape(-1, 3)
    dks = kernel_formulas.dk_dpars_longdouble(np, ops, params, t[:, None], t[None, :], np.eye(t.size, dtype=bool))
    return [np.asarray(dk, dtype=float) for dk in dks]


def kernel_gradient(pr, st, route='chol', G=None):
    """(gradient entries of the kernel parameters -- nodes then weights, divided by q; the norm sum |G| |dK/dtheta| / q
    of each entry)."""
    G = G_matrices(pr, st, route) if G is None else G
    grad, norm = [], []
    for Gg, kernel in zip(G, list(pr['nodes']) + list(pr['weights'])):
        for dk in dk_dpars(kernel, pr['time']):
            grad.append(np.sum(Gg * dk) / st['q'])
            norm.append(np.sum(np.abs(Gg) * np.abs(dk)) / st['q'])
    return np.array(grad), np.array(norm)


def fixed_state_elbo(Kf, Kw, jitt2, pr, st):
    """(LogL + LogP) / q at the fixed variational state `st` as a function of the prior matrices and the jitters: the
    masked expected log-likelihood (_mask_ref.expected_loglike) plus the prior part of cpu_ref.fixed_state_elbo."""
    q, p, N = st['q'], st['p'], st['N']
    mask = st['mask']
    Kw4 = Kw.reshape(q, p, N, N)
    mu_f, mu_w = st['mu'][0], st['mu'][1:]
    m_scr = mu_w.reshape(q, p, N)
    logp = 0.0
    cum = np.zeros((N, N))
    for j in range(q):
        cum = cum + st['sig_f'][j]
        L = np.linalg.cholesky(Kf[j])
        logp += -np.sum(np.log(np.diag(L))) - 0.5 * (mu_f[j] @ cho_solve((L, True), mu_f[j])
                                                     + np.trace(cho_solve((L, True), cum)))
        for i in range(p):
            L = np.linalg.cholesky(Kw4[j, i])
            logp += -np.sum(np.log(np.diag(L))) - 0.5 * (m_scr[j, i] @ cho_solve((L, True), m_scr[j, i])
                                                         + np.trace(cho_solve((L, True), st['sig_w'][j, i])))
    variance = np.where(mask, jitt2[:, None] + np.where(mask, pr['yerr2'], 1.0), 1.0)
    dsf = np.einsum('jnn->jn', st['sig_f'])
    dsw = np.einsum('jinn->jin', st['sig_w'])
    logl = _mask_ref.expected_loglike(st['y_raw'], variance, mask, mu_f, mu_w, dsf, dsw)
    return (logl + logp) / q


def finite_differences(pr, st, jitters=True):
    """Central differences (step 1e-5 max(1, |theta|)) of fixed_state_elbo in every kernel parameter (nodes, weights), zeros
    for the mean-function parameters (quirk Q3), then the jitters: the layout of inference.grad_ELBO.  jitters=False: the
    kernel parameters only."""
    nodes, weights, means = list(pr['nodes']), list(pr['weights']), pr['means']
    jit = list(pr['jitters'])
    t = np.asarray(pr['time'], dtype=float)

    def F():
        Kf = np.array([cpu_ref.kmatrix(k, t) for k in nodes])
        Kw = np.array([cpu_ref.kmatrix(k, t) for k in weights])
        return fixed_state_elbo(Kf, Kw, np.asarray(jit, dtype=float) ** 2, pr, st)

    fd = []
    for k in nodes + weights:
        for i in range(k.pars.size):
            v = k.pars[i]
            h = 1e-5 * max(1.0, abs(v))
            k.pars[i] = v + h; up = F()
            k.pars[i] = v - h; dn = F()
            k.pars[i] = v
            fd.append((up - dn) / (2 * h))
    if not jitters:
        return np.array(fd)
    fd += [0.0] * sum(0 if m is None else int(m._parsize) for m in means)
    for i in range(len(jit)):
        v = jit[i]
        h = 1e-5 * max(1.0, abs(v))
        jit[i] = v + h; up = F()
        jit[i] = v - h; dn = F()
        jit[i] = v
        fd.append((up - dn) / (2 * h))
    return np.array(fd)
