"""NumPy restatement of what gprn_elbocalc_batch_heldout's tail returns for ONE evaluation, from a state (p + 1, q, N):

    m_in = sum_j mu_f_j(n) mu_w_ij(n)
    v_in = sum_j [mu_w_ij^2 var_f_j + var_w_ij (var_f_j + mu_f_j^2)] + jitter_i^2 + yerr_in^2
    lpd_i = sum_{n held} -1/2 [log(2 pi v_in) + (y_resid_in - m_in)^2 / v_in]

on the held-out entries `held` (p, N bool); entries outside it are never read (NaN / inf there are selected away).
"""
import numpy as np


def predictive(mu, var, jitt2, yerr2, held):
    """(m, v), each (p, N), zero outside `held`."""
    held = np.asarray(held, dtype=bool)
    p, N = held.shape
    mu = np.asarray(mu, dtype=float).reshape(p + 1, -1, N)
    var = np.asarray(var, dtype=float).reshape(p + 1, -1, N)
    mf, vf, mw, vw = mu[0], var[0], mu[1:], var[1:]
    m = np.einsum('iqn,qn->in', mw, mf)
    v = np.sum(mw ** 2 * vf[None] + vw * (vf + mf ** 2)[None], axis=1)
    v = v + np.asarray(jitt2, dtype=float)[:, None] + np.where(held, yerr2, 0.0)
    return np.where(held, m, 0.0), np.where(held, v, 0.0)


def terms(mu, var, y_resid, jitt2, yerr2, held):
    """The per-entry terms of the log predictive density, (p, N), zero outside `held`."""
    held = np.asarray(held, dtype=bool)
    m, v = predictive(mu, var, jitt2, yerr2, held)
    v1 = np.where(held, v, 1.0)
    r = np.where(held, np.asarray(y_resid, dtype=float).reshape(held.shape), 0.0) - m
    return np.where(held, -0.5 * (np.log(2 * np.pi * v1) + r ** 2 / v1), 0.0)


def score(mu, var, y_resid, jitt2, yerr2, held):
    """(held mean (p, N), held variance (p, N), lpd (p,), n_held (p,))."""
    m, v = predictive(mu, var, jitt2, yerr2, held)
    t = terms(mu, var, y_resid, jitt2, yerr2, held)
    return m, v, t.sum(axis=1), np.asarray(held, dtype=bool).sum(axis=1)
