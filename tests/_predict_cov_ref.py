"""NumPy / SciPy restatement of the full predictive covariance (tests only): the reference's _gp.GP.prediction
(_gp.py:125-137) keeps diag(y_cov) of  y_cov = K** - K* (K + diag v)^-1 K*^T;  here the whole matrix, and its per-output
combination under the mean-field independence of the latent GPs (inference.predict_cov)."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from gpyrn_amd import meanfield

TINY = 1.25e-12


def kernel_matrix(kernel, t):
    """_gp.GP._kernel_matrix (_gp.py:40-50): + 1.25e-12 I for one-argument kernels, nothing for the two-argument ones."""
    t = np.asarray(t, dtype=float)
    if isinstance(kernel, meanfield._TWO_ARGUMENT):
        return np.asarray(kernel(t[:, None], t[None, :]), dtype=float)
    return np.asarray(kernel(t[:, None] - t[None, :]), dtype=float) + TINY * np.eye(t.size)


def cross_matrix(kernel, tstar, t):
    tstar, t = np.asarray(tstar, dtype=float), np.asarray(t, dtype=float)
    if isinstance(kernel, meanfield._TWO_ARGUMENT):
        return np.asarray(kernel(tstar[:, None], t[None, :]), dtype=float)
    return np.asarray(kernel(tstar[:, None] - t[None, :]), dtype=float)


def latent_state(mu, var, p, q, N):
    """mean and variance vectors of every latent GP in the library's order (nodes, then weight (j, i) at q + j p + i)."""
    m, v = np.reshape(mu, (p + 1, q, N)), np.reshape(var, (p + 1, q, N))
    rows = [(0, j) for j in range(q)] + [(1 + i, j) for j in range(q) for i in range(p)]
    return [m[r] for r in rows], [v[r] for r in rows]


def latent_posterior(kernel, t, m, v, tstar):
    """(mean, C) of one latent GP at tstar: _gp.py:125-137 with the covariance kept whole."""
    K = kernel_matrix(kernel, t) + np.diag(v)
    Ks = cross_matrix(kernel, tstar, t)
    cf = cho_factor(K, lower=True)
    mean = Ks @ cho_solve(cf, m)
    C = kernel_matrix(kernel, tstar) - Ks @ cho_solve(cf, Ks.T)
    return mean, C


def output_cov(means, covs, jitters, p, q, joint):
    """Per-output covariance from the latent means / covariances (library order)."""
    ns = means[0].size
    fm, fC = means[:q], covs[:q]
    wm = lambda j, i: means[q + j * p + i]
    wC = lambda j, i: covs[q + j * p + i]
    out = np.zeros((p * ns, p * ns))
    for i in range(p):
        for k in range(p):
            blk = np.zeros((ns, ns))
            for j in range(q):
                if i == k:
                    blk += np.outer(wm(j, i), wm(j, i)) * fC[j] + wC(j, i) * (fC[j] + np.outer(fm[j], fm[j])) \
                        + jitters[i] ** 2 * np.eye(ns)
                else:
                    blk += np.outer(wm(j, i), wm(j, k)) * fC[j]
            out[i * ns:(i + 1) * ns, k * ns:(k + 1) * ns] = blk
    if joint:
        return out
    return np.array([out[i * ns:(i + 1) * ns, i * ns:(i + 1) * ns] for i in range(p)])


def prediction_variance(nPred, nVar, wPred, wVar, jitters, p, q):
    """inference._Prediction's variance (meanfield.py:1364-1373), term by term."""
    ns = nPred.shape[1]
    wP, wV = wPred.reshape(q, p, ns), wVar.reshape(q, p, ns)
    jitt2 = np.array(jitters) ** 2
    out = np.zeros((ns, p))
    for i in range(p):
        for j in range(q):
            out[:, i] += wP[j, i] * wP[j, i] * nVar[j] + wV[j, i] * (nVar[j] + nPred[j] * nPred[j]) + jitt2[i]
    return out
