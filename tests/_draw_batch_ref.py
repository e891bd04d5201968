"""Dense restatement of what gprn_elbocalc_batch_draws returns per slot: tests/_varpred_ref.py's posterior form of prediction
with the covariance kept whole, and draws from it.  Nothing is restated here but the wrapping: `posterior` is
_varpred_ref.latent_inputs + predict_latent at one vector's own components (mean* (G, ns), C* (G, ns, ns)), the draws are
mean* + chol(C* + nu I) z, and the outputs' draws are _varpred_ref.combine's mean of each latent draw -- sum_j w_ij o f_j --
without mean functions and noise."""
import numpy as np

from oracle import cpu_ref
from tests import _varpred_ref as V

NU_MIN, NU_MAX = 1.25e-12, 1.25e-6


def posterior(pr, mask, order, mu0, var0, components, tstar, sweeps=1):
    """mean* (G, ns), C* (G, ns, ns) and the state (mu, var) after `sweeps` sweeps from (mu0, var0) at `components` = (nodes,
    weights, means, jitters): the predictive of the posterior the LAST of them computes."""
    nodes, weights, means, jit = components
    Kf, Kw, _, _, yres, jitt2 = cpu_ref.setup(np.asarray(pr['time']), nodes, weights, means, jit, pr['y_raw'])
    mu, var = mu0, var0
    for _ in range(sweeps):
        inputs, mu, var = V.latent_inputs(Kf, Kw, yres, pr['y_raw'], pr['yerr2'], jitt2, mu, var, mask, order)
    lat_mean, lat_cov = V.predict_latent(list(nodes) + list(weights), pr['time'], tstar, inputs)
    return lat_mean, lat_cov, mu, var


def ladder(C):
    """The smallest nu = 1.25e-12 x 100^k <= 1.25e-6 at which NumPy factors C + nu I, and the factor."""
    nu = NU_MIN
    while True:
        try:
            return nu, np.linalg.cholesky(C + nu * np.eye(C.shape[0]))
        except np.linalg.LinAlgError:
            if nu >= 0.5 * NU_MAX:
                raise
            nu *= 100.0


def latent_draws(lat_mean, lat_cov, z):
    """(G, n, ns) draws mean*_g + L_g z_g from normals z (G, n, ns), and every latent GP's nugget (G)."""
    out, nus = [], []
    for m, C, zg in zip(lat_mean, lat_cov, z):
        nu, L = ladder(C)
        out.append(m[None, :] + zg @ L.T)
        nus.append(nu)
    return np.array(out), np.array(nus)


def output_draws(lat, lat_cov, p, q, jitters):
    """(p, n, ns): V.combine's output mean of every latent draw lat[:, d] -- sum_j w_ij o f_j."""
    n = lat.shape[1]
    return np.transpose(np.array([V.combine(lat[:, d], lat_cov, p, q, jitters)[0] for d in range(n)]), (2, 0, 1))
