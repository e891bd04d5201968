"""Dense NumPy / SciPy restatement of the variational form of prediction (inference(..., predict='variational'), option
"predict_form" = GPRN_PREDICT_POSTERIOR): the predictive distribution of the posterior a sweep computes.

From the state a sweep STARTS from, every latent GP g gets (K, d, pred) exactly as tests/_mask_ref.sweep (the reference's
Jacobi order) or tests/_order_mask_ref.sweep (the sequential order) form them -- `latent_inputs` repeats their loops and
is pinned to them in tests/test_varpred.py.  With s = sqrt(d) (zero where the precision is), S = diag(s), B = I + S K S:

    q(f_g) = N(mu_g, Sigma_g),   Sigma_g = K - K S B^-1 S K,   mu_g = Sigma_g pred
    mean*  = K* (pred - S B^-1 S K pred)
    C*     = K** - (L_B^-1 S K*^T)^T (L_B^-1 S K*^T),            B = L_B L_B^T

Nothing is divided by s and K is never inverted.  The nugget (cpu_ref.NUGGET, the set-up's; none for the two-argument
kernels) and WhiteNoise are delta(t, t'): K is the set-up's own matrix, K* carries them exactly where t*_m == t_n, K**
wherever t*_m == t*_n -- on its diagonal and between duplicated times.

The per-output combination under the mean-field independence of the latent GPs (f_j: node j, w_ij: weight (j, i)):

    mean_i(t)              = m_i(t) + sum_j w_ij f_j
    Cov(y_i(t), y_i(t'))   = sum_j [ w_ij w_ij' C_fj + C_wij (C_fj + f_j f_j') ] + jitter_i^2 [t, t' the same ENTRY of t*]
    Cov(y_i(t), y_k(t'))   = sum_j w_ij w_kj' C_fj                                            (i != k)

-- the jitter once (the reference form adds it once per node), and per entry of t*: it is observation noise, two
observations at one time have independent noise.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import cpu_ref
from tests import _mask_ref as M

TWO_ARGUMENT = ('HarmonicPeriodic', 'QuasiHarmonicPeriodic', 'Polynomial')


# ------------------------------------------------------------------ kernels at arbitrary pairs of times
def kernel_blocks(kernel, t, tstar):
    """(K*, K**) of `kernel` between tstar and t / tstar and tstar, delta terms by the coincidence rule.

    The kernel is evaluated once on the SQUARE difference matrix of (tstar, t) stacked, where the reference's WhiteNoise is
    w^2 on the diagonal only; its delta amplitude -- k(0) on the diagonal minus k(0) off it, read from a 2 x 2 matrix of
    zeros -- plus the nugget then moves from the diagonal to every pair of EQUAL times."""
    t = np.asarray(t, dtype=float)
    tstar = np.asarray(tstar, dtype=float)
    T = np.concatenate([tstar, t])
    if type(kernel).__name__ in TWO_ARGUMENT:
        full = np.asarray(kernel(T[:, None], T[None, :]), dtype=float)          # (no nugget, no delta term: quirk Q9)
    else:
        full = np.array(kernel(T[:, None] - T[None, :]), dtype=float)
        z = np.asarray(kernel(np.zeros((2, 2))), dtype=float)
        delta = float(z[0, 0] - z[0, 1])
        full -= delta * np.eye(T.size)
        full += (delta + cpu_ref.NUGGET) * (T[:, None] == T[None, :])
    ns = tstar.size
    return full[:ns, ns:], full[:ns, :ns]


# ------------------------------------------------------------------ (K, d, pred) of every latent GP
def latent_inputs(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask=None, order='reference'):
    """Per latent GP g (node j at j, weight (j, i) at q + j p + i): (K, d, pred) as one sweep from (mu, var) forms them,
    and the state (new_mu, new_var) that sweep leaves -- _mask_ref.sweep / _order_mask_ref.sweep, operation by operation."""
    seq = order == 'sequential'
    q, N = Kf.shape[0], Kf.shape[-1]
    p = Kw.shape[0] // q
    Kw4 = Kw.reshape(q, p, N, N)
    mask = np.ones((p, N), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    y = np.where(mask, y, 0.0)
    variance = np.where(mask, jitt2[:, None] + np.where(mask, yerr2, 1.0), 1.0)
    prec = np.where(mask, 1.0 / variance, 0.0)
    muF, muW = cpu_ref.split_u(mu, p, q, N)
    varF, varW = cpu_ref.split_u(var, p, q, N)
    inputs = [None] * (q + q * p)
    mu_f, dsf = np.empty((q, N)), np.empty((q, N))
    muF_cur = np.array(muF, dtype=float)
    for j in range(q):
        d = np.sum((muW[:, j] ** 2 + varW[:, j]) * prec, axis=0)
        others = [k for k in range(q) if k != j]
        resid = y - np.sum(muW[:, others] * muF_cur[others][None], axis=1)
        pred = np.sum(resid * muW[:, j] * prec, axis=0)
        inputs[j] = (Kf[j], d, pred)
        sig, mu_f[j], _ = M._gp(Kf[j], d, pred)
        dsf[j] = np.diag(sig)
        if seq:
            muF_cur[j] = mu_f[j]
    mu_w, dsw = np.empty((p, q, N)), np.empty((q, p, N))
    muW_cur = np.array(muW, dtype=float)
    for j in range(q):
        for i in range(p):
            d = (mu_f[j] ** 2 + dsf[j]) * prec[i]
            others = [k for k in range(q) if k != j]
            resid = y[i] - np.sum(mu_f[others] * muW_cur[i, others], axis=0)
            pred = resid * mu_f[j] * prec[i]
            inputs[q + j * p + i] = (Kw4[j, i], d, pred)
            sig, mu_w[i, j], _ = M._gp(Kw4[j, i], d, pred)
            dsw[j, i] = np.diag(sig)
        if seq:
            muW_cur[:, j] = mu_w[:, j]
    new_mu = np.concatenate((mu_f[None], mu_w))
    new_var = np.concatenate((dsf[None], np.transpose(dsw, (1, 0, 2))))
    return inputs, new_mu, new_var


# ------------------------------------------------------------------ one latent GP
def gp_predict(K, d, pred, Ks, Kss):
    """mean* (ns,) and C* (ns, ns) of one latent GP from (K, d, pred) and its blocks K* (ns, N), K** (ns, ns)."""
    s = np.sqrt(d)
    N = K.shape[0]
    B = np.eye(N) + s[:, None] * K * s[None, :]
    Lb = np.linalg.cholesky(B)
    w = cho_solve((Lb, True), s * (K @ pred))            # B^-1 S K pred
    mean = Ks @ (pred - s * w)
    W = solve_triangular(Lb, s[:, None] * Ks.T, lower=True)   # L_B^-1 S K*^T
    C = Kss - W.T @ W
    return mean, 0.5 * (C + C.T)


def predict_latent(kernels, t, tstar, inputs):
    """Latent means (G, ns) and covariances (G, ns, ns) at tstar; kernels: nodes then weights (index q + j p + i)."""
    means, covs = [], []
    for kernel, (K, d, pred) in zip(kernels, inputs):
        Ks, Kss = kernel_blocks(kernel, t, tstar)
        m, C = gp_predict(K, d, pred, Ks, Kss)
        means.append(m)
        covs.append(C)
    return np.array(means), np.array(covs)


# ------------------------------------------------------------------ the outputs
def combine(lat_mean, lat_cov, p, q, jitters, mean_values=None, joint=False):
    """Output means (ns, p) and covariances: (p, ns, ns), or (p ns, p ns) with `joint` (row i ns + t); mean_values (p, ns):
    the mean functions at tstar, or None."""
    ns = lat_mean.shape[1]
    f, Cf = lat_mean[:q], lat_cov[:q]
    w = lat_mean[q:].reshape(q, p, ns)
    Cw = lat_cov[q:].reshape(q, p, ns, ns)
    jit2 = np.asarray(jitters, dtype=float) ** 2
    mean = np.zeros((ns, p))
    for i in range(p):
        if mean_values is not None:
            mean[:, i] += mean_values[i]
        for j in range(q):
            mean[:, i] += w[j, i] * f[j]
    blocks = np.zeros((p, p, ns, ns))
    for i in range(p):
        for k in range(p):
            for j in range(q):
                blocks[i, k] += np.outer(w[j, i], w[j, k]) * Cf[j]
                if i == k:
                    blocks[i, k] += Cw[j, i] * (Cf[j] + np.outer(f[j], f[j]))
            if i == k:
                blocks[i, k] += jit2[i] * np.eye(ns)
    if joint:
        return mean, blocks.transpose(0, 2, 1, 3).reshape(p * ns, p * ns)
    return mean, np.array([blocks[i, i] for i in range(p)])


def variances(lat_mean, lat_var, p, q, jitters):
    """The variance-only combination (ns, p): sum_j [w^2 v_f + v_w (v_f + f^2)] + jitter^2, the jitter once."""
    ns = lat_mean.shape[1]
    f, vf = lat_mean[:q], lat_var[:q]
    w, vw = lat_mean[q:].reshape(q, p, ns), lat_var[q:].reshape(q, p, ns)
    out = np.zeros((ns, p))
    for i in range(p):
        for j in range(q):
            out[:, i] += w[j, i] ** 2 * vf[j] + vw[j, i] * (vf[j] + f[j] ** 2)
        out[:, i] += float(jitters[i]) ** 2
    return out


# ------------------------------------------------------------------ problems and prediction times
def synthetic(N, p, q, seed=0, composite=False):
    """A problem of any size in the layout of _mask_ref.problem: gpyrn_amd.synth's series and benchmark model (QuasiPeriodic
    nodes, SquaredExponential weights), Constant means 0.3; `composite`: node 0 becomes SE x Cosine and weight 0
    SE + WhiteNoise -- postfix programs with a delta term."""
    from gpyrn_amd import covfunc, meanfunc, synth
    t, ys, es = synth.rv_series(N, p, seed=seed)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, 'QP'))
    means = [meanfunc.Constant(0.3) for _ in range(p)]
    if composite:
        nodes[0] = covfunc.Multiplication(covfunc.SquaredExponential(0.9, 38.0), covfunc.Cosine(1.0, 10.6))
        weights[0] = covfunc.Sum(covfunc.SquaredExponential(1.0, 60.0), covfunc.WhiteNoise(0.05))
    y, yerr = np.array(ys), np.array(es)
    Kf, Kw, _, _, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, y)
    meta = dict(N=N, p=p, q=q)
    return dict(meta=meta, nodes=nodes, weights=weights, means=means, jitters=jit, time=t, Kf=Kf, Kw=Kw,
                y_resid=yres, y_raw=y, yerr2=yerr ** 2, jitt2=jitt2)


def args(pr):
    return pr['Kf'], pr['Kw'], pr['y_resid'], pr['y_raw'], pr['yerr2'], pr['jitt2']


def init_state(pr, mask=None):
    m = np.ones(pr['y_raw'].shape, dtype=bool) if mask is None else mask
    return M.init_state(pr, m)


def mixed_times(t, ns, seed=0):
    """ns prediction times: data times, times between them, times outside the span and (ns >= 2) one duplicated time, in a
    seeded shuffle.  ns = 1: one data time."""
    t = np.asarray(t, dtype=float)
    rng = np.random.RandomState(seed)
    if ns == 1:
        return np.array([t[t.size // 3]])
    n_out = max(2, ns // 10)
    n_data = min(t.size, max(1, ns // 3))
    n_between = ns - 1 - n_out - n_data
    assert n_between >= 0, 'ns too small for a mixed set'
    span = np.ptp(t)
    data = t[rng.choice(t.size, n_data, replace=False)]
    gaps = rng.choice(t.size - 1, n_between, replace=True)
    between = t[gaps] + (t[gaps + 1] - t[gaps]) * rng.uniform(0.2, 0.8, n_between)
    outside = np.concatenate([t.min() - span * rng.uniform(0.01, 0.2, n_out // 2),
                              t.max() + span * rng.uniform(0.01, 0.2, n_out - n_out // 2)])
    ts = np.concatenate([data, between, outside])
    ts = np.concatenate([ts, ts[:1]])                    # the duplicate: a DATA time twice
    rng.shuffle(ts)
    assert ts.size == ns
    return ts
