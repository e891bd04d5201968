"""Dense NumPy / SciPy restatement of one sweep and its ELBO under a data mask (inference(..., mask=)).

Output i at time n contributes nothing when mask[i, n] is False: it is left out of the node precision d_j
(meanfield.py:765), the weight precision d (:838, 850), the right-hand sides and every term of the expected
log-likelihood (:895-990, log(2 pi v) included).  Prior, entropy and constants are unchanged; every latent GP lives on
all N times.  Per latent GP, with s = sqrt(d) (zero where d = 0):

    Sigma = K - K S (I + S K S)^-1 S K,   mu = Sigma pred

-- explicit, not the reference's Woodbury form (which divides by d) and not the device's B-form.  The quirks are
kept as oracle/cpu_ref.py keeps them (Q1 cumulative node trace, Q2 raw reshape of mu_w, Q3 raw y, Q5 / q, Q6 Jacobi
order).  With an all-True mask this is the reference's sweep up to rounding (tests/test_mask.py pins it to the goldens).
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import cpu_ref

LOG2PI = np.log(2 * np.pi)


def _gp(K, d, pred):
    """Sigma, mu = Sigma pred, log det K - log det Sigma's B (= log det B) for one latent GP."""
    s = np.sqrt(d)
    N = K.shape[0]
    B = np.eye(N) + s[:, None] * K * s[None, :]
    Lb = np.linalg.cholesky(B)
    SK = s[:, None] * K
    W = solve_triangular(Lb, SK, lower=True)          # L_B^-1 S K
    sigma = K - W.T @ W
    mu = sigma @ pred
    return sigma, mu, 2.0 * np.sum(np.log(np.diag(Lb)))


def sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, return_sigma=False):
    """One ELBOaux under `mask` (p, N bool).  Same contract as cpu_ref.sweep_ref: (ELBO, new_mu, new_var,
    (LogL, LogP, Ent)).  Masked entries of y / y_raw / yerr2 are never read."""
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
    for j in range(q):
        d = np.sum((muW[:, j] ** 2 + varW[:, j]) * prec, axis=0)
        others = [k for k in range(q) if k != j]
        resid = y - np.sum(muW[:, others] * muF[others][None], axis=1)
        pred = np.sum(resid * muW[:, j] * prec, axis=0)
        sig_f[j], mu_f[j], ldB = _gp(Kf[j], d, pred)
        Lk = np.linalg.cholesky(Kf[j])
        ldK = 2.0 * np.sum(np.log(np.diag(Lk)))
        ent += 0.5 * (ldK - ldB)
        cum = cum + sig_f[j]                           # Q1: the cumulative sumSigmaF
        a = solve_triangular(Lk, mu_f[j], lower=True)
        logp += -0.5 * ldK - 0.5 * (a @ a + np.trace(cho_solve((Lk, True), cum)))
    dsf = np.einsum('jnn->jn', sig_f)

    sig_w = np.empty((q, p, N, N))
    mu_w = np.empty((p, q, N))
    for j in range(q):
        for i in range(p):
            d = (mu_f[j] ** 2 + dsf[j]) * prec[i]
            others = [k for k in range(q) if k != j]
            resid = y[i] - np.sum(mu_f[others] * muW[i, others], axis=0)
            pred = resid * mu_f[j] * prec[i]
            sig_w[j, i], mu_w[i, j], ldB = _gp(Kw4[j, i], d, pred)
            ent += 0.5 * (2.0 * np.sum(np.log(np.diag(np.linalg.cholesky(Kw4[j, i])))) - ldB)
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


def expected_loglike(y_raw, variance, mask, mu_f, mu_w, dsf, dsw):
    """cpu_ref.expected_loglike summed over the observed (i, n) only."""
    p, q, N = mu_w.shape
    w = mask.astype(float)
    fit = np.einsum('iqn,qn->in', mu_w, mu_f)
    t1 = np.sum(np.where(mask, np.log(2 * np.pi * variance), 0.0))
    t2 = np.sum(np.where(mask, (y_raw - fit) ** 2 / variance, 0.0))
    t3 = 0.0
    for i in range(p):
        for j in range(q):
            t3 += np.sum(w[i] * (dsf[j] * mu_w[i, j] ** 2 + dsw[j, i] * mu_f[j] ** 2 + dsf[j] * dsw[j, i]) / variance[i])
    return -0.5 * t1 - 0.5 * t2 - 0.5 * t3


def sweeps(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, n):
    """n forced sweeps from (mu, var): per-sweep ELBO (n,), parts (n, 3), final state."""
    E, P = [], []
    for _ in range(n):
        e, mu, var, parts = sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask)
        E.append(e)
        P.append(parts)
    return np.array(E), np.array(P), mu, var


def elbo_calc(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask, max_iter=10000):
    """ELBOcalc's loop and stop rule (cpu_ref.elbo_calc) over the masked sweep: (ELBO, mu, var, iterNumber, elboArray)."""
    E, *_ = sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask)
    hist = [E]
    it = 0
    while it < max_iter:
        E, mu, var, _ = sweep(Kf, Kw, y, y_raw, yerr2, jitt2, mu, var, mask)
        hist.append(E)
        it += 1
        if it > 3:
            last = np.array(hist[-3:])
            crit = np.abs(np.std(last) / np.mean(last))
            if crit < 1e-3 and crit != 0:
                break
    return E, mu, var, it, np.array(hist)


# ------------------------------------------------------------------ problems
def insert_times(time, extra_before=True, extra_after=True, every=1, per_gap=1, n_after=1):
    """The fixture's times with all-masked times inserted: `per_gap` evenly spaced times in every `every`-th gap (one: its
    midpoint), one before the first time, `n_after` after the last and one that keeps the mean of the grid.  Returns (new
    time vector, index of each original time in it)."""
    time = np.asarray(time, dtype=float)
    gaps = np.diff(time)
    new = [time[:-1][::every] + gaps[::every] * (k / (per_gap + 1)) for k in range(1, per_gap + 1)]
    new = list(np.concatenate(new))
    if extra_before:
        new.append(time[0] - np.median(gaps))
    if extra_after:
        new += [time[-1] + k * np.median(gaps) for k in range(1, n_after + 1)]
    # one more time that keeps mean(t) where it was: the reference's Linear mean is slope (t - mean(t)) + intercept
    new.append(time.mean() * (time.size + len(new) + 1) - time.sum() - np.sum(new))
    full = np.concatenate([time, new])
    order = np.argsort(full, kind='stable')
    full = full[order]
    pos = np.empty(full.size, dtype=int)
    pos[order] = np.arange(full.size)
    return full, pos[:time.size]


def partial_mask(p, N, seed, lo=0.15, hi=0.30, gap_output=0):
    """15-30 % of each output masked (seeded), output `gap_output` with one contiguous gap; every time keeps at least one
    observed output."""
    rng = np.random.RandomState(seed)
    mask = np.ones((p, N), dtype=bool)
    for i in range(p):
        frac = rng.uniform(lo, hi)
        k = max(1, int(round(frac * N)))
        if i == gap_output:
            start = rng.randint(N // 4, N - k - N // 8)
            mask[i, start:start + k] = False
        else:
            mask[i, rng.choice(N, k, replace=False)] = False
    for n in np.flatnonzero(~mask.any(axis=0)):     # (q >= 2 needs an observed output at every time)
        mask[rng.randint(p), n] = True
    return mask


def problem(tag, time=None, y=None, yerr=None):
    """The fixture's model (covfunc / meanfunc objects) and its matrices at `time` (default: the fixture's):
    dict with meta, d, nodes, weights, means, jitters, Kf, Kw, y_resid, y_raw, yerr2, jitt2, mu0, var0."""
    from gpyrn_amd import covfunc, meanfunc
    from tests import _cases
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    t = np.array(d['time']) if time is None else np.asarray(time, dtype=float)
    y = np.array(d['y']) if y is None else np.asarray(y, dtype=float)
    yerr = np.array(d['yerr']) if yerr is None else np.asarray(yerr, dtype=float)
    Kf, Kw, _, _, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, y)
    return dict(meta=meta, d=d, nodes=nodes, weights=weights, means=means, jitters=jit, time=t, Kf=Kf, Kw=Kw,
                y_resid=yres, y_raw=y, yerr2=yerr ** 2, jitt2=jitt2)


def inserted(tag, **kw):
    """The fixture with all-masked times inserted (insert_times): (problem at the new times, mask, positions of the
    original times).  The inserted y / yerr are NaN / inf: they must never be read."""
    from tests import _cases
    meta, d = _cases.load(tag)
    t, pos = insert_times(d['time'], **kw)
    p, N = np.array(d['y']).shape
    y = np.full((p, t.size), np.nan)
    e = np.full((p, t.size), np.inf)
    y[:, pos] = d['y']
    e[:, pos] = d['yerr']
    mask = np.zeros((p, t.size), dtype=bool)
    mask[:, pos] = True
    pr = problem(tag, time=t, y=np.where(mask, y, 0.0), yerr=np.where(mask, e, 1.0))
    pr['y_nan'], pr['yerr_inf'] = y, e
    return pr, mask, pos


def init_state(pr, mask):
    """_initMuVar on the zero-filled y (what inference does under a mask)."""
    nodes, weights = pr['nodes'], pr['weights']
    return cpu_ref.init_mu_var(np.where(mask, pr['y_raw'], 0.0), [n.pars[0] for n in nodes],
                               [w.pars[0] for w in weights], pr['jitters'])


def at_positions(state, pos):
    """The (p+1, q, N_full) state at the original times."""
    return np.asarray(state)[..., pos]
