"""Time of the full predictive covariance and of joint posterior draws (inference.predict_cov / sample_posterior) on the
GPU against the NumPy / SciPy restatement of the same algebra on the host, at BASELINE config 3's shape (N = 4096, p = 3,
q = 2: eight latent GPs), ns = 1024 and 4096 prediction times, 64 draws.

usage: python profiles/predict_cov_timing.py [--out FILE] [--reps R]
(default --out: predict_cov_timing.json in the working directory).  The host side runs on the BLAS threads the
environment allows (OMP_NUM_THREADS; profiles/predict_cov_timing.json was taken with 16).  Device times are host wall
clocks around whole calls (each ends in a device synchronisation and copies its results to the host), after one warm-up
call per shape; host times the same, one repetition."""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy.linalg import cho_factor, cho_solve

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402

TINY = 1.25e-12


def host_posterior(g, tstar, draws=0, rng=None):
    """The restatement: per latent GP cho_factor(K + diag v), C = K** - K* (K + diag v)^-1 K*^T, then either the per-output
    covariance or chol(C + nu I) and the draws."""
    N, p, q = g.time.size, g.p, g.q
    m, v = np.reshape(g._mu, (p + 1, q, N)), np.reshape(g._var, (p + 1, q, N))
    rows = [(0, j) for j in range(q)] + [(1 + i, j) for j in range(q) for i in range(p)]
    t = g.time
    means, covs = [], []
    for k, r in zip(list(g.nodes) + list(g.weights), rows):
        K = k(t[:, None] - t[None, :]) + TINY * np.eye(N) + np.diag(v[r])
        Ks = k(tstar[:, None] - t[None, :])
        cf = cho_factor(K, lower=True)
        means.append(Ks @ cho_solve(cf, m[r]))
        covs.append(k(tstar[:, None] - tstar[None, :]) + TINY * np.eye(tstar.size) - Ks @ cho_solve(cf, Ks.T))
    if not draws:
        out = []
        for i in range(p):
            c = np.zeros_like(covs[0])
            for j in range(q):
                w, cw = means[q + j * p + i], covs[q + j * p + i]
                c += np.outer(w, w) * covs[j] + cw * (covs[j] + np.outer(means[j], means[j]))
            out.append(c + q * g.jitters[i] ** 2 * np.eye(tstar.size))
        return out
    lat = []
    for mean, c in zip(means, covs):
        nu = TINY
        while True:
            try:
                L = np.linalg.cholesky(c + nu * np.eye(tstar.size))
                break
            except np.linalg.LinAlgError:
                nu *= 100.0
        lat.append(mean[None] + (L @ rng.standard_normal((tstar.size, draws))).T)
    return [sum(lat[q + j * p + i] * lat[j] for j in range(q)) for i in range(p)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='predict_cov_timing.json')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    N, p, q, kind = synth.CONFIGS[3]
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[x for pair in zip(ys, es) for x in pair])
    g.set_components(nodes, weights, means, jit)
    g._mu, g._var = g._initMuVar(nodes, weights, jit)
    span = np.ptp(t)
    rec = {'shape': {'N': N, 'p': p, 'q': q, 'latent_gps': q * (p + 1), 'draws': 64},
           'host_threads': os.environ.get('OMP_NUM_THREADS'), 'rows': []}
    for ns in (1024, 4096):
        ts = np.linspace(t.min() - 0.2 * span, t.max() + 0.2 * span, ns)
        row = {'ns': ns}
        for what, call in (('predict_cov', lambda: g.predict_cov(tstar=ts)),
                           ('predict_cov_joint', lambda: g.predict_cov(tstar=ts, joint=True)),
                           ('sample_posterior_64', lambda: g.sample_posterior(tstar=ts, n=64, rng=0))):
            call()                                             # warm-up of this shape
            ts_ = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                ts_.append(time.perf_counter() - t0)
            row[what + '_device_s'] = ts_
        for what, kw in (('predict_cov', {}), ('sample_posterior_64', {'draws': 64, 'rng': np.random.default_rng(0)})):
            t0 = time.perf_counter()
            host_posterior(g, ts, **kw)
            row[what + '_host_s'] = time.perf_counter() - t0
        row['speedup_predict_cov'] = row['predict_cov_host_s'] / min(row['predict_cov_device_s'])
        row['speedup_sample_posterior_64'] = row['sample_posterior_64_host_s'] / min(row['sample_posterior_64_device_s'])
        rec['rows'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
