"""Times the ELBO gradient in its two forms on one GPU: grad_ELBO(mean_sweeps=0) with fused=False (explicit covariances:
a keep_sigma sweep, then gprn_grad_kernel per latent GP) and fused=True (a plain sweep, then ONE gprn_grad_elbo), and beside
it the device-only part -- gprn_grad_elbo against the sum of the gprn_grad_kernel calls plus what the keep_sigma sweep costs
over a plain one.  One process, a warm-up, then the median of REPS repetitions per leg, the two forms alternating.

    python profiles/grad_fused_timing.py [out.json]        (default: profiles/grad_fused_timing.json)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gpyrn_amd as gpyrn                                   # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth              # noqa: E402

REPS = 9
# N, p, q, node kernel: one tile; the solar table's size; a small mid-size problem; config 3 (SE / QP as synth.py builds them)
SHAPES = [(45, 1, 1, 'SE'), (497, 4, 1, 'QP'), (512, 3, 2, 'QP'), (4096, 3, 2, 'QP')]


def clock(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def rows(g, mu):
    q, p, N = g.q, g.p, g.N
    m_scr = mu[1:].reshape(q, p, N)
    return [mu[0, j] for j in range(q)] + [m_scr[j, i] for j in range(q) for i in range(p)]


def one_shape(N, p, q, kind):
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair])
    g.set_components(nodes, weights, means, jit)
    _, mu0, var0, _ = g.ELBOcalc(max_iter=4)            # (the state after four trips, converged or not)
    mu0, var0 = np.array(mu0, dtype=float), np.array(var0, dtype=float)
    kernels = list(g.nodes) + list(g.weights)
    n_k = sum(k.pars.size for k in kernels)
    ctx = g._setup_device(*g._get_components())

    def whole(fused):
        g._mu, g._var = mu0.copy(), var0.copy()
        return g.grad_ELBO(mean_sweeps=0, fused=fused)

    def sweep(keep):
        ctx.set_muvar(mu0, var0)
        ctx.keep_sigma(keep)
        try:
            return clock(lambda: ctx.sweep(1, commit=True))
        finally:
            ctx.keep_sigma(False)

    def device_parent():
        ctx.set_muvar(mu0, var0)
        ctx.keep_sigma(True)
        try:
            ctx.sweep(1, commit=True)
            mu, _ = ctx.get_muvar()
            ms = rows(g, mu)
            return clock(lambda: [ctx.grad_kernel(gp, ms[gp], k.pars.size) for gp, k in enumerate(kernels)])
        finally:
            ctx.keep_sigma(False)

    def device_fused():
        ctx.set_muvar(mu0, var0)
        ctx.sweep(1, commit=True)
        return clock(lambda: ctx.grad_elbo(n_k))

    ref, new = whole(False)[1], whole(True)[1]              # warm-up, and the two forms side by side
    legs = {'grad_ELBO_default_ms': [], 'grad_ELBO_fused_ms': [], 'sweep_keep_sigma_ms': [], 'sweep_plain_ms': [],
            'grad_kernel_calls_ms': [], 'grad_elbo_call_ms': []}
    sweep(True), sweep(False), device_parent(), device_fused()
    for _ in range(REPS):
        legs['grad_ELBO_default_ms'].append(clock(lambda: whole(False)))
        legs['grad_ELBO_fused_ms'].append(clock(lambda: whole(True)))
        legs['sweep_keep_sigma_ms'].append(sweep(True))
        legs['sweep_plain_ms'].append(sweep(False))
        legs['grad_kernel_calls_ms'].append(device_parent())
        legs['grad_elbo_call_ms'].append(device_fused())
    med = {k: float(np.median(v)) for k, v in legs.items()}
    dev_parent = med['grad_kernel_calls_ms'] + med['sweep_keep_sigma_ms'] - med['sweep_plain_ms']
    out = dict(N=N, p=p, q=q, nodes=kind, reps=REPS, median_ms=med,
               spread_ms={k: [float(min(v)), float(max(v))] for k, v in legs.items()},
               device_only_parent_ms=dev_parent, device_only_fused_ms=med['grad_elbo_call_ms'],
               speedup_grad_ELBO=med['grad_ELBO_default_ms'] / med['grad_ELBO_fused_ms'],
               speedup_device_only=dev_parent / med['grad_elbo_call_ms'],
               forms_differ_by=float(np.abs(new - ref).max() / np.abs(ref).max()),
               fallbacks=int(ctx.option('fallbacks')))
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'grad_fused_timing.json')
    results = [one_shape(*s) for s in SHAPES]
    with open(path, 'w') as f:
        json.dump({'what': 'grad_ELBO(mean_sweeps=0), fused=False against fused=True, and the device-only parts; '
                           'medians of %d repetitions in one process, the forms alternating' % REPS,
                   'shapes': results}, f, indent=1)
        f.write('\n')
