"""Cost of a data mask (inference(..., mask=)): BASELINE config 3 (N = 4096, p = 3, q = 2) sweeps with no mask, an all-True
mask, and 10 % / 50 % of one output masked (a contiguous block, so that each masked entry is a point of zero precision
for the two weights of that output), and one nELBO at the reference notebook's N = 45 with and without a mask.

usage: python profiles/mask_timing.py [--out FILE] [--sweeps S]
(default --out: mask_timing.json in the working directory).  Sweep rates: device-synchronised host wall clock around one
call of S forced sweeps, after a warm-up call.  nELBO: median of 50 calls; N = 45 runs on the small path with and without
a mask (an all-True mask is no mask: inference does not hand it to the device)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402


def model(cfg, mask_kind, N=None):
    N0, p, q, kind = synth.CONFIGS[cfg]
    N = N or N0
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    mask = None
    if mask_kind == 'ones':
        mask = np.ones((p, N), dtype=bool)
    elif mask_kind:
        mask = np.ones((p, N), dtype=bool)
        k = int(round(mask_kind * N))
        mask[p - 1, N // 3:N // 3 + k] = False
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair], mask=mask)
    g.set_components(nodes, weights, means, jit)
    return g


def sweep_rate(g, n):
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
    ctx.set_muvar(mu0, var0)
    ctx.sweep(3, commit=False)
    t0 = time.perf_counter()
    _, _, info = ctx.sweep(n, commit=False)
    dt = time.perf_counter() - t0
    return {'sweeps_per_s': n / dt, 'ms_per_sweep': 1e3 * dt / n, 'info': int(info),
            'fallbacks': int(ctx.option('fallbacks'))}


def nelbo_ms(g, reps=50):
    x = g.get_parameters()
    g.nELBO(x)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        g.nELBO(x)
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='mask_timing.json')
    ap.add_argument('--sweeps', type=int, default=100)
    a = ap.parse_args()
    res = {'config3': {}, 'nelbo_N45_ms': {}}
    for name, kind in [('no_mask', None), ('all_true', 'ones'), ('one_output_10pct', 0.10), ('one_output_50pct', 0.50)]:
        res['config3'][name] = sweep_rate(model(3, kind), a.sweeps)
        print(name, res['config3'][name], flush=True)
    base = res['config3']['no_mask']['ms_per_sweep']
    for name in res['config3']:
        res['config3'][name]['vs_no_mask'] = res['config3'][name]['ms_per_sweep'] / base
    for name, kind in [('no_mask', None), ('one_output_10pct', 0.10)]:
        res['nelbo_N45_ms'][name] = nelbo_ms(model(1, kind, N=45))
        print('nELBO N=45', name, res['nelbo_N45_ms'][name], flush=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
