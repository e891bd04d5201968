"""Cost of the sequential sweep order (inference(..., sweep_order='sequential')) against the reference's order:

* ms per forced sweep at BASELINE config 3 (N = 4096, p = 3, q = 2) and at config 5's shape with N = 2048 (p = 4, q = 3):
  the launch path, where every later group adds a mean refresh of four O(N^2) launches to its phase;
* ms per forced sweep and per warm nELBO at N = 45, p = 2, q = 2: the one-tile path, two launches more per sweep;
* a batch of 32 evaluations at N = 512, p = 3, q = 2, three trips each (max_iter = 3: the stop rule cannot fire, so both
  orders run the same number of sweeps);
* trips and wall time of a full ELBOcalc at config 3 in both orders.

usage: python profiles/order_timing.py [--out FILE] [--sweeps S]
(default --out: order_timing.json in the working directory).  Sweep rates: device-synchronised host wall clock around one
call of S forced sweeps (uncommitted), after a warm-up call; the two orders alternate on one context, best of three."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402

ORDERS = ('reference', 'sequential')


def model(N, p, q, kind, order='reference'):
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair], sweep_order=order)
    g.set_components(nodes, weights, means, jit)
    return g


def sweep_ms(N, p, q, kind, n, rounds=3):
    g = model(N, p, q, kind)
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    mu0, var0 = g._initMuVar(g.nodes, g.weights, g.jitters)
    ctx.set_muvar(mu0, var0)
    best = {o: np.inf for o in ORDERS}
    for o in ORDERS:
        g.sweep_order = o
        ctx.sweep(2, commit=False)
    for _ in range(rounds):
        for o in ORDERS:
            g.sweep_order = o
            t0 = time.perf_counter()
            ctx.sweep(n, commit=False)
            best[o] = min(best[o], 1e3 * (time.perf_counter() - t0) / n)
    out = {'N': N, 'p': p, 'q': q, 'sweeps': n, 'ms_per_sweep': best,
           'sequential_over_reference': best['sequential'] / best['reference'], 'fallbacks': int(ctx.option('fallbacks'))}
    ctx.close()
    g._ctx = None
    return out


def nelbo_ms(N, p, q, kind, reps=50):
    out = {}
    for o in ORDERS:
        g = model(N, p, q, kind, o)
        x = g.get_parameters()
        g.nELBO(x)
        ts, its = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            e, _, _, it = g.ELBOcalc(mu='previous', var='previous')
            ts.append(time.perf_counter() - t0)
            its.append(int(it))
        out[o] = {'ms_per_nelbo': 1e3 * float(np.median(ts)), 'trips': int(np.median(its)),
                  'ms_per_trip': 1e3 * float(np.median(ts)) / max(1, int(np.median(its)))}
    return {'N': N, 'p': p, 'q': q, **out}


def batch_ms(N, p, q, kind, B, max_iter=3, reps=5):
    out = {}
    for o in ORDERS:
        g = model(N, p, q, kind, o)
        x0 = np.array(g.get_parameters(), dtype=float)
        rng = np.random.RandomState(5)
        sets = [x0 * (1.0 + 0.02 * rng.standard_normal(x0.size)) for _ in range(B)]
        g.nELBO_batch(sets, max_iter=max_iter)
        ts = []
        for _ in range(reps):
            g._mu = g._var = None
            t0 = time.perf_counter()
            g.nELBO_batch(sets, max_iter=max_iter)
            ts.append(time.perf_counter() - t0)
        out[o] = 1e3 * float(np.median(ts))
    return {'N': N, 'p': p, 'q': q, 'evaluations': B, 'trips_each': max_iter, 'ms_per_call': out,
            'sequential_over_reference': out['sequential'] / out['reference']}


def elbocalc_wall(N, p, q, kind):
    out = {}
    for o in ORDERS:
        g = model(N, p, q, kind, o)
        g._setup_device(g.nodes, g.weights, g.means, g.jitters)
        t0 = time.perf_counter()
        e, _, _, it = g.ELBOcalc()
        out[o] = {'trips': int(it), 'seconds': time.perf_counter() - t0, 'elbo': float(e)}
    return {'N': N, 'p': p, 'q': q, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='order_timing.json')
    ap.add_argument('--sweeps', type=int, default=20)
    a = ap.parse_args()
    res = {}
    N, p, q, kind = synth.CONFIGS[3]
    res['config3_sweep'] = sweep_ms(N, p, q, kind, a.sweeps)
    print(json.dumps(res['config3_sweep']), flush=True)
    _, p5, q5, k5 = synth.CONFIGS[5]
    res['cfg5shape_N2048_sweep'] = sweep_ms(2048, p5, q5, k5, min(a.sweeps, 8))
    print(json.dumps(res['cfg5shape_N2048_sweep']), flush=True)
    res['one_tile_N45_q2_sweep'] = sweep_ms(45, 2, 2, 'SE', 64)
    print(json.dumps(res['one_tile_N45_q2_sweep']), flush=True)
    res['one_tile_N45_q2_nelbo'] = nelbo_ms(45, 2, 2, 'SE')
    print(json.dumps(res['one_tile_N45_q2_nelbo']), flush=True)
    res['batch32_N512_p3q2'] = batch_ms(512, 3, 2, 'QP', 32)
    print(json.dumps(res['batch32_N512_p3q2']), flush=True)
    res['config3_elbocalc'] = elbocalc_wall(N, p, q, kind)
    print(json.dumps(res['config3_elbocalc']), flush=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
