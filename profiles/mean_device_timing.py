"""Evaluations per second of the side-by-side ELBO batches with ``device_means`` on against off, on this build:
profiles/mean_device_timing.json.

    python profiles/mean_device_timing.py [--out DIR]   (needs the GPU; a run without one fails; DIR: where the json goes)

Shapes: N = 45 with B = 256 and N = 497 with B = 32, p = 2, q = 1, one Keplerian + Constant on output 0 and a Linear on
output 1; ``nELBO_batch`` and ``nELBO_and_grad_batch`` in the bound form, both under a fixed number of sweeps' worth of work
(max_iter / sweeps = 10) from one stored state.  Each leg is a fresh process (``--leg``) that warms its shape up, then times
nine calls with a host clock around the call -- every call ends in the library's synchronise and read-back -- and reports
the median; the legs alternate on / off, nine processes each, and the figure is the median of the nine medians with their
range.  Beside the call time a leg reports the share of it spent evaluating means: the host's per-vector loop
(``set_parameters`` + ``_mean``, timed on its own over the same vectors) with the option off; with it on the means are
evaluated inside ``gprn_elbocalc_batch_means``, and the share given is an upper estimate: stand-alone ``gprn_eval_mean`` (and
``gprn_eval_mean_grad``) calls on the same vectors, copies and synchronisation included, over the call time.  A block
``against_parent_build`` already in the json is kept as it is: those figures were recorded by hand from runs of this build and
the parent commit's build side by side, which this script cannot make."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(45, 256), (497, 32)]
TRIPS, CALLS, PROCESSES = 10, 9, 9


def model(N, device_means, elbo):
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc
    r = np.random.RandomState(100 + N)
    t = np.sort(r.uniform(0.0, 60.0 * N / 45, N))
    y = 0.3 * r.randn(2, N)
    y[0] += meanfunc.Keplerian(11.3, 3.7, 0.4, 0.8, 2.1)(t)
    e = 0.1 + 0.1 * r.rand(2, N)
    g = gpyrn.inference(1, t, y[0], e[0], y[1], e[1], device_means=device_means, elbo=elbo)
    g.set_components(covfunc.SquaredExponential(1.0, 7.0), [covfunc.SquaredExponential(0.5, 15.0), covfunc.SquaredExponential(0.5, 16.0)],
                     [meanfunc.Keplerian(11.0, 3.5, 0.35, 0.7, 2.0) + meanfunc.Constant(0.1), meanfunc.Linear(0.001, 0.05)],
                     [0.2, 0.2])
    return g


def leg(N, B, on, what):
    from gpyrn_amd import _hip
    g = model(N, on, 'bound' if what == 'grad' else 'reference')
    x0 = np.array(g.get_parameters(), dtype=float)
    _, mu0, var0, _ = g.ELBOcalc(max_iter=40)
    r = np.random.RandomState(8)
    sets = [x0 * (1 + 0.02 * r.uniform(-1, 1, x0.size)) for _ in range(B)]
    spent = [0.0]
    for name in ('eval_mean', 'eval_mean_grad'):
        inner = getattr(_hip.Context, name)

        def timed(self, *a, _inner=inner, **k):
            t0 = time.perf_counter()
            out = _inner(self, *a, **k)
            spent[0] += time.perf_counter() - t0
            return out
        setattr(_hip.Context, name, timed)

    def call():
        g.set_parameters(x0.copy())
        g._mu, g._var = np.array(mu0), np.array(var0)
        t0 = time.perf_counter()
        if what == 'grad':
            g.nELBO_and_grad_batch(sets, sweeps=TRIPS, start=(np.array(mu0), np.array(var0)))
        else:
            g.nELBO_batch(sets, max_iter=TRIPS)
        return time.perf_counter() - t0
    for _ in range(3):
        call()
    times, shares = [], []
    for _ in range(CALLS):
        spent[0] = 0.0
        dt = call()
        times.append(dt)
        shares.append(spent[0] / dt)
    host_means = None
    if on:                                               # the device's mean work on its own: an upper estimate of its share
        g.set_parameters(x0.copy())
        g._mu, g._var = np.array(mu0), np.array(var0)
        ctx, _, yr, _, _, _ = g._batch_stage(sets)
        reps = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            ctx.eval_mean(yr.params)
            if what == 'grad':
                ctx.eval_mean_grad(yr.params)
            reps.append(time.perf_counter() - t0)
        shares = [float(np.median(reps)) / float(np.median(times))]
    if not on:                                           # the per-vector loop's mean work on its own
        t0 = time.perf_counter()
        for x in sets:
            g.set_parameters(x)
            g._mean(g._get_components()[2])
        host_means = (time.perf_counter() - t0) * (2 if what == 'grad' else 1)
    dt = float(np.median(times))
    print(json.dumps({'seconds': dt, 'evals_per_s': B / dt,
                      'mean_share': float(np.median(shares)) if on else host_means / dt}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--leg':
        N, B, on, what = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] == 'on', sys.argv[5]
        return leg(N, B, on, what)
    from gpyrn_amd import _hip
    if _hip.device_count() < 1:
        raise SystemExit('mean_device_timing: no GPU')
    out = {'trips': TRIPS, 'calls_per_process': CALLS, 'processes_per_leg': PROCESSES, 'legs': []}
    kept = os.path.join(ROOT, 'profiles', 'mean_device_timing.json')
    if os.path.exists(kept):
        with open(kept) as f:
            old = json.load(f)
        if 'against_parent_build' in old:
            out['against_parent_build'] = old['against_parent_build']
    for N, B in SHAPES:
        for what in ('nelbo', 'grad'):
            runs = {'on': [], 'off': []}
            for _ in range(PROCESSES):
                for mode in ('on', 'off'):               # alternating, a fresh process each
                    res = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', str(N), str(B), mode, what],
                                         capture_output=True, text=True, timeout=300, check=True)
                    runs[mode].append(json.loads(res.stdout.strip().splitlines()[-1]))
            rec = {'N': N, 'B': B, 'call': 'nELBO_batch' if what == 'nelbo' else "nELBO_and_grad_batch (elbo='bound')"}
            for mode in ('on', 'off'):
                eps = np.array([r_['evals_per_s'] for r_ in runs[mode]])
                rec['device_means_' + mode] = {'evals_per_s_median': float(np.median(eps)), 'evals_per_s_range': [float(eps.min()), float(eps.max())],
                                               'mean_share_of_call': float(np.median([r_['mean_share'] for r_ in runs[mode]]))}
            rec['speedup'] = rec['device_means_on']['evals_per_s_median'] / rec['device_means_off']['evals_per_s_median']
            out['legs'].append(rec)
            print(json.dumps(rec), flush=True)
    out_dir = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles')
    dst = os.path.join(out_dir, 'mean_device_timing.json')
    with open(dst, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', dst)


if __name__ == '__main__':
    main()
