"""Predictions per second for many parameter vectors, side by side (inference.predict_batch(states=) -> gprn_predict_batch)
against one inference._Prediction per vector ON THE SAME TREE (the parent has no side-by-side form), at three shapes:
N = 45, p = q = 1, B = 256, 200 times (one tile); N = 497, p = 4, q = 1, B = 32, 1000 times (the reference's solar table);
N = 512, p = 3, q = 2, B = 32, 1000 times.  Every vector is the model's own perturbed by 1 %, every state the converged one
of the unperturbed parameters perturbed by 1 %.  Each shape is taken three ways: both output pairs (separate=True: the latent
rows come back too), the out_* pair alone, and one by one.  Device-synchronised host wall clock around the Python call, median
of `--reps` calls (at least nine) after a warm-up call that sizes the buffers.

With --bench-trees A B (two checkouts of the project, each built): bench.py's headline (--gpus 1 --steps S --warmup W) and
bench.py --latency at N = 45 and 512 run alternately in fresh processes, `--bench-runs` times per tree -- the run-to-run
spread of tree A on this box, and tree B's medians against it.  The first step that fails is the last: the JSON then holds
what was taken and the error, the exit status is 1, and nothing more is started on the device.

usage: python profiles/predict_batch_timing.py [--out FILE] [--reps R] [--bench-trees PARENT THIS] [--bench-runs K]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402

SHAPES = [(45, 1, 1, 'SE', 256, 200), (497, 4, 1, 'QP', 32, 1000), (512, 3, 2, 'QP', 32, 1000)]


def model(N, p, q, kind):
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair])
    g.set_components(nodes, weights, means, jit)
    return g


def median_s(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def shape(N, p, q, kind, B, ns, reps):
    g = model(N, p, q, kind)
    x0 = np.array(g.get_parameters(), dtype=float)
    sys.stdout = open(os.devnull, 'w')                        # (ELBOcalc may print a line)
    try:
        _, mu_w, var_w, trips = g.ELBOcalc()
    finally:
        sys.stdout.close()
        sys.stdout = sys.__stdout__
    rng = np.random.RandomState(5)
    sets = [x0 * (1.0 + 0.01 * rng.standard_normal(x0.size)) for _ in range(B)]
    mu = np.array([np.asarray(mu_w) * (1.0 + 0.01 * rng.standard_normal(np.shape(mu_w))) for _ in range(B)])
    var = np.array([np.asarray(var_w) * rng.uniform(0.99, 1.01, np.shape(var_w)) for _ in range(B)])
    lo, hi = g.time.min(), g.time.max()
    tstar = np.linspace(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), ns)
    shp = (p + 1, q, N)
    out = {'N': N, 'p': p, 'q': q, 'vectors': B, 'times': ns}

    def both_pairs():
        return g.predict_batch(sets, tstar=tstar, states=(mu, var), separate=True)

    def outputs_only():
        return g.predict_batch(sets, tstar=tstar, states=(mu, var))

    def one_by_one():
        res = []
        for b, x in enumerate(sets):
            g.set_parameters(x)
            res.append(g._Prediction(tstar=tstar, mu=mu[b].reshape(shp), var=var[b].reshape(shp)))
        return res

    mean, pvar = outputs_only()
    ref = one_by_one()
    out['all_finite'] = bool(np.all(np.isfinite(mean)) and np.all(np.isfinite(pvar)))
    out['worst_mean_difference_to_one_by_one'] = float(max(np.abs(mean[b] - ref[b][0]).max() for b in range(B)))
    for name, f, r in (('side_by_side_both_pairs', both_pairs, reps), ('side_by_side_outputs_only', outputs_only, reps),
                       ('one_by_one', one_by_one, reps)):
        med, lo_, hi_ = median_s(f, r)
        out[name] = {'ms_per_call': 1e3 * med, 'ms_min': 1e3 * lo_, 'ms_max': 1e3 * hi_, 'calls': r,
                     'vectors_per_s': B / med, 'ms_per_vector': 1e3 * med / B}
    out['one_by_one_over_side_by_side_both_pairs'] = out['one_by_one']['ms_per_call'] / out['side_by_side_both_pairs']['ms_per_call']
    out['one_by_one_over_side_by_side_outputs_only'] = out['one_by_one']['ms_per_call'] / out['side_by_side_outputs_only']['ms_per_call']
    out['batch_chunk'] = int(g._backend().option('batch_chunk'))
    out['fallbacks'] = int(g._backend().option('fallbacks'))
    return out


class Stop(Exception):
    """A step failed: nothing more is started on the device."""


def bench_line(tree, args, pick):
    """One fresh process of `tree`'s bench.py: the picked figures of its JSON lines.  A time limit, a non-zero exit status or
    no output raises Stop."""
    try:
        r = subprocess.run([sys.executable, os.path.join(tree, 'bench.py')] + args, cwd=tree, capture_output=True, text=True,
                           timeout=600)
    except subprocess.TimeoutExpired:
        raise Stop('bench.py %s in %s ran into its time limit' % (' '.join(args), tree))
    if r.returncode:
        raise Stop('bench.py %s in %s: exit status %d: %s' % (' '.join(args), tree, r.returncode, r.stderr[-300:]))
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith('{'):
            out.update(pick(json.loads(line)))
    if not out:
        raise Stop('bench.py %s in %s printed no JSON line' % (' '.join(args), tree))
    return out


def bench_legs(trees, runs, steps, warmup, res):
    """Fills res[leg][tree]; the first run that fails ends everything (Stop), what was taken so far stays in `res`."""
    head = lambda j: {'sweeps_per_s': j['value']} if 'sweeps/s' == j.get('unit') else {}

    def lat(j):
        if j.get('unit') != 'evaluations/s':
            return {}
        n = j['config']['workload'].split('N=')[1].split(',')[0]
        out = {'N%s_evaluations_per_s' % n: j['value']}
        if j.get('side_by_side'):
            out['N%s_side_by_side_per_s' % n] = j['side_by_side']['value']
        return out

    legs = {'headline': (['--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)], head),
            'latency': (['--latency', '--latency-only', '45,512', '--latency-cpu-s', '0', '--latency-mcmc', '0'], lat)}
    for leg, (args, pick) in legs.items():
        res[leg] = {name: {'runs': []} for name in trees}
        for _ in range(runs):
            for name, tree in trees.items():
                res[leg][name]['runs'].append(bench_line(tree, args, pick))
        for name in trees:
            rs = res[leg][name]['runs']
            for k in sorted({k for r in rs for k in r}):
                v = np.array([r[k] for r in rs if k in r])
                res[leg][name][k] = {'median': float(np.median(v)), 'min': float(v.min()), 'max': float(v.max()),
                                     'spread': float((v.max() - v.min()) / np.median(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='predict_batch_timing.json')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--bench-trees', nargs=2, metavar=('PARENT', 'THIS'), default=None)
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--bench-steps', type=int, default=10)
    ap.add_argument('--bench-warmup', type=int, default=2)
    a = ap.parse_args()
    res = {'shapes': [], 'bench': {}}
    failed = None
    # the first step that fails -- an error of the library, a benchmark process that dies or hangs -- is the last one: the
    # file then holds what was taken and the error, and the exit status is 1
    try:
        for N, p, q, kind, B, ns in SHAPES:
            res['shapes'].append(shape(N, p, q, kind, B, ns, max(9, a.reps)))
            print(json.dumps(res['shapes'][-1]), flush=True)
        if a.bench_trees:
            bench_legs({'parent': os.path.abspath(a.bench_trees[0]), 'this': os.path.abspath(a.bench_trees[1])}, a.bench_runs,
                       a.bench_steps, a.bench_warmup, res['bench'])
            print(json.dumps({k: {n: {m: w for m, w in v.items() if m != 'runs'} for n, v in leg.items()}
                              for k, leg in res['bench'].items()}), flush=True)
        else:
            res['bench'] = {'not_taken': 'no --bench-trees given'}
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
        res['not_taken'] = 'everything after the failed step: shapes %d of %d taken' % (len(res['shapes']), len(SHAPES))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    if failed:
        print('stopped: ' + failed, file=sys.stderr, flush=True)
        sys.exit(1)


if __name__ == '__main__':
    main()
