"""Speed of this build against the parent commit's build after the kernel variants' selection moved into one dispatcher
(with_flags): the device code is the parent's, so only the host's way to a launch can have moved.  Two launch-bound figures
exercise it:

* ms per warm nELBO evaluation at N = 45, p = q = 2 (the one-tile path: set-up, loop under the stop rule, read-back);
* ms per side-by-side call of 256 evaluations at N = 45 (nELBO_batch, warm),

and bench.py's headline.  The protocol is profiles/elbo_bound_timing.py's: every leg is a FRESH process that takes every figure
once; the legs alternate (parent_a, this, parent_b) for --rounds rounds and a figure is the median over the rounds.  The parent
runs twice per round: the range of all its values is the parent's own run-to-run spread, the margin this build's median is held
to.  bench.py runs in both trees alternately, --bench-rounds times each; the parent's own range is its margin.  The script
reports booleans and asserts nothing.

usage: python profiles/variant_dispatch_timing.py --parent-tree DIR [--out FILE] [--rounds R] [--bench-rounds R]
The first leg that fails is the last: the JSON then holds what was taken and the error, and the exit status is 1."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = ('nelbo_N45_ms', 'batch256_N45_ms')


def leg(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc, synth
    t, ys, es = synth.rv_series(45, 2)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(2, 2, 'SE'))
    g = gpyrn.inference(2, t, *[a for pair in zip(ys, es) for a in pair])
    g.set_components(nodes, weights, means, jit)
    x = np.array(g.get_parameters(), dtype=float)
    g.ELBOcalc()
    out = {}
    sys.stdout = open(os.devnull, 'w')                    # (nELBO prints its progress line)
    try:
        for k in range(5):
            g.nELBO(x * (1.0 + 1e-4 * (k % 3)))
        t0 = time.perf_counter()
        for k in range(100):
            g.nELBO(x * (1.0 + 1e-4 * (k % 3)))           # changed hyper-parameters: every evaluation pays its set-up
        out['nelbo_N45_ms'] = 1e3 * (time.perf_counter() - t0) / 100
        keep = (np.array(g._mu), np.array(g._var))
        sets = [x * (1.0 + 1e-4 * (k % 7)) for k in range(256)]
        for _ in range(2):
            g._mu, g._var = keep
            g.nELBO_batch(sets)
        t0 = time.perf_counter()
        for _ in range(10):
            g._mu, g._var = keep
            g.nELBO_batch(sets)
        out['batch256_N45_ms'] = 1e3 * (time.perf_counter() - t0) / 10
    finally:
        sys.stdout = sys.__stdout__
    ctx = g._backend()
    out['batch_chunk'], out['fallbacks'] = int(ctx.option('batch_chunk')), int(ctx.option('fallbacks'))
    print(json.dumps(out), flush=True)


def child(tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', tree], capture_output=True, text=True, timeout=200)
    if r.returncode:
        raise RuntimeError('the leg on %s ended with status %d: %s' % (tree, r.returncode, r.stderr[-400:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench(tree):
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '3'], cwd=tree, capture_output=True,
                       text=True, timeout=400)
    if r.returncode:
        raise RuntimeError('bench.py in %s ended with status %d: %s' % (tree, r.returncode, r.stderr[-400:]))
    row = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    return {k: row.get(k) for k in ('metric', 'value', 'unit', 'ms_per_step') if row.get(k) is not None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='variant_dispatch_timing.json')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--parent-tree', required='--leg' not in sys.argv)
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(a.leg)
        return
    parent = os.path.abspath(a.parent_tree)
    order = [('parent_a', parent), ('this', HERE), ('parent_b', parent)]
    res = {'rounds': a.rounds, 'legs_per_round': [o[0] for o in order], 'runs': {o[0]: [] for o in order}}
    failed = None
    try:
        for r in range(a.rounds):
            for name, tree in order:
                res['runs'][name].append(child(tree))
            print('round', r + 1, json.dumps({n: res['runs'][n][-1] for n, _ in order}), flush=True)
        med = {n: {f: float(np.median([x[f] for x in rs])) for f in FIGURES} for n, rs in res['runs'].items()}
        both = {f: [x[f] for x in res['runs']['parent_a'] + res['runs']['parent_b']] for f in FIGURES}
        pmed = {f: float(np.median(both[f])) for f in FIGURES}
        res['median_ms'] = dict(med, parent=pmed)
        res['parent_rel_range_of_all_runs'] = {f: (max(both[f]) - min(both[f])) / pmed[f] for f in FIGURES}
        res['parent_rel_distance_of_medians'] = {f: abs(med['parent_a'][f] - med['parent_b'][f]) / pmed[f] for f in FIGURES}
        res['this_over_parent'] = {f: med['this'][f] / pmed[f] for f in FIGURES}
        res['this_not_slower_beyond_parent_range'] = {f: bool(med['this'][f] / pmed[f] - 1.0 <= res['parent_rel_range_of_all_runs'][f])
                                                      for f in FIGURES}
        res['bench'] = {'parent': [], 'this': []}
        for _ in range(a.bench_rounds):
            for name, tree in (('parent', parent), ('this', HERE)):
                res['bench'][name].append(bench(tree))
            print('bench', json.dumps({n: res['bench'][n][-1] for n in ('parent', 'this')}), flush=True)
        val = {n: [b['value'] for b in res['bench'][n]] for n in ('parent', 'this')}
        pm = float(np.median(val['parent']))
        res['bench_headline'] = {'parent_median': pm, 'this_median': float(np.median(val['this'])),
                                 'parent_rel_range': (max(val['parent']) - min(val['parent'])) / pm,
                                 'this_over_parent': float(np.median(val['this'])) / pm}
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}), flush=True)
    sys.exit(1 if failed else 0)


if __name__ == '__main__':
    main()
