"""Cost of one joint posterior curve per vector, side by side (inference.sample_posterior_batch -> gprn_elbocalc_batch_draws)
against the only other way to the same curves ON THIS BUILD -- per vector, nELBO then sample_posterior in the variational form
-- and of carrying the pass at all against the parent commit's build:

* the feature: curves per second for the three shapes of the ELBO batches (N = 45, p = q = 1, B = 256; N = 497, p = 4, q = 1,
  B = 32; N = 512, p = 3, q = 2, B = 32) at n = 1 draw and ns = 1000 times, warm start, 1 % perturbations;
* the pass's share of a side-by-side call, from the library's own timers (GPRN_BATCH_TIMERS=1: the pass's field of the chunk's
  line over its total);
* nothing else moved: nELBO_batch (gprn_elbocalc_batch without a pass) at the first two shapes, this build against the parent's
  (--parent-tree DIR, a built checkout of the parent commit).

Every leg is a FRESH process that takes every figure once (the mean of a few calls behind a warm-up call); the legs alternate
(parent_a, this, parent_b, share) for --rounds rounds (default 9), and a figure is the median over the rounds.  The parent
runs twice per round: the range of all its values is its own run-to-run spread, and "inside the parent's own run-to-run
range" is measured against it.  The script reports booleans; it asserts nothing.

--bench-trees: ahead of the rounds bench.py's headline in the parent's tree and in this one, alternately, twice each.

usage: python profiles/draw_batch_timing.py [--parent-tree DIR] [--out FILE] [--rounds R] [--bench-trees] [--budget-s S]
(default --out: draw_batch_timing.json in the working directory; --budget-s: no round is started that would not fit into S
seconds at the pace so far, and `rounds_done` says how many the medians are over).  Without --parent-tree the parent's legs are "not
measured".  The first leg that fails is the last: the JSON then holds what was taken and the error, the exit status is 1, and
nothing more is started on the device."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (N, p, q, kernels, B, vectors taken one by one, repetitions of a side-by-side call)
SHAPES = {'N45': (45, 1, 1, 'SE', 256, 16, 3), 'N497': (497, 4, 1, 'QP', 32, 4, 2), 'N512': (512, 3, 2, 'QP', 32, 4, 2)}
PARENT_SHAPES = ('N45', 'N497')
NS = 1000


def _tree():
    """--leg NAME TREE: the package of that checkout; else this one's."""
    if '--leg' in sys.argv:
        return os.path.abspath(sys.argv[sys.argv.index('--leg') + 2])
    return HERE


sys.path.insert(0, _tree())
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402


def _model(N, p, q, kind):
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair], predict='variational')
    g.set_components(nodes, weights, means, jit)
    g.ELBOcalc()                                           # the warm start every vector shares
    span = np.ptp(t)
    return g, np.linspace(t.min() - 0.2 * span, t.max() + 0.2 * span, NS)


def _vectors(g, B):
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(11)
    return [x0 * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, x0.size)) for _ in range(B)]


def _quiet(f, *a, **kw):
    """(nELBO and nELBO_batch report on stdout; the leg's last line must be its JSON)"""
    keep = sys.stdout
    sys.stdout = open(os.devnull, 'w')
    try:
        return f(*a, **kw)
    finally:
        sys.stdout.close()
        sys.stdout = keep


def leg(name):
    out = {'fallbacks': 0}
    parent = name.startswith('parent')
    for shape, (N, p, q, kind, B, n_one, reps) in SHAPES.items():
        if parent and shape not in PARENT_SHAPES:
            continue
        g, ts = _model(N, p, q, kind)
        sets = _vectors(g, B)
        state = (g._mu, g._var)
        # ---- nELBO_batch alone: in every leg
        _quiet(g.nELBO_batch, sets)
        g._mu, g._var = state
        t0 = time.perf_counter()
        for _ in range(reps):
            _quiet(g.nELBO_batch, sets)
            g._mu, g._var = state
        out['elbo_batch_ms_per_vector_' + shape] = 1e3 * (time.perf_counter() - t0) / (reps * B)
        if not parent:
            # ---- one by one: per vector, nELBO then sample_posterior in the variational form
            def one(x):
                _quiet(g.nELBO, x)
                return g.sample_posterior(tstar=ts, n=1, rng=1)
            one(sets[0])
            g._mu, g._var = state
            t0 = time.perf_counter()
            for x in sets[1:1 + n_one]:
                one(x)
                g._mu, g._var = state
            out['one_by_one_ms_per_curve_' + shape] = 1e3 * (time.perf_counter() - t0) / n_one
            # ---- side by side
            g.sample_posterior_batch(sets, tstar=ts, n=1, rng=1)
            g._mu, g._var = state
            t0 = time.perf_counter()
            for _ in range(reps):
                g.sample_posterior_batch(sets, tstar=ts, n=1, rng=1)
                g._mu, g._var = state
            out['side_by_side_ms_per_curve_' + shape] = 1e3 * (time.perf_counter() - t0) / (reps * B)
        out['fallbacks'] += int(g._backend().option('fallbacks'))
        g._backend().close()
        g._ctx = None
    return out


def child(name, tree, timers=False):
    env = dict(os.environ)
    if timers:
        env['GPRN_BATCH_TIMERS'] = '1'
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, tree], capture_output=True, text=True,
                       timeout=300, env=env)
    if r.returncode:
        raise RuntimeError('leg %s on %s ended with status %d: %s' % (name, tree, r.returncode, r.stderr[-400:]))
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if timers:
        # the chunk lines that ran a draw pass, per problem size: the pass's share of the call
        shares = {}
        for ln in r.stderr.splitlines():
            m = re.search(r'prediction(?: / draw)? pass (\d+) \| total (\d+)', ln)
            if not m or int(m.group(1)) == 0:
                continue
            key = 'N45' if 'one tile' in ln else ('N497' if 'N = 497' in ln else 'N512')
            shares.setdefault(key, []).append(float(m.group(1)) / float(m.group(2)))
        out = {'pass_share_' + k: float(np.median(v[1:] if len(v) > 1 else v)) for k, v in shares.items()}   # (behind the warm-up)
    return out


def bench(tree, args):
    r = subprocess.run([sys.executable, 'bench.py'] + args, cwd=tree, capture_output=True, text=True, timeout=300)
    if r.returncode:
        raise RuntimeError('bench.py %s in %s ended with status %d: %s' % (' '.join(args), tree, r.returncode, r.stderr[-400:]))
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    return [{k: row.get(k) for k in ('metric', 'value', 'unit', 'ms_per_step', 'config', 'schedule') if row.get(k) is not None}
            for row in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='draw_batch_timing.json')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-trees', action='store_true')
    ap.add_argument('--budget-s', type=float, default=0.0, help='seconds the rounds may take; 0: all of --rounds')
    ap.add_argument('--leg', nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg[0])), flush=True)
        return
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    order = [('parent_a', parent, False), ('this', HERE, False), ('parent_b', parent, False), ('share', HERE, True)]
    order = [o for o in order if o[1]]
    res = {'ns': NS, 'n_draws': 1, 'rounds': a.rounds,
           'shapes': {k: dict(N=v[0], p=v[1], q=v[2], kernels=v[3], B=v[4]) for k, v in SHAPES.items()},
           'legs_per_round': [o[0] for o in order], 'runs': {o[0]: [] for o in order}}
    if not parent:
        res['parent'] = 'not measured'
        res['bench'] = 'not measured'
    failed = None
    began = time.time()
    try:
        if a.bench_trees and parent:
            res['bench'] = {'parent': [], 'this': []}
            for _ in range(2):
                for name, tree in (('parent', parent), ('this', HERE)):
                    res['bench'][name].append(bench(tree, ['--gpus', '1', '--steps', '20', '--warmup', '3']))
            print(json.dumps(res['bench']), flush=True)
        for r in range(a.rounds):
            if a.budget_s and r and time.time() - began > a.budget_s * r / (r + 1.0):
                break                                      # (another round would not fit: the medians are over rounds_done)
            for name, tree, timers in order:
                res['runs'][name].append(child(name, tree, timers))
            print('round', r + 1, json.dumps({o[0]: res['runs'][o[0]][-1] for o in order}), flush=True)
            res['rounds_done'] = r + 1
            with open(a.out, 'w') as f:                    # (what was taken so far, should the run be cut short)
                json.dump(res, f, indent=1)
        med = {n: {f: float(np.median([x[f] for x in rs if f in x])) for f in rs[0]} for n, rs in res['runs'].items()}
        res['median'] = med
        res['fallbacks'] = {n: int(sum(x.get('fallbacks', 0) for x in rs)) for n, rs in res['runs'].items()}
        res['feature'] = {}
        for s in SHAPES:
            one, side = med['this']['one_by_one_ms_per_curve_' + s], med['this']['side_by_side_ms_per_curve_' + s]
            res['feature'][s] = {'one_by_one_ms_per_curve': one, 'side_by_side_ms_per_curve': side,
                                 'curves_per_second_one_by_one': 1e3 / one, 'curves_per_second_side_by_side': 1e3 / side,
                                 'ratio': one / side, 'side_by_side_is_faster': bool(side < one),
                                 'draw_pass_share_of_the_call': med['share'].get('pass_share_' + s)}
        if parent:
            both = res['runs']['parent_a'] + res['runs']['parent_b']
            res['nothing_else_moved'] = {}
            for s in PARENT_SHAPES:
                f = 'elbo_batch_ms_per_vector_' + s
                vals = [x[f] for x in both]
                pmed = float(np.median(vals))
                spread = (max(vals) - min(vals)) / pmed
                res['nothing_else_moved'][s] = {'parent_ms_per_vector': pmed, 'this_ms_per_vector': med['this'][f],
                                                'this_over_parent': med['this'][f] / pmed,
                                                'parent_rel_range_of_all_runs': spread,
                                                'inside_the_parents_range': bool(abs(med['this'][f] / pmed - 1.0) <= spread)}
        if parent and not a.bench_trees:
            res['bench'] = 'not measured'
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}), flush=True)
    sys.exit(1 if failed else 0)


if __name__ == '__main__':
    main()
