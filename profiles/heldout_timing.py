"""Cost of a k-fold cross-validation side by side (inference.cross_validate -> gprn_elbocalc_batch_heldout) against the same
folds one by one on the SAME build, and of carrying per-evaluation masks at all against the parent commit's build:

* the feature: ms per fold for N = 45 (p = q = 1, k = 10), N = 497 (p = 4, q = 1, k = 5) and N = 512 (p = 3, q = 2, k = 5),
  folds from cv_folds(k, rng=0), every fold from its own cold start.  One by one: per fold a FRESH object with mask=fold, then
  ELBOcalc and the variational predict at the data times -- the only way to a held-out score without this call.  No ratio is
  fixed in advance: the script records what it measures;
* nothing else moved: nELBO_batch without a mask and nELBO_batch under batch_under_mask at the same shapes, this build against
  the parent's (--parent-tree DIR, a built checkout of the parent commit), and with --bench-trees bench.py's headline in both
  trees, alternately, twice each.

Every leg is a FRESH process that takes every figure once (the mean of a few calls behind a warm-up call); the legs alternate
(parent_a, this, parent_b) for --rounds rounds (default 9), and a figure is the median over the rounds.  The parent runs twice
per round: the range of all its values is its own run-to-run spread, and "inside the parent's own run-to-run range" is measured
against it.  The script reports booleans; it asserts nothing.

usage: python profiles/heldout_timing.py [--parent-tree DIR] [--out FILE] [--rounds R] [--bench-trees]
(default --out: heldout_timing.json in the working directory).  Without --parent-tree the parent's legs are "not measured".
The first leg that fails is the last: the JSON then holds what was taken and the error, the exit status is 1, and nothing more
is started on the device."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (N, p, q, kernels, folds, vectors of an nELBO_batch call, repetitions of a side-by-side call)
SHAPES = {'N45': (45, 1, 1, 'SE', 10, 256, 5), 'N497': (497, 4, 1, 'QP', 5, 32, 3), 'N512': (512, 3, 2, 'QP', 5, 32, 3)}


def _tree():
    """--leg NAME TREE: the package of that checkout; else this one's."""
    if '--leg' in sys.argv:
        return os.path.abspath(sys.argv[sys.argv.index('--leg') + 2])
    return HERE


sys.path.insert(0, _tree())
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402


def _model(N, p, q, kind, **kw):
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair], **kw)
    g.set_components(nodes, weights, means, jit)
    return g


def _partial_mask(p, N, q):
    """a fifth of every output unobserved, every time with an observed output where q >= 2 asks for one"""
    rng = np.random.RandomState(7)
    mask = rng.uniform(size=(p, N)) > 0.2
    if p == 1:
        return mask
    for n in np.flatnonzero(~mask.any(axis=0)):
        mask[rng.randint(p), n] = True
    return mask


def _vectors(g, B):
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(11)
    return [x0 * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, x0.size)) for _ in range(B)]


def _quiet(f, *a, **kw):
    """(ELBOcalc and nELBO_batch report on stdout; the leg's last line must be its JSON)"""
    keep = sys.stdout
    sys.stdout = open(os.devnull, 'w')
    try:
        return f(*a, **kw)
    finally:
        sys.stdout.close()
        sys.stdout = keep


def _close(g):
    g._backend().close()
    g._ctx = None


def leg(name):
    out = {'fallbacks': 0}
    for shape, (N, p, q, kind, k, B, reps) in SHAPES.items():
        # ---- nELBO_batch without a mask and under batch_under_mask: in every leg
        for what, kw in (('elbo_batch', {}), ('masked_elbo_batch', dict(mask=_partial_mask(p, N, q), batch_under_mask=True))):
            g = _model(N, p, q, kind, **kw)
            _quiet(g.ELBOcalc)
            sets = _vectors(g, B)
            state = (g._mu, g._var)
            _quiet(g.nELBO_batch, sets)
            g._mu, g._var = state
            t0 = time.perf_counter()
            for _ in range(reps):
                _quiet(g.nELBO_batch, sets)
                g._mu, g._var = state
            out['%s_ms_per_vector_%s' % (what, shape)] = 1e3 * (time.perf_counter() - t0) / (reps * B)
            out['fallbacks'] += int(g._backend().option('fallbacks'))
            _close(g)
        if name.startswith('parent'):
            continue
        # ---- the k folds side by side ...
        g = _model(N, p, q, kind)
        folds = g.cv_folds(k, rng=0)
        cv = _quiet(g.cross_validate, folds)
        t0 = time.perf_counter()
        for _ in range(reps):
            cv = _quiet(g.cross_validate, folds)
        out['side_by_side_ms_per_fold_' + shape] = 1e3 * (time.perf_counter() - t0) / (reps * k)
        out['elpd_' + shape] = float(cv.elpd[0])
        out['fallbacks'] += int(g._backend().option('fallbacks'))
        _close(g)
        # ... and one by one: a fresh mask= object per fold, ELBOcalc, the variational predict at the data times
        def one(f):
            g1 = _model(N, p, q, kind, mask=np.asarray(folds[f]), predict='variational')
            _quiet(g1.ELBOcalc)
            pred = g1._Prediction(tstar=np.asarray(g1.time, dtype=float))
            _close(g1)
            return pred
        one(0)
        t0 = time.perf_counter()
        for f in range(k):
            one(f)
        out['one_by_one_ms_per_fold_' + shape] = 1e3 * (time.perf_counter() - t0) / k
    return out


def child(name, tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, tree], capture_output=True, text=True, timeout=400)
    if r.returncode:
        raise RuntimeError('leg %s on %s ended with status %d: %s' % (name, tree, r.returncode, r.stderr[-400:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench(tree, args):
    r = subprocess.run([sys.executable, 'bench.py'] + args, cwd=tree, capture_output=True, text=True, timeout=300)
    if r.returncode:
        raise RuntimeError('bench.py %s in %s ended with status %d: %s' % (' '.join(args), tree, r.returncode, r.stderr[-400:]))
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    return [{f: row.get(f) for f in ('metric', 'value', 'unit', 'ms_per_step', 'config', 'schedule') if row.get(f) is not None}
            for row in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='heldout_timing.json')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--bench-trees', action='store_true')
    ap.add_argument('--leg', nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg[0])), flush=True)
        return
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    order = [o for o in (('parent_a', parent), ('this', HERE), ('parent_b', parent)) if o[1]]
    res = {'rounds': a.rounds, 'shapes': {s: dict(N=v[0], p=v[1], q=v[2], kernels=v[3], folds=v[4], B=v[5]) for s, v in SHAPES.items()},
           'legs_per_round': [o[0] for o in order], 'runs': {o[0]: [] for o in order}}
    if not parent:
        res['parent'] = 'not measured'
    res['bench'] = 'not measured'
    failed = None
    try:
        for r in range(a.rounds):
            for name, tree in order:
                res['runs'][name].append(child(name, tree))
            print('round', r + 1, json.dumps({o[0]: res['runs'][o[0]][-1] for o in order}), flush=True)
        med = {n: {f: float(np.median([x[f] for x in rs if f in x])) for f in rs[0]} for n, rs in res['runs'].items()}
        res['median'] = med
        res['fallbacks'] = {n: int(sum(x.get('fallbacks', 0) for x in rs)) for n, rs in res['runs'].items()}
        res['feature'] = {}
        for s, v in SHAPES.items():
            one, side = med['this']['one_by_one_ms_per_fold_' + s], med['this']['side_by_side_ms_per_fold_' + s]
            res['feature'][s] = {'folds': v[4], 'one_by_one_ms_per_fold': one, 'side_by_side_ms_per_fold': side, 'ratio': one / side,
                                 'side_by_side_is_faster': bool(side < one), 'elpd': med['this']['elpd_' + s]}
        if parent:
            both = res['runs']['parent_a'] + res['runs']['parent_b']
            res['nothing_else_moved'] = {}
            for s in SHAPES:
                for what in ('elbo_batch', 'masked_elbo_batch'):
                    f = '%s_ms_per_vector_%s' % (what, s)
                    vals = [x[f] for x in both]
                    pmed = float(np.median(vals))
                    spread = (max(vals) - min(vals)) / pmed
                    res['nothing_else_moved'][what + '_' + s] = {
                        'parent_ms_per_vector': pmed, 'this_ms_per_vector': med['this'][f], 'this_over_parent': med['this'][f] / pmed,
                        'parent_rel_range_of_all_runs': spread, 'inside_the_parents_range': bool(abs(med['this'][f] / pmed - 1.0) <= spread)}
        if a.bench_trees and parent:
            res['bench'] = {'parent': [], 'this': []}
            for _ in range(2):
                for name, tree in (('parent', parent), ('this', HERE)):
                    res['bench'][name].append(bench(tree, ['--gpus', '1', '--steps', '20', '--warmup', '3']))
            print(json.dumps(res['bench']), flush=True)
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({f: v for f, v in res.items() if f != 'runs'}), flush=True)
    sys.exit(1 if failed else 0)


if __name__ == '__main__':
    main()
