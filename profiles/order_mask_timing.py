"""Cost of the sequential sweep order UNDER A DATA MASK (inference(..., mask=, sweep_order='sequential',
sequential_under_mask=True); option "order_mask") against the reference's order under the same mask:

* ms per forced sweep at BASELINE config 3 (N = 4096, p = 3, q = 2) with 10 % of output 0 masked: the launch path, where the
  later group adds the masked mean refresh (four O(N^2) launches) to its phase, in front of the mask's rows;
* the same at N = 45, p = 2, q = 2: the one-tile path, one masked refresh launch more per half-sweep;
* the option-off column: the UNMASKED sweep in both orders on this tree (option "order_mask" = 0: the instantiations the
  parent commit has) and, with --parent-tree DIR (a built checkout of the parent commit), the same on the parent's build,
  measured in a fresh process alternately with this tree's.

usage: python profiles/order_mask_timing.py [--out FILE] [--sweeps S] [--parent-tree DIR] [--rounds R]
(default --out: order_mask_timing.json in the working directory).  Sweep rates: device-synchronised host wall clock around
one call of S forced sweeps (uncommitted), after a warm-up call; the two orders alternate on one context, best of three.
The first step that fails is the last: the JSON then holds what was taken and the error, the exit status is 1, and nothing
more is started on the device."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ('reference', 'sequential')
# beside config 3: (label, N, p, q, kernels, forced sweeps per call)
SHAPES = [('one_tile_N45_q2', 45, 2, 2, 'SE', 64)]


def _tree():
    """--child TREE: the package of that checkout (the option-off leg on the parent's build); else this one's."""
    if '--child' in sys.argv:
        return os.path.abspath(sys.argv[sys.argv.index('--child') + 1])
    return HERE


sys.path.insert(0, _tree())
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402


def shapes(sweeps):
    N, p, q, kind = synth.CONFIGS[3]
    return [('config3', N, p, q, kind, sweeps)] + SHAPES


def make_mask(p, N, frac=0.10, seed=11):
    """`frac` of output 0 masked (seeded); every time keeps an observed output."""
    mask = np.ones((p, N), dtype=bool)
    mask[0, np.random.RandomState(seed).choice(N, max(1, int(round(frac * N))), replace=False)] = False
    return mask


def model(N, p, q, kind, **kw):
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair], **kw)
    g.set_components(nodes, weights, means, jit)
    return g


def sweep_ms(g, n, rounds=3):
    """ms per forced sweep of `g` in both orders, alternating on its one context."""
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
    out = {'sweeps': n, 'ms_per_sweep': best, 'sequential_over_reference': best['sequential'] / best['reference'],
           'fallbacks': int(ctx.option('fallbacks'))}
    ctx.close()
    g._ctx = None
    return out


def unmasked(sweeps):
    """The option-off column: no mask, both orders (what the parent commit's build runs too)."""
    res = {}
    for label, N, p, q, kind, n in shapes(sweeps):
        res[label] = {'N': N, 'p': p, 'q': q, **sweep_ms(model(N, p, q, kind), n)}
    return res


def child(tree, sweeps):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tree, '--sweeps', str(sweeps)],
                       capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise RuntimeError('the option-off leg on %s ended with status %d: %s' % (tree, r.returncode, r.stderr[-400:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='order_mask_timing.json')
    ap.add_argument('--sweeps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(unmasked(a.sweeps)), flush=True)
        return
    res = {'masked': {}, 'option_off': {}}
    failed = None
    try:
        for label, N, p, q, kind, n in shapes(a.sweeps):
            mask = make_mask(p, N)
            g = model(N, p, q, kind, mask=mask, sequential_under_mask=True)
            res['masked'][label] = {'N': N, 'p': p, 'q': q, 'masked_entries_per_output': (~mask).sum(axis=1).tolist(),
                                    **sweep_ms(g, n)}
            print(json.dumps({label: res['masked'][label]}), flush=True)
        # the option-off column, in fresh processes: this tree and the parent's alternate
        trees = {'this': HERE}
        if a.parent_tree:
            trees['parent'] = os.path.abspath(a.parent_tree)
        else:
            res['option_off']['parent'] = {'not_taken': 'no --parent-tree given'}
        runs = {k: [] for k in trees}
        for _ in range(a.rounds):
            for k, tree in trees.items():
                runs[k].append(child(tree, a.sweeps))
        for k, rs in runs.items():
            res['option_off'][k] = {label: {o: min(r[label]['ms_per_sweep'][o] for r in rs) for o in ORDERS} for label in rs[0]}
        if a.parent_tree:
            res['option_off']['this_over_parent'] = {
                label: {o: res['option_off']['this'][label][o] / res['option_off']['parent'][label][o] for o in ORDERS}
                for label in res['option_off']['this']}
        print(json.dumps(res['option_off']), flush=True)
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    if failed:
        print('stopped: ' + failed, file=sys.stderr, flush=True)
        sys.exit(1)


if __name__ == '__main__':
    main()
