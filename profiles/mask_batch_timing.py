"""Side-by-side ELBO batches under a data mask (inference(..., batch_under_mask=True), option "batch_mask") against

* the same list one by one on the SAME object with batch_under_mask = False -- the path this change leaves as it was, and
  so the baseline -- and
* the unmasked batch of the same shape (the price of the mask),

each with and without gradients (nELBO_batch; nELBO_and_grad_batch, whose one-by-one branch is each vector's loop from the
same state and gprn_grad_elbo behind it), at the ELBO batches' three shapes:

  N = 45, p = q = 1, B = 256   (one tile)        10 % of the times masked in every output: the node has rows U too
  N = 497, p = 4, q = 1, B = 32                  10 % and 50 % of one output masked
  N = 512, p = 3, q = 2, B = 32                  10 % and 50 % of one output masked

Every leg starts from the same converged state at the unperturbed parameters (nELBO's warm start) and perturbs them by 1 %;
device-synchronised host wall clock around the Python call; per round the forms run one after the other (alternating, so
that drift of the box meets all of them alike), median of `--reps` rounds after a warm-up round that sizes the buffers.

With --bench-trees A B (two checkouts of the project, each built): bench.py's headline and bench.py --latency at N = 45 and
512 run alternately in fresh processes, `--bench-runs` times per tree (profiles/grad_batch_timing.py's leg).  The first step
that fails is the last: the JSON then holds what was taken and the error, the exit status is 1, and nothing more is started
on the device.

usage: python profiles/mask_batch_timing.py [--out FILE] [--reps R] [--bench-trees PARENT THIS] [--bench-runs K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import covfunc, meanfunc, synth  # noqa: E402
from profiles.grad_batch_timing import bench_legs  # noqa: E402

# (N, p, q, kernels, B, masks: (label, fraction, 'times' = every output at those times | 'output' = output 0 alone))
SHAPES = [(45, 1, 1, 'SE', 256, [('10 % of the times', 0.10, 'times')]),
          (497, 4, 1, 'QP', 32, [('10 % of one output', 0.10, 'output'), ('50 % of one output', 0.50, 'output')]),
          (512, 3, 2, 'QP', 32, [('10 % of one output', 0.10, 'output'), ('50 % of one output', 0.50, 'output')])]


def make_mask(p, N, frac, how, seed=11):
    rng = np.random.RandomState(seed)
    mask = np.ones((p, N), dtype=bool)
    idx = rng.choice(N, max(1, int(round(frac * N))), replace=False)
    if how == 'times':
        mask[:, idx] = False
    else:
        mask[0, idx] = False
    return mask


def model(N, p, q, kind, mask=None):
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    kw = {} if mask is None else {'mask': mask}
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair], **kw)
    g.set_components(nodes, weights, means, jit)
    return g


def one_mask(N, p, q, kind, B, label, frac, how, reps):
    mask = make_mask(p, N, frac, how)
    g = model(N, p, q, kind, mask)                            # masked: side by side or one by one, by its attribute
    u = model(N, p, q, kind)                                  # the unmasked batch of the same shape
    out = {'N': N, 'p': p, 'q': q, 'evaluations': B, 'mask': label, 'masked_entries_per_output': (~mask).sum(axis=1).tolist()}
    rng = np.random.RandomState(5)
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * (1.0 + 0.01 * rng.standard_normal(x0.size)) for _ in range(B)]
    warm = {}
    for name, m in (('masked', g), ('unmasked', u)):
        _, mu_w, var_w, trips = m.ELBOcalc()
        warm[name] = (np.array(mu_w), np.array(var_w))
        out['trips_of_the_warm_start_' + name] = int(trips)

    def leg(m, name, side, grad):
        def f():
            m._mu, m._var = warm[name]
            m.batch_under_mask = side
            return m.nELBO_and_grad_batch(sets) if grad else m.nELBO_batch(sets)
        return f

    legs = {}
    for grad in (False, True):
        tail = '_with_gradients' if grad else ''
        legs['masked_side_by_side' + tail] = leg(g, 'masked', True, grad)
        legs['masked_one_by_one' + tail] = leg(g, 'masked', False, grad)
        legs['unmasked_side_by_side' + tail] = leg(u, 'unmasked', False, grad)
    sys.stdout = open(os.devnull, 'w')                        # (nELBO / nELBO_batch print a progress line per call)
    try:
        times = {k: [] for k in legs}
        for r in range(reps + 1):                             # (round 0: the warm-up that sizes the buffers)
            for k, f in legs.items():
                t0 = time.perf_counter()
                res = f()
                dt = time.perf_counter() - t0
                if r:
                    times[k].append(dt)
                elif k == 'masked_side_by_side_with_gradients':
                    out['all_finite'] = bool(np.all(np.isfinite(res[0])) and np.all(np.isfinite(res[1])))
                    out['batch_chunk'] = int(g._backend().option('batch_chunk'))
    finally:
        sys.stdout.close()
        sys.stdout = sys.__stdout__
    for k, ts in times.items():
        med = float(np.median(ts))
        out[k] = {'ms_per_call': 1e3 * med, 'ms_min': 1e3 * min(ts), 'ms_max': 1e3 * max(ts), 'calls': len(ts),
                  'vectors_per_s': B / med, 'ms_per_vector': 1e3 * med / B}
    for tail in ('', '_with_gradients'):
        side, one, plain = (out[k + tail]['ms_per_call'] for k in ('masked_side_by_side', 'masked_one_by_one', 'unmasked_side_by_side'))
        out['side_by_side_over_one_by_one' + tail] = one / side
        out['masked_over_unmasked_batch' + tail] = side / plain
    out['fallbacks'] = int(g._backend().option('fallbacks')) + int(u._backend().option('fallbacks'))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='mask_batch_timing.json')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--bench-trees', nargs=2, metavar=('PARENT', 'THIS'), default=None)
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--bench-steps', type=int, default=10)
    ap.add_argument('--bench-warmup', type=int, default=2)
    a = ap.parse_args()
    res = {'shapes': [], 'bench': {}}
    failed = None
    try:
        for N, p, q, kind, B, masks in SHAPES:
            for label, frac, how in masks:
                res['shapes'].append(one_mask(N, p, q, kind, B, label, frac, how, a.reps))
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
        res['not_taken'] = 'everything after the failed step: %d legs taken' % len(res['shapes'])
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    if failed:
        print('stopped: ' + failed, file=sys.stderr, flush=True)
        sys.exit(1)


if __name__ == '__main__':
    main()
