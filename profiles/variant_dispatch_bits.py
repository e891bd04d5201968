"""Bits of this build against the parent commit's build, after the kernel variants' selection moved into one dispatcher
(with_flags) and the one-tile wrappers were folded: the device code is the parent's, so every result must be the parent's, bit
for bit; a difference means another kernel or argument was selected.

Each tree runs in a FRESH child process (--leg TREE FILE) that writes its arrays to FILE; the parent process compares with
np.array_equal:

* ELBOcalc at N = 45, p = q = 2 in the eight combinations of (data mask, sweep order, ELBO form): history, trips, state;
* nELBO_and_grad_batch (three forced sweeps and the loop under the stop rule) and predict_batch(from_sweeps=True) with B = 8 on
  one tile, for plain, masked and bound;
* one forced sweep at config 3's shape: ELBO, parts, state.

usage: python profiles/variant_dispatch_bits.py --parent-tree DIR [--out FILE]   (exit status 1 on any difference or error)"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = list(itertools.product((False, True), ('reference', 'sequential'), ('reference', 'bound')))


def leg(tree, path):
    sys.path.insert(0, os.path.abspath(tree))
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc, synth
    assert os.path.abspath(os.path.dirname(os.path.dirname(gpyrn.__file__))) == os.path.abspath(tree)

    def model(N, p, q, kind, masked=False, order='reference', form='reference', **kw):
        t, ys, es = synth.rv_series(N, p)
        nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
        y, e = np.array(ys), np.array(es)
        mask = None
        if masked:
            rng = np.random.RandomState(3)
            mask = np.ones((p, N), dtype=bool)
            for i in range(p):
                mask[i, rng.choice(N, N // 5, replace=False)] = False
            for n in np.flatnonzero(~mask.any(axis=0)):
                mask[0, n] = True
            y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
        g = gpyrn.inference(q, t, *[a for i in range(p) for a in (y[i], e[i])], mask=mask, sweep_order=order,
                            sequential_under_mask=True, batch_under_mask=True, elbo=form, **kw)
        g.set_components(nodes, weights, means, jit)
        return g

    out = {}
    sys.stdout = open(os.devnull, 'w')
    for masked, order, form in COMBOS:
        key = 'elbocalc_%d_%s_%s' % (masked, order, form)
        g = model(45, 2, 2, 'SE', masked, order, form)
        E, mu, var, it = g.ELBOcalc()
        assert g.last_info == 0
        out[key + '_hist'], out[key + '_mu'], out[key + '_var'], out[key + '_it'] = np.array(g._elbo_history), mu, var, np.array(it)
    for name, masked, form in (('plain', False, 'reference'), ('masked', True, 'reference'), ('bound', False, 'bound')):
        g = model(45, 2, 2, 'SE', masked, 'reference', form, predict='variational')
        x = np.array(g.get_parameters(), dtype=float)
        sets = [x * (1.0 + 0.01 * k) for k in range(8)]
        start = g._initMuVar(g.nodes, g.weights, g.jitters)
        vals, grads = g.nELBO_and_grad_batch(sets, sweeps=3, start=start)
        out['batch_%s_forced_vals' % name], out['batch_%s_forced_grads' % name] = np.array(vals), grads
        g.ELBOcalc()
        keep = (np.array(g._mu), np.array(g._var))
        vals, grads = g.nELBO_and_grad_batch(sets, max_iter=100)
        out['batch_%s_loop_vals' % name], out['batch_%s_loop_grads' % name] = np.array(vals), grads
        g._mu, g._var = keep
        mean, var = g.predict_batch(sets, tstar=np.linspace(g.time[0] - 1.0, g.time[-1] + 1.0, 30), from_sweeps=True, max_iter=100)
        out['batch_%s_pred_mean' % name], out['batch_%s_pred_var' % name] = mean, var
        assert g.last_info == 0 and g._backend().option('batch_chunk') == 8
    N, p, q, kind = synth.CONFIGS[3]
    g = model(N, p, q, kind)
    ctx = g._setup_device(g.nodes, g.weights, g.means, g.jitters)
    ctx.set_muvar(*g._initMuVar(g.nodes, g.weights, g.jitters))
    elbo, parts, info = ctx.sweep(1, commit=True)
    assert info == 0
    out['config3_elbo'], out['config3_parts'] = elbo, parts
    out['config3_mu'], out['config3_var'] = ctx.get_muvar()
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default='variant_dispatch_bits.json')
    ap.add_argument('--leg', nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(*a.leg)
        return
    res, failed = {'equal': {}, 'all_equal': False}, None
    try:
        with tempfile.TemporaryDirectory() as tmp:
            files = {}
            for name, tree in (('parent', os.path.abspath(a.parent_tree)), ('this', HERE)):
                files[name] = os.path.join(tmp, name + '.npz')
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', tree, files[name]], capture_output=True,
                                   text=True, timeout=500)
                if r.returncode:
                    raise RuntimeError('the leg on %s ended with status %d: %s' % (tree, r.returncode, r.stderr[-600:]))
            pa, th = np.load(files['parent']), np.load(files['this'])
            assert sorted(pa.files) == sorted(th.files)
            for k in sorted(pa.files):
                res['equal'][k] = bool(np.array_equal(pa[k], th[k]) and np.all(np.isfinite(th[k])))
            res['all_equal'] = all(res['equal'].values())
            res['arrays'], res['values_compared'] = len(pa.files), int(sum(pa[k].size for k in pa.files))
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    sys.exit(0 if res['all_equal'] and not failed else 1)


if __name__ == '__main__':
    main()
