"""Bits of this build against the parent commit's build, after the covariance fills were folded onto one body per shape
(csrc/fill.hip): the element arithmetic, grids and store patterns are the parent's, so every result must be the parent's, bit
for bit.

Each tree runs in a FRESH child process (--leg TREE FILE) with that tree's library (GPRN_HIP_LIB) and writes its arrays to
FILE; the parent process compares with np.array_equal(..., equal_nan=True):

* square fills (eval_kernel): SE, QP, HarmonicPeriodic, SHO, SE * Periodic and Polynomial (the full-matrix kernel) at N = 45
  and N = 200 (ld = 256: ten lower blocks);
* rectangular fills (test_fill_rect): both forms, single and batched, SE and SE * Periodic, ns = 1 and ns = ld + 3;
* nELBO_batch with B = 5 at N = 45 and B = 3 at N = 200 (the K2 copy and the set-up fill of both batch paths), one-kernel
  programs and a model whose node is a sum;
* predict_batch from states and from_sweeps=True (DIAG, the batched K* fills of both forms);
* sample_posterior_batch, two draws at times with a repeated value (batched K**, the coincide kernels);
* eval_kernel_grad of a composite, nELBO_and_grad_batch with grad_exact on and off.

usage: python profiles/fill_bodies_bits.py --parent-tree DIR [--out FILE]   (exit status 1 on any difference or error)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(tree, path):
    sys.path.insert(0, os.path.abspath(tree))
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc, synth
    assert os.path.abspath(os.path.dirname(os.path.dirname(gpyrn.__file__))) == os.path.abspath(tree)
    cf = covfunc

    def model(N, composite=False, **kw):
        t, ys, es = synth.rv_series(N, 2)
        if composite:
            nodes = [cf.Sum(cf.SquaredExponential(1.0, 7.0), cf.Matern32(0.5, 9.0))]
            weights = [cf.SquaredExponential(0.5, 15.0), cf.QuasiPeriodic(0.5, 16.0, 11.0, 1.2)]
            means, jit = [meanfunc.Constant(0.0), meanfunc.Constant(0.0)], [0.2, 0.2]
        else:
            nodes, weights, means, jit = synth.build_components(cf, meanfunc, synth.component_spec(2, 1, 'SE'))
        g = gpyrn.inference(1, t, ys[0], es[0], ys[1], es[1], **kw)
        g.set_components(nodes, weights, means, jit)
        used.append(g)
        return g

    def healthy():
        """every model so far ran its calls on the batched kernels: no call fell back, the last one ended well"""
        for g in used:
            assert g._backend().option('fallbacks') == 0 and g.last_info in (0, None), (g.last_info, g._backend().option('fallbacks'))

    used, out = [], {}
    stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
    se_per = cf.Multiplication(cf.SquaredExponential(1.1, 9.0), cf.Periodic(0.9, 5.3, 1.4))
    square = {'se': cf.SquaredExponential(1.3, 6.0), 'qp': cf.QuasiPeriodic(1.2, 20.0, 7.1, 0.8),
              'harmonic': cf.HarmonicPeriodic(2, 1.1, 9.3, 1.7), 'sho': cf.SHO(1.2, 8.0, 2.5), 'se_x_periodic': se_per,
              'polynomial': cf.Polynomial(0.7, 0.01, 0.5, 2.0)}
    for N in (45, 200):
        g = model(N)
        ctx = g._backend()
        ld = -(-N // 128) * 128
        for name, k in square.items():
            ops, pars = k._device_program()
            out['square_%s_%d' % (name, N)] = ctx.eval_kernel(ops, pars, 0.0 if name == 'polynomial' else 1e-6)
        s = np.random.RandomState(5).uniform(0.0, 2.0, N)
        s[::7] = 0.0
        for name in ('se', 'se_x_periodic'):
            ops, pars = square[name]._device_program()
            for ns in (1, ld + 3):
                ts = np.sort(np.random.RandomState(ns).uniform(g.time[0] - 2.0, g.time[-1] + 2.0, ns))
                ts[0] = g.time[3]                                   # (a data time: the delta terms of the posterior form)
                for form in (0, 1):
                    for batched in (0, 1, 2):
                        Ks, kss = ctx.test_fill_rect(ops, pars, 1.25e-12, ts, form=form, batched=batched, s=s if form else None)
                        key = 'rect_%s_%d_ns%d_form%d_batched%d' % (name, N, ns, form, batched)
                        out[key + '_Ks'], out[key + '_kss'] = Ks, kss
        ops, pars = se_per._device_program()
        out['grad_fill_%d' % N] = ctx.eval_kernel_grad(ops, pars)
        for composite in (False, True):
            tag = '%s_%d' % ('sum' if composite else 'se', N)
            B = 5 if N == 45 else 3
            g = model(N, composite)
            x = np.array(g.get_parameters(), dtype=float)
            sets = [x * (1.0 + 0.01 * k) for k in range(B)]
            out['nelbo_batch_' + tag] = np.array(g.nELBO_batch(sets, max_iter=6))
            tstar = np.linspace(g.time[0] - 1.0, g.time[-1] + 1.0, 30)
            tstar[7] = tstar[6]                                     # (a repeated time)
            d = (g.p + 1) * g.q * g.N
            r = np.random.RandomState(2)
            states = (0.1 * r.randn(B, d), 0.5 + r.rand(B, d))
            out['predict_states_mean_' + tag], out['predict_states_var_' + tag] = g.predict_batch(sets, tstar=tstar, states=states)
            healthy()
            for exact in (False, True):
                g = model(N, composite, exact_derivatives=exact)
                start = g._initMuVar(g.nodes, g.weights, g.jitters)
                vals, grads = g.nELBO_and_grad_batch(sets, sweeps=2, start=start)
                out['grad_batch_vals_%s_exact%d' % (tag, exact)], out['grad_batch_grads_%s_exact%d' % (tag, exact)] = np.array(vals), grads
                healthy()
            g = model(N, composite, predict='variational')
            start = g._initMuVar(g.nodes, g.weights, g.jitters)
            out['predict_sweeps_mean_' + tag], out['predict_sweeps_var_' + tag] = g.predict_batch(
                sets, tstar=tstar, from_sweeps=True, sweeps=2, start=start)
            draws, lat = g.sample_posterior_batch(sets, tstar=tstar, n=2, rng=5, separate=True, sweeps=2, start=start)
            out['draws_' + tag], out['draws_latent_' + tag] = draws, lat
            assert g.last_info == 0
            healthy()
    sys.stdout = stdout
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default='fill_bodies_bits.json')
    ap.add_argument('--leg', nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(*a.leg)
        return
    res, failed = {'equal': {}, 'all_equal': False, 'seconds_per_leg': {}}, None
    try:
        with tempfile.TemporaryDirectory() as tmp:
            files = {}
            for name, tree in (('parent', os.path.abspath(a.parent_tree)), ('this', HERE)):
                files[name] = os.path.join(tmp, name + '.npz')
                env = dict(os.environ, GPRN_HIP_LIB=os.path.join(tree, 'gpyrn_amd', 'libgprn_hip.so'))
                began = time.time()
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', tree, files[name]], capture_output=True,
                                   text=True, timeout=300, env=env)
                res['seconds_per_leg'][name] = round(time.time() - began, 1)
                if r.returncode:
                    raise RuntimeError('the leg on %s ended with status %d: %s' % (tree, r.returncode, r.stderr[-1500:]))
            pa, th = np.load(files['parent']), np.load(files['this'])
            assert sorted(pa.files) == sorted(th.files)
            for k in sorted(pa.files):
                res['equal'][k] = bool(np.array_equal(pa[k], th[k], equal_nan=True))
            res['all_equal'] = all(res['equal'].values())
            res['arrays'], res['values_compared'] = len(pa.files), int(sum(pa[k].size for k in pa.files))
            res['finite_values'] = int(sum(np.isfinite(th[k]).sum() for k in th.files))
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    sys.exit(0 if res['all_equal'] and not failed else 1)


if __name__ == '__main__':
    main()
