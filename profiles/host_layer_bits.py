"""Bits of the public side-by-side ("batch") methods under this tree's Python layer against the parent commit's, on the GPU,
after the copies in gpyrn_amd/meanfield.py and gpyrn_amd/_hip.py were folded onto shared helpers.  The library did not change
and both layers load the same one (this tree's, through GPRN_HIP_LIB); the refactor hands it the same bytes in the same order,
so every returned array and the state the object keeps must be equal byte for byte, NaN rows of a failed evaluation included.
A difference is a bug in the refactor.

Two FRESH child processes (--leg FILE), each under its own ``timeout``, one after the other; the second starts only if the
first ended with status 0.  The first has PYTHONPATH at --parent-tree (a checkout of the parent commit: its Python package is
all that is read), the second at this tree.  The parent process compares and exits with status 1 on any difference or error.

Shapes (profiles/batch_tail_bits.py's): one tile N = 45, p = q = 2, B = 5; two tiles N = 200, p = q = 2, B = 3; t*: ld + 3
times.  Per shape: plain and masked (``batch_under_mask=True``, a fifth of each output unobserved) x the reference and the bound
form of the ELBO x Linear means with ``device_means`` / Linear means on the host / constant means.  Calls: ``nELBO_batch``;
``nELBO_and_grad_batch`` forced with three sweeps and under the stop rule; ``heldout_batch`` and ``cross_validate``; with
``predict='variational'`` ``predict_batch(from_sweeps=True)``, ``sample_posterior_batch`` and ``posterior_predictive(draws=2)``;
with ``predict='reference'`` ``predict_batch`` with and without ``states``.  Once more at one tile with a NaN jitter in the
middle vector (a numerical verdict: that vector's rows are NaN), and once with ``batch_max_N = 0``, so that the one-by-one
driver runs on the device.

usage: python profiles/host_layer_bits.py --parent-tree DIR [--out FILE]"""
import argparse
import itertools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {'one_tile': (45, 2, 2, 5), 'two_tiles': (200, 2, 2, 3)}
LEG_SECONDS = 420


def _model(N, p, q, masked, means, **kw):
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc, synth
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, _, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, 'SE'))
    if means == 'constant':
        mean_list = [meanfunc.Constant(0.1 * (i + 1)) for i in range(p)]
    else:
        mean_list = [meanfunc.Linear(0.01 * (i + 1), 0.1 * (i + 1)) for i in range(p)]
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
    g = gpyrn.inference(q, t, *[a for i in range(p) for a in (y[i], e[i])], mask=mask, batch_under_mask=True,
                        device_means=means == 'linear_device', **kw)
    g.set_components(nodes, weights, mean_list, jit)
    return g


def _flat(value):
    """The arrays of a return value, in order."""
    if isinstance(value, tuple) and hasattr(value, '_fields'):
        value = tuple(value)
    if isinstance(value, (tuple, list)) and any(isinstance(v, (np.ndarray, list, tuple)) for v in value):
        return [a for v in value for a in _flat(v)]
    return [np.asarray(value)]


def leg(path):
    out, refused = {}, []
    sys.stdout = open(os.devnull, 'w')

    def keep(key, g, call):
        try:
            value = call()
        except (ValueError, NotImplementedError, np.linalg.LinAlgError) as exc:      # (a refusal: its text is compared)
            value = np.frombuffer(('%s: %s' % (type(exc).__name__, exc)).encode(), dtype=np.uint8)
            refused.append(key)
        state = [np.zeros(0) if a is None else np.asarray(a) for a in (g._mu, g._var, getattr(g, 'last_nuggets', None))]
        after = state + [np.asarray(0 if g.last_info is None else g.last_info), np.array(g.get_parameters(), dtype=float)]
        for i, a in enumerate(_flat(value) + after):
            out['%s#%d' % (key, i)] = a

    def drive(key, N, p, q, B, masked, form, means, failed=False, one_by_one=False):
        ld = -(-N // 128) * 128

        def fresh(predict):
            g = _model(N, p, q, masked, means, elbo=form, predict=predict)
            if one_by_one:
                g.batch_max_N = 0
            x0 = np.array(g.get_parameters(), dtype=float)
            sets = [x0 * (1.0 + 0.01 * k) for k in range(B)]
            if failed:
                sets[B // 2][-1] = np.nan
            t = np.asarray(g.time, dtype=float)
            return g, sets, np.linspace(t[0] - 1.0, t[-1] + 1.0, ld + 3), g._initMuVar(g.nodes, g.weights, g.jitters)

        g, sets, ts, start = fresh('variational')
        forced = dict(sweeps=3, start=start)
        if not failed:
            keep(key + '/nELBO_batch', g, lambda: g.nELBO_batch(sets, max_iter=20))
            keep(key + '/grad_loop', g, lambda: g.nELBO_and_grad_batch(sets, max_iter=20))
        keep(key + '/grad_forced', g, lambda: g.nELBO_and_grad_batch(sets, **forced))
        if form == 'reference':
            keep(key + '/varpred_forced', g, lambda: g.predict_batch(sets, tstar=ts, from_sweeps=True, separate=True, **forced))
            keep(key + '/draws_forced', g, lambda: g.sample_posterior_batch(sets, tstar=ts, n=2, noise=True, separate=True, rng=5,
                                                                            **forced))
            if not failed:
                keep(key + '/varpred_loop', g, lambda: g.predict_batch(sets, tstar=ts, from_sweeps=True, max_iter=20))
                keep(key + '/mixture_draws', g, lambda: g.posterior_predictive(sets, tstar=ts, draws=2, rng=3, **forced))
        if failed or one_by_one:
            return
        folds = g.cv_folds(2, rng=0)
        keep(key + '/heldout', g, lambda: g.heldout_batch(sets, np.tile(folds, (B, 1, 1))[:B], sweeps=3))
        keep(key + '/cross_validate', g, lambda: g.cross_validate(folds, sets[:2], max_iter=20))
        if form == 'reference':
            g, sets, ts, start = fresh('reference')
            rng = np.random.default_rng(11)
            shape = (B, p + 1, q, N)
            mu0, var0 = (np.tile(np.ravel(a), (B, 1)).reshape(shape) for a in start)
            states = (mu0 + 0.01 * rng.standard_normal(shape), var0)
            keep(key + '/predict_states', g, lambda: g.predict_batch(sets, tstar=ts, states=states, separate=True))
            keep(key + '/predict_loop', g, lambda: g.predict_batch(sets, tstar=ts, max_iter=20))

    for shape, (N, p, q, B) in SHAPES.items():
        for masked, form, means in itertools.product((False, True), ('reference', 'bound'),
                                                     ('linear_device', 'linear_host', 'constant')):
            drive('%s/%s/%s/%s' % (shape, 'masked' if masked else 'plain', form, means), N, p, q, B, masked, form, means)
    N, p, q, B = SHAPES['one_tile']
    drive('one_tile/plain/reference/linear_device/failed', N, p, q, B, False, 'reference', 'linear_device', failed=True)
    for form in ('reference', 'bound'):
        drive('one_tile/plain/%s/linear_host/one_by_one' % form, N, p, q, B, False, form, 'linear_host', one_by_one=True)
    out['__refused__'] = np.frombuffer(json.dumps(refused).encode(), dtype=np.uint8)
    np.savez(path, **out)


def _child(tree, path):
    env = dict(os.environ, PYTHONPATH=tree, GPRN_HIP_LIB=os.path.join(HERE, 'gpyrn_amd', 'libgprn_hip.so'))
    r = subprocess.run(['timeout', '-k', '10', str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), '--leg', path],
                       capture_output=True, text=True, env=env)
    if r.returncode:
        raise RuntimeError('the leg on %s ended with status %d: %s' % (tree, r.returncode, r.stderr[-1500:]))


def condense(res):
    """The file's form: per setting the calls whose arrays were all equal, and the calls that differed by name."""
    equal = res.pop('equal')
    res['cases'], res['differing'], res['equal_calls'] = len(equal), sorted(k for k, v in equal.items() if not v), {}
    for case in sorted(k for k, v in equal.items() if v):
        setting, _, call = case.rpartition('/')
        res['equal_calls'][setting] = (res['equal_calls'].get(setting, '') + ' ' + call).strip()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default='host_layer_bits.json')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg)
    res = {'shapes': {k: dict(N=v[0], p=v[1], q=v[2], B=v[3]) for k, v in SHAPES.items()}, 'equal': {}, 'all_equal': False}
    failed = None
    try:
        parent = os.path.abspath(a.parent_tree)
        assert os.path.exists(os.path.join(parent, 'gpyrn_amd', 'meanfield.py')), parent
        with tempfile.TemporaryDirectory() as tmp:
            files = {}
            for name, tree in (('parent', parent), ('this', HERE)):            # (a leg that fails stops the next)
                files[name] = os.path.join(tmp, name + '.npz')
                _child(tree, files[name])
            pa, th = np.load(files['parent']), np.load(files['this'])
            assert sorted(pa.files) == sorted(th.files)
            for k in sorted(pa.files):
                a_, b_ = pa[k], th[k]
                same = bool(a_.dtype == b_.dtype and a_.shape == b_.shape and a_.tobytes() == b_.tobytes())
                case = k.rsplit('#', 1)[0]
                res['equal'][case] = res['equal'].get(case, True) and same
            res['refused'] = json.loads(th['__refused__'].tobytes().decode())
            res['all_equal'] = all(res['equal'].values())
            res['arrays'], res['values_compared'] = len(pa.files), int(sum(pa[k].size for k in pa.files))
            res['nan_values'] = int(sum(np.isnan(th[k]).sum() for k in th.files if th[k].dtype.kind == 'f'))
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    res = condense(res)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'equal_calls'}), flush=True)
    sys.exit(0 if res['all_equal'] and not failed else 1)


if __name__ == '__main__':
    main()
