"""Bits and device memory of this build against the parent commit's build, after everything that runs behind a chunk's loop of
the side-by-side batches moved into one tail (csrc/batch_tail.hip) that reads one description of what the loop left.  Kernels,
launch order and summation orders did not change, so every output array must be the parent's bit for bit; a difference means a
pass was handed another buffer, another state copy or another order.

Each build runs in a FRESH child process (--leg FILE) of THIS tree's Python package; the parent's is its library alone, named
through GPRN_HIP_LIB (--parent-tree DIR: a built checkout of the parent commit).  The parent process compares the arrays byte
for byte (NaN rows of a failed evaluation included) and exits with status 1 on any difference or error.

Shapes: one tile N = 45, p = q = 2, B = 5 (ld = 128); two tiles N = 200, p = q = 2, B = 3 (ld = 256, T = 2).  t*: ld + 3 times, so
a second, ragged block of t* runs.  Calls, through Context: gprn_elbocalc_batch_grad forced with three sweeps and under the stop
rule, in the reference and the bound form; gprn_elbocalc_batch_means with resid_out and mean_grad_out in the bound form;
gprn_elbocalc_batch_predict with both pairs; gprn_elbocalc_batch_draws with n_draws = 2.  Each of them in four settings:

* plain;
* chunks: "batch_mem_mb" so small that the list runs in at least two chunks and the passes' scratch gets nothing of the budget
  (groups of one evaluation).  Above one tile 1.5 evaluations' slabs: chunks of one.  On one tile a chunk never holds fewer than
  16 evaluations, so this setting alone runs B = 21 there (16 + 5); "batch_chunk" is read back and recorded.  The draws once more
  with all evaluations' slabs and 1.5 evaluations' draw scratch in the budget: one chunk, the pass in groups inside it;
* failed: a NaN jitter in the middle vector, so that no pivot of its B is positive (a numerical verdict, as in
  tests/test_draw_batch_gpu.py::test_a_failed_pivot_in_the_middle_of_a_batch);
* masked: a fifth of each output's points unobserved, under "batch_mask" = 1.

--memory: free device memory (hipMemGetInfo of the runtime the library uses) before and after 40 repetitions each of the
predict call and the draws call, after one warm-up call, at both shapes on both builds: the drift and the warm footprint (free
before the context is made less free after the repetitions).

usage: python profiles/batch_tail_bits.py --parent-tree DIR [--out FILE] [--memory]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {'one_tile': (45, 2, 2, 5), 'two_tiles': (200, 2, 2, 3)}
SETTINGS = ('plain', 'chunks', 'failed', 'masked')


def _model(N, p, q, form, masked):
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc, synth
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, _, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, 'SE'))
    means = [meanfunc.Linear(0.01 * (i + 1), 0.1 * (i + 1)) for i in range(p)]
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
    g = gpyrn.inference(q, t, *[a for i in range(p) for a in (y[i], e[i])], mask=mask, batch_under_mask=True, elbo=form,
                        device_means=True, predict='variational')
    g.set_components(nodes, weights, means, jit)
    return g


def _slab_bytes(N, p, q, form):
    """what one evaluation takes in a chunk above one tile (csrc/midn.hip mid_bytes_per_eval, restated, no mask)"""
    G, ld = q * (p + 1), -(-N // 128) * 128
    T, d, n_q1 = ld // 128, (p + 1) * q * N, (q - 1 if form == 'reference' else 0)
    return 8 * ((4 * G + n_q1) * ld * ld + G * ld * (7 + 2 * T + 2) + n_q1 * q // 2 * ld + 2 * d + 2 * p * N + 64)


def _draw_bytes(N, p, q, ns, nd):
    """the draw pass's scratch for one evaluation (csrc/batch_layout.h draw_scratch, restated without its paddings)"""
    G, ld = q * (p + 1), -(-N // 128) * 128
    ns_pad, nd_pad, nblk = -(-ns // 128) * 128, -(-nd // 128) * 128, -(-ns // ld)
    return 8 * (G * (ns_pad * ld + 3 * ns_pad * ns_pad + 2 * nd_pad * ns_pad + 3 * ns_pad) + p * nd * ns + ns + (nblk * 4 + 3) * G)


def _staged(g, B, failed):
    x0 = np.array(g.get_parameters(), dtype=float)
    sets = [x0 * (1.0 + 0.01 * k) for k in range(B)]
    if failed:
        sets[B // 2][-1] = np.nan
    start = g._initMuVar(g.nodes, g.weights, g.jitters)
    ctx, kp, yr, jt, m0, v0 = g._batch_stage(sets, start=start)
    from gpyrn_amd import _hip
    assert isinstance(yr, _hip.MeanParams)
    return ctx, kp, yr, jt, m0, v0


def _times(g, N):
    ld = -(-N // 128) * 128
    t = np.asarray(g.time, dtype=float)
    return np.linspace(t[0] - 1.0, t[-1] + 1.0, ld + 3)


def leg(path):
    sys.path.insert(0, HERE)
    from gpyrn_amd import _hip
    out, chunks = {}, {}
    sys.stdout = open(os.devnull, 'w')
    for shape, (N, p, q, B0) in SHAPES.items():
        for setting in SETTINGS:
            B = 21 if (setting == 'chunks' and shape == 'one_tile') else B0
            for form in ('reference', 'bound'):
                key = '%s_%s_%s' % (shape, setting, form)
                g = _model(N, p, q, form, setting == 'masked')
                ctx, kp, yr, jt, m0, v0 = _staged(g, B, setting == 'failed')
                resid = yr.host_resid(ctx)
                ts = _times(g, N)
                G = q * (p + 1)
                z = np.random.default_rng(5).standard_normal((B, G, 2, ts.size))
                if setting == 'chunks':
                    ctx.option('batch_mem_mb', 1 if shape == 'one_tile' else int(1.5 * _slab_bytes(N, p, q, form) / 2 ** 20))

                def keep(name, res, extra=()):
                    # (info: the middle vector of the 'failed' setting must have failed, and nobody else)
                    assert [int(v > 0) for v in res[3]] == [int(setting == 'failed' and b == B // 2) for b in range(B)], (key, name, res[3])
                    for i, a in enumerate(tuple(res) + tuple(extra)):
                        if a is not None:
                            out['%s_%s_%d' % (key, name, i)] = np.asarray(a)
                    chunks['%s_%s' % (key, name)] = int(ctx.option('batch_chunk'))

                keep('grad_forced', ctx.elbocalc_batch(kp, resid, jt, m0, v0, 3, want_state=True, want_grad=True, forced=True))
                keep('grad_loop', ctx.elbocalc_batch(kp, resid, jt, m0, v0, 100, want_state=True, want_grad=True))
                if form == 'bound':
                    yr.want_mean_grad = True
                    res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, 3, want_state=True, want_grad=True, forced=True)
                    assert yr.mean_grad is not None
                    keep('means', res, (yr.resid, yr.mean_grad))
                    continue
                keep('predict', ctx.elbocalc_batch_predict(kp, resid, jt, m0, v0, 3, ts, forced=True))
                keep('draws', ctx.elbocalc_batch_draws(kp, resid, jt, m0, v0, 3, ts, z, forced=True))
                if setting == 'chunks':
                    ctx.option('batch_mem_mb', 1 if shape == 'one_tile' else
                               int(np.ceil((B * _slab_bytes(N, p, q, form) + 1.5 * _draw_bytes(N, p, q, ts.size, 2)) / 2 ** 20)))
                    keep('draws_groups', ctx.elbocalc_batch_draws(kp, resid, jt, m0, v0, 3, ts, z, forced=True))
                assert ctx.option('fallbacks') == 0
    out['__chunks__'] = np.frombuffer(json.dumps(chunks).encode(), dtype=np.uint8)
    np.savez(path, **out)


def memory_leg(path):
    sys.path.insert(0, HERE)
    from gpyrn_amd import _hip
    _hip.load_library()
    rt = ctypes.CDLL(next((ln.split()[-1] for ln in open('/proc/self/maps') if 'libamdhip64' in ln), 'libamdhip64.so'))
    rt.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]

    def free_bytes():
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert rt.hipDeviceSynchronize() == 0 and rt.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    keep_out, sys.stdout = sys.stdout, open(os.devnull, 'w')
    rec = {'library': "the parent tree's (GPRN_HIP_LIB)" if os.environ.get('GPRN_HIP_LIB') else "this tree's", 'reps': 40, 'calls': {}}
    for shape, (N, p, q, B) in SHAPES.items():
        for name in ('predict', 'draws'):
            g = _model(N, p, q, 'reference', False)
            g._backend()
            cold = free_bytes()                                # (the context exists; no batch has run on it)
            ctx, kp, yr, jt, m0, v0 = _staged(g, B, False)
            resid, ts = yr.host_resid(ctx), _times(g, N)
            z = np.random.default_rng(5).standard_normal((B, q * (p + 1), 2, ts.size))
            call = ((lambda: ctx.elbocalc_batch_predict(kp, resid, jt, m0, v0, 3, ts, forced=True)) if name == 'predict' else
                    (lambda: ctx.elbocalc_batch_draws(kp, resid, jt, m0, v0, 3, ts, z, forced=True)))
            call()                                             # warm-up: what the batch keeps is allocated here
            before = free_bytes()
            for _ in range(rec['reps']):
                call()
            after = free_bytes()
            rec['calls']['%s_%s' % (shape, name)] = {'free_before': before, 'free_after': after, 'drift_bytes': before - after,
                                                     'warm_footprint_bytes': cold - after}
            ctx.close()
            g._ctx = None
    sys.stdout = keep_out
    with open(path, 'w') as f:
        json.dump(rec, f)


def _child(flag, path, lib):
    env = dict(os.environ)
    env.pop('GPRN_HIP_LIB', None)
    if lib:
        env['GPRN_HIP_LIB'] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), flag, path], capture_output=True, text=True, timeout=500, env=env)
    if r.returncode:
        raise RuntimeError('the leg on %s ended with status %d: %s' % (lib or 'this build', r.returncode, r.stderr[-800:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default='batch_tail_bits.json')
    ap.add_argument('--memory', action='store_true')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--memory-leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg)
    if a.memory_leg:
        return memory_leg(a.memory_leg)
    res, failed = {'shapes': {k: dict(N=v[0], p=v[1], q=v[2], B=v[3]) for k, v in SHAPES.items()}, 'equal': {}, 'all_equal': False}, None
    try:
        parent_lib = os.path.join(os.path.abspath(a.parent_tree), 'gpyrn_amd', 'libgprn_hip.so')
        assert os.path.exists(parent_lib), parent_lib
        with tempfile.TemporaryDirectory() as tmp:
            files = {}
            for name, lib in (('parent', parent_lib), ('this', None)):
                files[name] = os.path.join(tmp, name + '.npz')
                _child('--leg', files[name], lib)
            pa, th = np.load(files['parent']), np.load(files['this'])
            assert sorted(pa.files) == sorted(th.files)
            for k in sorted(pa.files):
                a_, b_ = pa[k], th[k]
                res['equal'][k] = bool(a_.dtype == b_.dtype and a_.shape == b_.shape and a_.tobytes() == b_.tobytes())
            res['batch_chunk'] = json.loads(th['__chunks__'].tobytes().decode())
            res['all_equal'] = all(res['equal'].values())
            res['arrays'], res['values_compared'] = len(pa.files) - 1, int(sum(pa[k].size for k in pa.files if k != '__chunks__'))
            res['nan_values'] = int(sum(np.isnan(th[k]).sum() for k in th.files if th[k].dtype.kind == 'f'))
            if a.memory:
                res['memory'] = {}
                for name, lib in (('parent', parent_lib), ('this', None)):
                    path = os.path.join(tmp, name + '.json')
                    _child('--memory-leg', path, lib)
                    res['memory'][name] = json.load(open(path))
                res['memory']['zero_drift'] = all(c['drift_bytes'] == 0 for m in ('parent', 'this')
                                                  for c in res['memory'][m]['calls'].values())
                res['memory']['warm_footprint_this_minus_parent'] = {
                    k: res['memory']['this']['calls'][k]['warm_footprint_bytes'] - res['memory']['parent']['calls'][k]['warm_footprint_bytes']
                    for k in res['memory']['this']['calls']}
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != 'equal'}), flush=True)
    print('differing arrays:', [k for k, v in res['equal'].items() if not v], flush=True)
    sys.exit(0 if res['all_equal'] and not failed and (not a.memory or res['memory']['zero_drift']) else 1)


if __name__ == '__main__':
    main()
