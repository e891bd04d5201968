"""Timing around the celerite kernels (ids 24 .. 26), on one GPU: profiles/celerite_timing.json.

(a) The gate -- nothing else moved.  Against the parent commit's build of the library (--parent-lib PATH, a libgprn_hip.so made
    from the parent: git worktree + make -C gpyrn_amd/csrc), with the kernels that were there before:
      * bench.py's headline (--gpus 1 --steps 5 --warmup 2: config 3, sweeps/s),
      * nELBO_batch at N = 45 with B = 256 vectors and at N = 497 with B = 32 (p = q = 2, QuasiPeriodic nodes), ms per call.
    Every leg is a FRESH process that takes the three figures once; the legs alternate parent_a, this, parent_b for --rounds
    rounds (default 9) and a figure is the median over the rounds.  The parent runs twice per round: the range of all its
    values, both legs together, is its own run-to-run range in this session.  Passes if this build's median of each figure
    lies inside that range (or on its better side).  The script reports the booleans; it asserts nothing.  Beside each
    batch figure a leg records where the time of one more call goes (`detail`: the wall clock of the library's own call,
    gprn_elbocalc_batch, and the device time of every kernel family from the library's event timers), and the gate repeats
    their medians per build: a figure that moves shows there whether the device or the host moved.
(b) Recorded, not gated (this build alone, one more process):
      * the symmetric fill of SHO, Rotation and CeleriteTerm at N = 4096 beside QuasiPeriodic's in the same run: device time of
        the 'fill' family per matrix (median of nine) and 8 N^2 bytes over it,
      * gprn_grad_elbo for an all-SHO model (p = 3, q = 2) at N = 512 and 4096, option "grad_exact" on against off: device time
        of the 'vec' family, medians of nine.

usage: python profiles/celerite_timing.py --parent-lib PATH [--out FILE] [--rounds R]
The first leg that fails is the last: the JSON then holds what was taken and the error, and nothing more is started."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIGURES = ('bench_sweeps_per_s', 'nelbo_batch_N45_B256_ms', 'nelbo_batch_N497_B32_ms')
HIGHER_IS_BETTER = ('bench_sweeps_per_s',)


def batch_ms(N, B):
    """(ms of the second call, detail of a third: ms inside gprn_elbocalc_batch, device ms per kernel family)"""
    import gpyrn_amd as gpyrn
    from gpyrn_amd import _hip, covfunc, meanfunc, synth
    t, ys, es = synth.rv_series(N, 2)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(2, 2, 'QP'))
    g = gpyrn.inference(2, t, *[a for pair in zip(ys, es) for a in pair])
    g.set_components(nodes, weights, means, jit)
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(3)
    sets = [x0 * (1.0 + 0.01 * rng.standard_normal(x0.size)) for _ in range(B)]
    sys.stdout = open(os.devnull, 'w')                    # (the batch prints its progress line)
    try:
        g.nELBO_batch(sets)
        t0 = time.perf_counter()
        g.nELBO_batch(sets)
        ms = 1e3 * (time.perf_counter() - t0)
        inner, call = [], _hip.Context.elbocalc_batch

        def timed(self, *a, **kw):
            t1 = time.perf_counter()
            res = call(self, *a, **kw)
            inner.append(1e3 * (time.perf_counter() - t1))
            return res
        _hip.Context.elbocalc_batch = timed
        ctx = g._backend()
        ctx.profile_enable(_hip.T_NAMES)
        ctx.profile_read()
        try:
            g.nELBO_batch(sets)
            device = {k: v[0] for k, v in ctx.profile_read().items() if v[1]}
        finally:
            ctx.profile_enable(())
            _hip.Context.elbocalc_batch = call
    finally:
        sys.stdout = sys.__stdout__
    assert g.last_info == 0 and g._backend().option('fallbacks') == 0
    return ms, {'library_call_ms': float(sum(inner)), 'device_ms': device}


def gate_leg():
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5', '--warmup', '2'],
                         stdout=subprocess.PIPE, text=True, check=True, cwd=ROOT, timeout=300)
    out = {'bench_sweeps_per_s': float(json.loads(run.stdout.strip().splitlines()[-1])['value']), 'detail': {}}
    for key, N, B in (('nelbo_batch_N45_B256_ms', 45, 256), ('nelbo_batch_N497_B32_ms', 497, 32)):
        out[key], out['detail'][key] = batch_ms(N, B)
    return out


def recorded_leg():
    import gpyrn_amd as gpyrn
    from gpyrn_amd import _hip, covfunc as c, synth
    out = {'fill_N4096': {}, 'grad_elbo_all_SHO': {}}
    N = 4096
    t = np.sort(np.random.default_rng(1).uniform(0.0, 60.0 * N / 200.0, N))
    ctx = _hip.Context(0)
    ctx.set_data(t, np.zeros((1, N)), np.ones((1, N)), 1)
    ctx.profile_enable(('fill',))
    for name, k in (('QuasiPeriodic', c.QuasiPeriodic(1.1, 30.0, 12.5, 0.6)), ('SHO', c.SHO(1.3, 11.0, 3.0)),
                    ('SHO over-damped', c.SHO(1.3, 11.0, 0.3)), ('Rotation', c.Rotation(1.1, 9.0, 1.2, 0.3, 0.4)),
                    ('CeleriteTerm', c.CeleriteTerm(1.2, 0.3, 0.1, 0.7))):
        ops, pars = k._device_program()
        ctx.eval_kernel(ops, pars, 1e-6)
        ctx.profile_read()
        ms = []
        for _ in range(9):
            ctx.eval_kernel(ops, pars, 1e-6)
            ms.append(ctx.profile_read()['fill'][0])
        med = float(np.median(ms))
        out['fill_N4096'][name] = {'ms': med, 'ms_range': [float(min(ms)), float(max(ms))], 'TB_per_s': 8.0 * N * N / (med * 1e-3) / 1e12}
        print(json.dumps({name: out['fill_N4096'][name]}), flush=True)
    ctx.profile_enable(())
    ctx.close()
    P, Q = 3, 2
    for N in (512, 4096):
        t, ys, es = synth.rv_series(N, P)
        row = {}
        for exact in (0, 1):
            g = gpyrn.inference(Q, t, *[a for pair in zip(ys, es) for a in pair])
            ks = [c.SHO(1.0 + 0.05 * j, 11.0 * (1.0 + 0.05 * j), (0.3, 3.0, 0.7, 5.0)[j % 4]) + c.WhiteNoise(0.1) for j in range(Q + Q * P)]
            g.set_components(ks[:Q], ks[Q:], [None] * P, [0.3] * P)
            nd, wt, mn, jt = g._get_components()
            ctx = g._setup_device(nd, wt, mn, jt)
            ctx.option('grad_exact', exact)
            mu0, var0 = g._initMuVar(nd, wt, jt)
            ctx.set_muvar(np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float))
            _, _, info = ctx.sweep(1, commit=True)
            assert info == 0
            n_k = sum(len(k._device_program()[1]) for k in ks)
            ctx.grad_elbo(n_k)
            ctx.profile_enable(('vec',))
            ctx.profile_read()
            ms = []
            for _ in range(9):
                ctx.grad_elbo(n_k)
                ms.append(ctx.profile_read()['vec'][0])
            ctx.profile_enable(())
            row['exact' if exact else 'differences'] = {'vec_ms': float(np.median(ms)), 'vec_ms_range': [float(min(ms)), float(max(ms))]}
            assert ctx.option('fallbacks') == 0
            g._ctx = None
            ctx.close()
        row['speedup'] = row['differences']['vec_ms'] / row['exact']['vec_ms']
        out['grad_elbo_all_SHO']['N%d' % N] = row
        print(json.dumps({'grad_elbo N%d' % N: row}), flush=True)
    return out


def child(leg, lib=None):
    env = dict(os.environ)
    if lib:
        env['GPRN_HIP_LIB'] = os.path.abspath(lib)
    else:
        env.pop('GPRN_HIP_LIB', None)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', leg], env=env, stdout=subprocess.PIPE, text=True,
                         timeout=600)
    if run.returncode != 0:
        raise RuntimeError('leg %s ended with status %d' % (leg, run.returncode))
    return json.loads(run.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'celerite_timing.json'))
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--leg')
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(gate_leg() if a.leg == 'gate' else recorded_leg()))
        return 0
    result = {'what': __doc__.split('\n\n')[0], 'rounds': a.rounds, 'legs': {'parent_a': [], 'this': [], 'parent_b': []}}
    status = 0
    try:
        if a.parent_lib:
            for r in range(a.rounds):
                for name, lib in (('parent_a', a.parent_lib), ('this', None), ('parent_b', a.parent_lib)):
                    result['legs'][name].append(child('gate', lib))
                    print(r, name, json.dumps(result['legs'][name][-1]), flush=True)
            gate = {}
            for f in FIGURES:
                parent = [x[f] for x in result['legs']['parent_a'] + result['legs']['parent_b']]
                this = float(np.median([x[f] for x in result['legs']['this']]))
                lo, hi = min(parent), max(parent)
                inside = this >= lo if f in HIGHER_IS_BETTER else this <= hi
                gate[f] = {'parent_median': float(np.median(parent)), 'parent_range': [lo, hi],
                           'parent_a_median': float(np.median([x[f] for x in result['legs']['parent_a']])),
                           'parent_b_median': float(np.median([x[f] for x in result['legs']['parent_b']])),
                           'this_median': this, 'this_range': [min(x[f] for x in result['legs']['this']),
                                                               max(x[f] for x in result['legs']['this'])],
                           'inside_the_parents_range_or_better': bool(inside)}
                if f in result['legs']['this'][0].get('detail', {}):
                    for build, legs in (('parent', result['legs']['parent_a'] + result['legs']['parent_b']), ('this', result['legs']['this'])):
                        rows = [x['detail'][f] for x in legs]
                        gate[f][build + '_detail_medians'] = {
                            'library_call_ms': float(np.median([x['library_call_ms'] for x in rows])),
                            'device_ms': {k: float(np.median([x['device_ms'].get(k, 0.0) for x in rows])) for k in rows[0]['device_ms']}}
            result['gate'] = gate
            print(json.dumps(gate, indent=1))
        result['recorded'] = child('recorded')
    except Exception as e:                                 # noqa: BLE001  (what was taken is kept)
        result['error'] = repr(e)
        status = 1
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
