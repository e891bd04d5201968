"""Device memory that the entry points with per-call temporaries leave behind: free device memory (hipMemGetInfo of the
HIP runtime itself, through ctypes -- not through the library under test) before and after `--reps` repetitions of each
call on ONE context, after one warm-up call of that entry point (the warm-up sizes what the context keeps: the
prediction buffers, the diagnostics' scratch problem).  drift_bytes = free before - free after: what the repetitions cost.

usage: python profiles/api_scratch_memory.py [--out FILE] [--reps R]
The library is the one gpyrn_amd loads (GPRN_HIP_LIB names another build, e.g. the parent commit's)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpyrn_amd as gpyrn  # noqa: E402
from gpyrn_amd import _hip, covfunc, meanfunc, synth  # noqa: E402

_hip.load_library()                                            # (so that the runtime below is the one the library uses)
_rt = ctypes.CDLL(next((line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line), 'libamdhip64.so'))
_rt.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
_rt.hipDeviceSynchronize.argtypes = []


def free_bytes():
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert _rt.hipDeviceSynchronize() == 0
    assert _rt.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='api_scratch_memory.json')
    ap.add_argument('--reps', type=int, default=40)
    a = ap.parse_args()
    N, p, q, kind, ns, nd = 512, 3, 2, 'QP', 384, 8
    t, ys, es = synth.rv_series(N, p)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, kind))
    g = gpyrn.inference(q, t, *[x for pair in zip(ys, es) for x in pair])
    g.set_components(nodes, weights, means, jit)
    nd_, wt, mn, jt = g._get_components()
    ctx = g._setup_device(nd_, wt, mn, jt)
    mu0, var0 = g._initMuVar(nd_, wt, jt)
    ctx.set_muvar(np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float))
    ctx.keep_sigma(True)
    _, _, info = ctx.sweep(1, commit=True)
    assert info == 0
    mu, _ = ctx.get_muvar()
    rng = np.random.default_rng(0)
    span = np.ptp(t)
    ts = np.linspace(t.min() - 0.2 * span, t.max() + 0.2 * span, ns)
    z = rng.standard_normal((ctx.G, nd, ns))
    ops, pars = nd_[0]._device_program()
    zp = rng.standard_normal((4, N))
    S = np.eye(N)
    A, B, C = rng.standard_normal((256, 384)), rng.standard_normal((384, 128)), rng.standard_normal((256, 128))
    M = rng.standard_normal((2, 256, 256))
    spd = M @ M.transpose(0, 2, 1) + 256 * np.eye(256)
    calls = (('predict', lambda: ctx.predict(ts)),
             ('predict_cov', lambda: ctx.predict_cov(ts)),
             ('predict_draws', lambda: ctx.predict_draws(ts, z)),
             ('sample_prior', lambda: ctx.sample_prior(ops, pars, 1e-6, zp)),
             ('grad_matrices', lambda: ctx.grad_matrices(0)),
             ('prior_terms', lambda: ctx.prior_terms(0, S, mu[0, 0])),
             ('test_gemm', lambda: ctx.test_gemm(A, B, C, 0, 1, 1)),
             ('test_factor_invert', lambda: ctx.test_factor_invert(spd)))
    rec = {'library': _hip.LIB_PATH, 'shape': {'N': N, 'p': p, 'q': q, 'ns': ns, 'draws': nd}, 'reps': a.reps, 'calls': {}}
    for name, call in calls:
        call()                                                 # warm-up: what the context keeps is allocated here
        before = free_bytes()
        for _ in range(a.reps):
            call()
        after = free_bytes()
        rec['calls'][name] = {'free_before': before, 'free_after': after, 'drift_bytes': before - after}
        print(name, rec['calls'][name], flush=True)
    rec['fallbacks'] = ctx.option('fallbacks')
    os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
