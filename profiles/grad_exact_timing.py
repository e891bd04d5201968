"""Times gprn_grad_elbo with the exact parameter derivatives (option "grad_exact", csrc/dk_eval.h) against the
Richardson-extrapolated differences of the kernel program, on one GPU: three models whose kernels all take the generic path
-- all Matern52, all RQP, all QuasiPeriodic + WhiteNoise -- at N = 512 and N = 4096 (p = 3, q = 2: eight latent GPs), the
option off and on, and the same call on the parent commit's build of the library.  Per leg: one committed sweep, a warm-up,
then the median of REPS calls of gprn_grad_elbo -- the wall clock of the call, and the device time of its 'vec' family
(the library's event timers: the prelude's small kernels, which are the same in every leg, plus the contraction and
k_grad_final), so that the difference between two legs is the difference of their contraction kernels.

    python profiles/grad_exact_timing.py [out.json] [--parent-lib PATH]      (default: profiles/grad_exact_timing.json)
    python profiles/grad_exact_timing.py --resource-report                   (no GPU: compiles grad.hip and fill.hip with the
                                                                              compiler's resource remarks and writes the new
                                                                              kernels' figures to profiles/grad_exact_isa_resources.txt)

--parent-lib: libgprn_hip.so built from the parent commit (git worktree + make -C gpyrn_amd/csrc); it is loaded by a child
process of its own (GPRN_HIP_LIB), started before this one touches the GPU.  The only timing condition of the feature: on
none of the six cases is the exact leg's 'vec' time above the parent's.
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RESOURCES = os.path.join(ROOT, 'profiles', 'grad_exact_isa_resources.txt')
REPS = 9
P, Q = 3, 2
SIZES = (512, 4096)
MODELS = ('Matern52', 'RQP', 'QuasiPeriodic+WhiteNoise')
NEW_KERNELS = ('k_grad_contract_bILi2E', 'k_grad_contract_bILi1E', 'k_grad_exact_rows', 'k_fill_grad')


def kernel_of(model, c, j):
    """Latent GP j's kernel: the parameters vary a little from one latent GP to the next."""
    f = 1.0 + 0.05 * j
    if model == 'Matern52':
        return c.Matern52(1.0 * f, 8.0 * f)
    if model == 'RQP':
        return c.RQP(1.0 * f, 1.5, 20.0 * f, 11.0 * f, 0.8)
    return c.QuasiPeriodic(1.0 * f, 20.0 * f, 11.0 * f, 0.8) + c.WhiteNoise(0.1)


def one_case(model, N, exact):
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, synth
    t, ys, es = synth.rv_series(N, P)
    g = gpyrn.inference(Q, t, *[a for pair in zip(ys, es) for a in pair])
    nodes = [kernel_of(model, covfunc, j) for j in range(Q)]
    weights = [kernel_of(model, covfunc, Q + j) for j in range(Q * P)]
    g.set_components(nodes, weights, [None] * P, [0.3] * P)
    nd, wt, mn, jt = g._get_components()
    ctx = g._setup_device(nd, wt, mn, jt)
    if exact is not None:                                       # (the parent's build does not know the option)
        ctx.option('grad_exact', int(exact))
    mu0, var0 = g._initMuVar(nd, wt, jt)
    ctx.set_muvar(np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float))
    _, _, info = ctx.sweep(1, commit=True)
    assert info == 0
    n_k = sum(len(k._device_program()[1]) for k in list(nd) + list(wt))
    grad = ctx.grad_elbo(n_k)                                   # warm-up
    ctx.profile_enable(('vec',))
    ctx.profile_read()
    wall, vec = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        ctx.grad_elbo(n_k)
        wall.append(1e3 * (time.perf_counter() - t0))
        vec.append(ctx.profile_read()['vec'][0])
    ctx.profile_enable(())
    out = dict(model=model, N=N, n_params=n_k, call_ms=float(np.median(wall)), vec_ms=float(np.median(vec)),
               vec_ms_spread=[float(min(vec)), float(max(vec))], fallbacks=int(ctx.option('fallbacks')))
    g._ctx = None
    ctx.close()
    return out, grad


def leg(exact):
    rows = []
    for model in MODELS:
        for N in SIZES:
            r, grad = one_case(model, N, exact)
            r['grad_checksum'] = float(np.abs(grad).sum())
            rows.append(r)
            print(json.dumps(dict(leg='parent' if exact is None else ('exact' if exact else 'differences'), **r)), flush=True)
    return rows


def parent_leg(lib):
    """The same cases on another build of the library, in a child process of its own."""
    env = dict(os.environ, GPRN_HIP_LIB=os.path.abspath(lib))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg-parent'], env=env, stdout=subprocess.PIPE, text=True,
                         check=True)
    return json.loads(run.stdout.strip().splitlines()[-1])


def resource_report():
    """The compiler's resource remarks for the kernels this feature adds (and the difference instantiation beside them)."""
    csrc = os.path.join(ROOT, 'gpyrn_amd', 'csrc')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in ('grad.hip', 'fill.hip'):
            run = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I/opt/rocm/include',
                                  '-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(csrc, src), '-o',
                                  os.path.join(tmp, src + '.o')], stderr=subprocess.PIPE, text=True, check=True)
            keep = False
            for ln in run.stderr.splitlines():
                if 'Function Name:' in ln:
                    keep = any(k in ln for k in NEW_KERNELS)
                if keep and 'remark:' in ln:
                    lines.append(re.sub(r'\s*\[-Rpass-analysis=kernel-resource-usage\]', '', ln.split('remark:', 1)[1]).rstrip())
    with open(RESOURCES, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def read_resources():
    """{kernel: {VGPRs, ScratchSize, Occupancy, LDS}} from the saved report, or None."""
    if not os.path.exists(RESOURCES):
        return None
    out, cur = {}, None
    for ln in open(RESOURCES):
        m = re.search(r'Function Name: (\S+)', ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r'\s*(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|VGPRs Spill): (\d+)', ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


if __name__ == '__main__':
    args = sys.argv[1:]
    if '--resource-report' in args:
        resource_report()
        sys.exit(0)
    if '--leg-parent' in args:
        from gpyrn_amd import _hip
        _hip.SIGNATURES.pop('gprn_eval_kernel_grad', None)      # (the entry point this feature adds)
        known = _hip.Context.option
        # (... and the option: the set-up forwards it, the parent's library does not know it)
        _hip.Context.option = lambda self, name, value=-1: 0 if name == 'grad_exact' else known(self, name, value)
        print(json.dumps(leg(None)))
        sys.exit(0)
    parent_lib = args[args.index('--parent-lib') + 1] if '--parent-lib' in args else None
    paths = [a for i, a in enumerate(args) if not a.startswith('--') and (i == 0 or args[i - 1] != '--parent-lib')]
    path = paths[0] if paths else os.path.join(ROOT, 'profiles', 'grad_exact_timing.json')
    parent = parent_leg(parent_lib) if parent_lib else None     # (before this process opens the GPU)
    off, on = leg(False), leg(True)
    cases = []
    for i, (a, b) in enumerate(zip(off, on)):
        c = dict(model=a['model'], N=a['N'], n_params=a['n_params'], differences=a, exact=b,
                 vec_speedup_over_differences=a['vec_ms'] / b['vec_ms'],
                 gradients_differ_by=abs(a['grad_checksum'] - b['grad_checksum']) / a['grad_checksum'])
        if parent:
            c['parent'] = parent[i]
            c['exact_not_slower_than_parent'] = bool(b['vec_ms'] <= parent[i]['vec_ms'])
        cases.append(c)
    with open(path, 'w') as f:
        json.dump({'what': "gprn_grad_elbo, option 'grad_exact' off / on (and the parent commit's build): p = %d, q = %d, "
                           "medians of %d calls after one committed sweep; vec_ms = the device time of the call's 'vec' "
                           "family (prelude kernels + contraction + k_grad_final)" % (P, Q, REPS),
                   'cases': cases, 'resources': read_resources()}, f, indent=1)
        f.write('\n')
    if parent:
        print('exact not slower than the parent on every case:', all(c['exact_not_slower_than_parent'] for c in cases))
