"""A fixed, seeded list of side-by-side calls (ELBO batches on both drivers, with and without gradients, under a mask,
across chunks and through compaction; predict_batch) whose every output goes to one .npz -- and a second mode that compares
two such files field by field with np.array_equal.  For changes that must not move a bit: run it in a checkout of the
parent (twice: what differs between the parent's own runs is noise, not a finding) and in the changed tree, then compare.

usage: python profiles/batch_replay.py --out FILE.npz [--tree CHECKOUT]
       python profiles/batch_replay.py --compare A.npz B.npz [--noise A2.npz]
--tree: the built checkout whose gpyrn_amd is imported (default: the one this file lies in).  --noise: a second run of A's
tree; a field that differs between A and A2 is compared with rtol 1e-8 (the project's bound) instead, and listed."""
import argparse
import os
import sys
from itertools import chain

import numpy as np

MAX_ITER = 200
RTOL_NOISY = 1e-8


def _model(gpyrn, N, p, q, mask=None):
    from gpyrn_amd import covfunc, meanfunc, synth
    t, ys, es = synth.rv_series(N, p, seed=3)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(p, q, 'SE'))
    kw = {}
    if mask is not None:
        ys = [np.where(mask[i], ys[i], np.nan) for i in range(p)]
        es = [np.where(mask[i], es[i], np.inf) for i in range(p)]
        kw = dict(mask=mask, batch_under_mask=True)
    g = gpyrn.inference(q, t, *[a for pair in zip(ys, es) for a in pair], **kw)
    g.set_components(nodes, weights, means, jit)
    return g


def _inputs(g, sets, starts):
    """The arrays Context.elbocalc_batch takes; starts[b]: (mu, var), or None for the vector's own _initMuVar state."""
    ctx = g._backend()
    if g.mask is not None:
        ctx.option('batch_mask', 1)
    y_raw = np.concatenate(g.y)
    kp, yr, jt, m0, v0 = [], [], [], [], []
    for i, x in enumerate(sets):
        g.set_parameters(np.array(x, dtype=float))
        nodes, weights, means, jitters = g._get_components()
        specs = [g._kernel_spec(k) for k in chain(nodes, weights)]
        assert all(sp[0] == 'device' for sp in specs)
        if i == 0:
            for gp, sp in enumerate(specs):
                g._send_spec(ctx, gp, sp)
            g._prior_key = None
        kp.append(np.concatenate([sp[2] for sp in specs]))
        yr.append(y_raw - g._mean(means))
        jt.append(np.asarray(jitters, dtype=float))
        mu, var = starts[i] if starts[i] is not None else g._initMuVar(nodes, weights, jitters)
        m0.append(np.ravel(mu))
        v0.append(np.ravel(var))
    return ctx, np.array(kp), np.array(yr), np.array(jt), np.array(m0), np.array(v0)


FIELDS = ('elbo', 'trips', 'verdicts', 'info', 'mu', 'var', 'grad')


def _store(out, case, res, ctx):
    assert res is not None, case + ': the library has no side-by-side form for this problem'
    for name, a in zip(FIELDS, res):
        out['%s/%s' % (case, name)] = np.asarray(a)
    out[case + '/batch_chunk'] = np.array(ctx.option('batch_chunk'))
    assert ctx.option('fallbacks') == 0, case
    print('%-34s chunk %3d  trips %s' % (case, ctx.option('batch_chunk'), np.asarray(res[1]).tolist()))


def _elbo_cases(out, name, g, B, budget_mb=None, want_chunk=None, seed=5):
    """One problem: a warm state from evaluation 0 alone, then the list -- vector 0 unperturbed from that state, the others
    perturbed more and more from their own cold states, so that the loops end at different trips -- plain, with gradients
    under the stop rule, and forced with gradients.  want_chunk: the smallest whole budget in MB at which batch_chunk reads
    it is searched for (the per-evaluation byte counts are the library's own)."""
    x0 = np.array(g.get_parameters(), dtype=float)
    rng = np.random.RandomState(seed)
    sets = [x0 * (1.0 + (0.3 * b / B) * rng.uniform(-1.0, 1.0, x0.size)) for b in range(B)]
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets[:1], [None])
    warm = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True)
    _store(out, name + '/warm', warm, ctx)
    ctx, kp, yr, jt, m0, v0 = _inputs(g, sets, [(warm[4][0], warm[5][0])] + [None] * (B - 1))
    if want_chunk is not None:
        for budget_mb in range(1, 400):
            ctx.option('batch_mem_mb', budget_mb)
            ctx.elbocalc_batch(kp, yr, jt, m0, v0, 1)
            if ctx.option('batch_chunk') >= want_chunk:
                break
        assert ctx.option('batch_chunk') == want_chunk, (name, ctx.option('batch_chunk'))
        out[name + '/budget_mb'] = np.array(budget_mb)
    elif budget_mb is not None:
        ctx.option('batch_mem_mb', budget_mb)
    plain = ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True)
    _store(out, name + '/plain', plain, ctx)
    _store(out, name + '/grad', ctx.elbocalc_batch(kp, yr, jt, m0, v0, MAX_ITER, want_state=True, want_grad=True), ctx)
    _store(out, name + '/grad_forced',
           ctx.elbocalc_batch(kp, yr, jt, m0, v0, 3, want_state=True, want_grad=True, forced=True), ctx)
    return ctx, kp, jt, plain


def _predict_case(out, name, g, ctx, kp, jt, res, B=3):
    ld = 128 * ((g.N + 127) // 128)
    t = np.asarray(g.time, dtype=float)
    tstar = np.linspace(t[0] - 1.0, t[-1] + 3.0, ld + 5)          # two blocks of prediction times, the second ragged
    d = res[4][0].size
    pred = ctx.predict_batch(kp[:B], res[4][:B].reshape(B, d), res[5][:B].reshape(B, d), tstar, jitters=jt[:B])
    assert pred is not None, name
    for field, a in zip(('lat_mean', 'lat_var', 'out_mean', 'out_var', 'info'), pred):
        out['%s/%s' % (name, field)] = np.asarray(a)
    out[name + '/batch_chunk'] = np.array(ctx.option('batch_chunk'))
    assert ctx.option('fallbacks') == 0, name


def replay(path):
    import gpyrn_amd as gpyrn
    out = {}
    # ---- one tile, N = 45, p = q = 1: one chunk of 20; 40 under a budget that leaves the floor of 16 (16, 16, 8)
    g = _model(gpyrn, 45, 1, 1)
    ctx, kp, jt, res = _elbo_cases(out, 'n45_b20', g, 20)
    _predict_case(out, 'n45_predict', g, ctx, kp, jt, res)
    g = _model(gpyrn, 45, 1, 1)
    _elbo_cases(out, 'n45_b40_chunk16', g, 40, budget_mb=1)
    assert int(out['n45_b40_chunk16/plain/batch_chunk']) == 16
    # ---- one tile under a partial mask, N = 32, p = q = 2
    rng = np.random.RandomState(11)
    mask = rng.uniform(size=(2, 32)) > 0.2
    mask[0, ~mask.any(axis=0)] = True                             # (q >= 2 needs an observed output at every time)
    _elbo_cases(out, 'n32_masked', _model(gpyrn, 32, 2, 2, mask), 6)
    # ---- above one tile, N = 129 (two tiles, the second ragged), p = 2: chunks of 2 and compaction
    for q in (2, 1):
        g = _model(gpyrn, 129, 2, q)
        name = 'n129_q%d' % q
        ctx, kp, jt, res = _elbo_cases(out, name, g, 5, want_chunk=2)
        assert len(set(np.asarray(res[1]).tolist())) > 1, name + ': every loop ended at the same trip, no compaction ran'
        if q == 2:
            _predict_case(out, 'n129_predict', g, ctx, kp, jt, res)
    rng = np.random.RandomState(13)
    mask = rng.uniform(size=(2, 129)) > 0.2
    mask[0, ~mask.any(axis=0)] = True
    ctx, kp, jt, res = _elbo_cases(out, 'n129_q2_masked', _model(gpyrn, 129, 2, 2, mask), 5, want_chunk=2)
    assert len(set(np.asarray(res[1]).tolist())) > 1, 'n129_q2_masked: no compaction ran'
    np.savez(path, **out)
    print('%d fields -> %s' % (len(out), path))


def compare(a_path, b_path, noise_path):
    a, b = np.load(a_path), np.load(b_path)
    noisy = set()
    if noise_path:
        a2 = np.load(noise_path)
        noisy = {k for k in a.files if not np.array_equal(a[k], a2[k], equal_nan=True)}
    assert sorted(a.files) == sorted(b.files), 'the two files hold different fields'
    bad = []
    for k in sorted(a.files):
        if k in noisy:
            ok = a[k].shape == b[k].shape and np.allclose(a[k], b[k], rtol=RTOL_NOISY, atol=0.0, equal_nan=True)
            print('noisy between two runs of the first tree, compared with rtol %g: %s %s' % (RTOL_NOISY, k, 'ok' if ok else 'DIFFERS'))
        else:
            ok = np.array_equal(a[k], b[k], equal_nan=True)
        if not ok:
            bad.append(k)
    print('%d fields, %d bit for bit, %d noisy, %d differ%s' % (len(a.files), len(a.files) - len(noisy) - len([k for k in bad if k not in noisy]),
                                                               len(noisy), len(bad), ': ' + ', '.join(bad) if bad else ''))
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--noise')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.noise))
    sys.path.insert(0, os.path.abspath(args.tree))
    replay(args.out)
