"""The problems and NumPy restatements behind tests/test_small_variants_gpu.py: every instantiation of the one-tile kernels
(csrc/smalln.hip: k_small_phase, k_small_tail, k_small_prior and their `_b` forms; csrc/order.hip: k_order_small, `_b`) under
the eight combinations of (data mask, sweep order, ELBO form).

The model: synth.rv_series(N, 2) under synth.component_spec(2, 2) -- p = 2, q = 2 -- at N = 40 (one tile, nph = 3 with a ragged
last 16-column phase) and at N = 150 (two tiles: option "small_path" = 2, single-problem kernels only).  q = 2: the reference's
order diverges at q = 3 and three sweeps would lose the digits.  Masks: _mask_ref.partial_mask(2, N, MASK_SEED).  Three
parameter vectors, the model's own and every parameter scaled by 1.07 and by 0.93, so that a batch's slots differ in every
kernel parameter, mean and jitter.  Each vector's restatement is composed by tests/_schedule_cases.compose_sweep, computed once
per process and left read-only; every evaluation starts from _initMuVar at the FIRST vector's parameters (a batch shares its
starting state).
"""
import functools
import itertools

import numpy as np

from oracle import cpu_ref
from tests import _mask_ref, _schedule_cases as S

P, Q = 2, 2
N_ONE, N_TWO = 40, 150
N_SWEEPS = 3
MAX_ITER = 60
MASK_SEED = 7
SCALES = (1.0, 1.07, 0.93)
# (data mask?, sweep order, ELBO form)
COMBOS = tuple(itertools.product((False, True), ('reference', 'sequential'), ('reference', 'bound')))


def combo_id(combo):
    return '%s-%s-%s' % ('mask' if combo[0] else 'nomask', combo[1], combo[2])


def model(N, combo):
    """The inference object of the combination at N (no device is touched here); under a mask the masked y / yerr handed over
    are NaN / inf."""
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc, synth
    masked, order, form = combo
    t, ys, es = synth.rv_series(N, P)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(P, Q))
    y, e = np.array(ys), np.array(es)
    mask = _mask_ref.partial_mask(P, N, MASK_SEED) if masked else None
    if masked:
        y, e = np.where(mask, y, np.nan), np.where(mask, e, np.inf)
    args = [a for i in range(P) for a in (y[i], e[i])]
    g = gpyrn.inference(Q, t, *args, mask=mask, sweep_order=order, sequential_under_mask=True, batch_under_mask=True, elbo=form)
    g.set_components(nodes, weights, means, jit)
    return g


def parameter_sets(g):
    x0 = np.array(g.get_parameters(), dtype=float)
    return [x0 * s for s in SCALES]


def problem_at(g):
    """compose_sweep's problem dict for the model `g` at its CURRENT parameters (under a mask g.y is the zero-filled y)."""
    t = np.asarray(g.time, dtype=float)
    nodes, weights, means, jit = g._get_components()
    Kf, Kw, Lf, Lw, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, g.y)
    return dict(nodes=nodes, weights=weights, means=means, jitters=jit, time=t, Kf=Kf, Kw=Kw, Lf=Lf, Lw=Lw, y_resid=yres,
                y_raw=np.asarray(g.y, dtype=float), yerr2=np.asarray(g.yerr2, dtype=float), jitt2=jitt2, mask=g.mask)


def stop_rule(sweep, mu, var, max_iter):
    """cpu_ref.elbo_calc's loop and stop rule (quirk Q7 included) over any sweep(mu, var): (ELBO, mu, var, trips, crit) with
    crit[k] the rule's criterion after trip k + 4."""
    E, *_ = sweep(mu, var)
    hist, crits, it = [E], [], 0
    while it < max_iter:
        E, mu, var, _ = sweep(mu, var)
        hist.append(E)
        it += 1
        if it > 3:
            last = np.array(hist[-3:])
            crit = np.abs(np.std(last) / np.mean(last))
            crits.append(crit)
            if crit < 1e-3 and crit != 0:
                break
    return E, mu, var, it, np.array(crits)


@functools.lru_cache(maxsize=None)
def reference(N, combo):
    """Per parameter vector: the three forced sweeps (elbo (3,), parts (3, 3), the state after each) and, at N_ONE, the loop
    under the stop rule (elbo, state, trips, crit); plus the shared starting state."""
    g = model(N, combo)
    sets = parameter_sets(g)
    g.set_parameters(sets[0].copy())
    pr0 = problem_at(g)
    every = np.ones((P, N), dtype=bool)
    mu0, var0 = _mask_ref.init_state(pr0, every if g.mask is None else g.mask)
    mu0, var0 = np.array(mu0, dtype=float).ravel(), np.array(var0, dtype=float).ravel()
    out = []
    for x in sets:
        g.set_parameters(x.copy())
        sweep = S.compose_sweep(problem_at(g), *combo)
        E, parts, states = [], [], []
        mu, var = mu0, var0
        for _ in range(N_SWEEPS):
            e, mu, var, pt = sweep(mu, var)
            E.append(e)
            parts.append(pt)
            states.append((np.array(mu, dtype=float).reshape(P + 1, Q, N), np.array(var, dtype=float).reshape(P + 1, Q, N)))
        r = dict(elbo=np.array(E), parts=np.array(parts), states=states)
        if N == N_ONE:
            e, mu, var, it, crit = stop_rule(sweep, mu0, var0, MAX_ITER)
            r.update(loop_elbo=e, loop_mu=np.array(mu, dtype=float).reshape(P + 1, Q, N),
                     loop_var=np.array(var, dtype=float).reshape(P + 1, Q, N), trips=it, crit=crit)
        out.append(r)
    mu0.setflags(write=False)
    var0.setflags(write=False)
    return dict(mu0=mu0, var0=var0, sets=sets, vectors=out)
