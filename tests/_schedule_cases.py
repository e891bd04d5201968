"""The problem and the NumPy restatements behind tests/test_schedule_matrix.py (CPU) and tests/test_schedule_matrix_gpu.py:
the smallest shape on which a sweep runs the FULL outer-panel schedule of csrc/factor.hip, in every combination of data mask,
sweep order and ELBO form that has been merged into that schedule.

The shape: q = 3, p = 2, N = 1290 -- T = 11 tiles, ld = 1408, a last tile of 10 rows.  Read off ensure_tasks (factor.hip) and
sweep_impl (api_sweep.hip), GPRN_OUTER = 4, GPRN_LAT_MAX = 32:

* node phase 3 x 11 = 33 > 32 and weight phase 6 x 11 = 66 > 32: both take the throughput task lists (set 0);
* three outer panels, tiles [0, 4), [4, 8), [8, 11);
* the first panel's update (k1 = 4, n1 = 8, n2 = 11): clsB(i, j) = 2 for j >= 8, i > j + 1, i.e. tile (10, 8) -- a B tile no tile
  step of the first panel touches, so with overlap bit 1 it is formed from K inside the K = 512 update (mode bit 5, ft_s) on the
  bulk stream -- and clsR(i) = 2 for i >= 8: rows 8 .. 10 of R.  So nrest > 0: "rest" runs on the bulk stream, rows_final is
  called behind panels 0 and 1 (rows [0, 4), [4, 8)) and the chain joins the bulk stream at the end;
* node_joins = outers[0][0].nrest > 0 is true, so with overlap bit 16 under the flag schedule the ends of sweeps 1 .. 3 of a call
  of four are deferred to the next sweep's node phase.
(At T = 9 and 10 the first panel's "rest" holds rows of R only -- every B tile beyond the next panel is a diagonal or
sub-diagonal one, which belongs to "next" -- and 3 x 10 = 30 would put the node phase on the latency lists, whose outer panel is
16 tiles: one panel, nothing deferred.  T = 11 is the first at which all of the above holds.)

The model: synth.rv_series(1290, 2) under synth.component_spec(2, 3): QuasiPeriodic nodes, SquaredExponential weights, Constant
means, the flagship workload's components at this size.  The starting state is _initMuVar's with the node means divided by q:
_initMuVar starts every node-weight product at y, so the fit sum_j w_ij f_j at q y, and the reference's order (a Jacobi iteration,
DESIGN.md 2b) carries that excess forward by a factor of 16 per sweep in LogL at q = 3; by sweep 4 the precisions d have grown to
where diag Sigma = (1 - colnorm2(X)) / d has lost the digits the 1e-8 bound needs (two CPU restatements of that trajectory agree
to 1.4e-9 on the variances only, and LogP passes through zero).  From the divided start the four sweeps stay moderate and the
state still moves in every sweep (tests/test_schedule_matrix.py states the agreement that is left).  The mask: _mask_ref.partial_mask(2, 1290, seed 5) plus 40 times at which
EVERY output is masked -- rows of zero precision in the node phase -- across the tile boundary 256, across the boundary 1024
between outer panels 1 and 2, and inside the ragged last tile.

Each restatement is computed once per process (4 forced sweeps, every sweep's ELBO, parts and state kept) and left read-only.
"""
import functools

import numpy as np

from oracle import cpu_ref
from tests import _bound_ref, _mask_ref, _order_mask_ref, _order_ref

N, P, Q = 1290, 2, 3
TILE = 128
T = (N + TILE - 1) // TILE
N_SWEEPS = 4
MASK_SEED = 5
# per output: runs of masked times across a tile boundary (256), across the boundary of outer panels 1 and 2 (1024), in the last tile
ZERO_ROWS = (np.concatenate([np.arange(246, 266), np.arange(1281, 1285)]),
             np.concatenate([np.arange(1018, 1030), np.arange(1285, 1289)]))

# name -> (data mask?, sweep order, ELBO form)
CONFIGS = {
    'plain': (False, 'reference', 'reference'),
    'mask': (True, 'reference', 'reference'),
    'sequential': (False, 'sequential', 'reference'),
    'order_mask': (True, 'sequential', 'reference'),
    'bound': (False, 'reference', 'bound'),
    'bound_order_mask': (True, 'sequential', 'bound'),
}


def data_mask():
    mask = _mask_ref.partial_mask(P, N, MASK_SEED)
    for i, rows in enumerate(ZERO_ROWS):
        mask[:, rows] = True
        mask[i, rows] = False
    return mask


@functools.lru_cache(maxsize=None)
def problem(masked):
    """The model (covfunc / meanfunc objects) and its dense matrices, as tests/_mask_ref.problem lays them out, plus Lf, Lw, the
    mask (None: no mask) and the _initMuVar state (under a mask: of the zero-filled y, as inference forms it)."""
    from gpyrn_amd import covfunc, meanfunc, synth
    t, ys, es = synth.rv_series(N, P)
    nodes, weights, means, jit = synth.build_components(covfunc, meanfunc, synth.component_spec(P, Q))
    y, yerr = np.array(ys), np.array(es)
    mask = data_mask() if masked else None
    if masked:
        assert mask.shape == (P, N) and mask.any(axis=0).all() and not any(mask[i, rows].any() for i, rows in enumerate(ZERO_ROWS))
        y, yerr = np.where(mask, y, 0.0), np.where(mask, yerr, 1.0)
    Kf, Kw, Lf, Lw, yres, jitt2 = cpu_ref.setup(t, nodes, weights, means, jit, y)
    pr = dict(meta=dict(p=P, q=Q, N=N), nodes=nodes, weights=weights, means=means, jitters=jit, time=t, Kf=Kf, Kw=Kw, Lf=Lf,
              Lw=Lw, y_resid=yres, y_raw=y, yerr=yerr, yerr2=yerr ** 2, jitt2=jitt2, mask=mask)
    mu0, var0 = _mask_ref.init_state(pr, np.ones((P, N), dtype=bool) if mask is None else mask)
    pr['mu0'], pr['var0'] = np.array(mu0, dtype=float).ravel(), np.array(var0, dtype=float).ravel()
    pr['mu0'][:Q * N] /= Q                                 # (the node rows: see the module docstring)
    for a in (Kf, Kw, Lf, Lw, yres, pr['y_raw'], pr['yerr'], pr['yerr2'], pr['mu0'], pr['var0']):
        a.setflags(write=False)
    return pr


def compose_sweep(pr, masked, order, form):
    """sweep(mu, var) -> (ELBO, mu, var, parts) of the combination (data mask?, sweep order, ELBO form) on the problem `pr`
    (Kf, Kw, Lf, Lw, y_resid, y_raw, yerr2, jitt2, mask): which restatement each combination is held against, stated once
    (tests/test_small_variants_gpu.py composes its one-tile references through here too)."""
    Kf, Kw, Lf, Lw, y, y_raw, e2, j2, mask = (pr[k] for k in ('Kf', 'Kw', 'Lf', 'Lw', 'y_resid', 'y_raw', 'yerr2', 'jitt2', 'mask'))
    assert (mask is not None) == masked
    if form == 'bound':                                    # tests/_bound_ref.sweeps, route 'B'
        return lambda mu, var: _bound_ref.sweep(Kf, Kw, Lf, Lw, y, e2, j2, mu, var, mask=mask, order=order, route='B')
    if not masked and order == 'reference':                # oracle/cpu_ref
        inv = _order_ref._kf_inv(Lf)
        return lambda mu, var: cpu_ref.sweep_B(Kf, Kw, Lf, Lw, y, y_raw, e2, j2, mu, var, Kf_inv=inv)
    if order == 'reference':                               # tests/_mask_ref.sweeps
        return lambda mu, var: _mask_ref.sweep(Kf, Kw, y, y_raw, e2, j2, mu, var, mask)
    if not masked:                                         # tests/_order_ref.sweeps
        inv = _order_ref._kf_inv(Lf)
        return lambda mu, var: _order_ref.sweep(Kf, Kw, Lf, Lw, y, y_raw, e2, j2, mu, var, 'sequential', Kf_inv=inv)
    return lambda mu, var: _order_mask_ref.sweep(Kf, Kw, y, y_raw, e2, j2, mu, var, mask, 'sequential')   # tests/_order_mask_ref.sweeps


def _one_sweep(name, pr):
    """The `sweep` of configuration `name` that the module's `sweeps` loops over."""
    return compose_sweep(pr, *CONFIGS[name])


def run_sweeps(sweep, mu, var, n=N_SWEEPS):
    """n forced sweeps: per-sweep ELBO (n,), parts (n, 3) and the state after EVERY sweep ([(mu, var)] of shape (p+1, q, N))."""
    E, parts, states = [], [], []
    for _ in range(n):
        e, mu, var, pt = sweep(mu, var)
        E.append(e)
        parts.append(pt)
        states.append((np.array(mu, dtype=float).reshape(P + 1, Q, N), np.array(var, dtype=float).reshape(P + 1, Q, N)))
    return np.array(E), np.array(parts), states


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of configuration `name`, once: dict with the problem, elbo (4,), parts (4, 3), states (after each sweep)."""
    pr = problem(CONFIGS[name][0])
    E, parts, states = run_sweeps(_one_sweep(name, pr), pr['mu0'], pr['var0'])
    for a in (E, parts) + tuple(x for st in states for x in st):
        a.setflags(write=False)
    return dict(pr=pr, elbo=E, parts=parts, states=states)
