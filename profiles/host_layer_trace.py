"""What the Python layer of the side-by-side ("batch") API hands the device context, and what it returns -- recorded without
a GPU, so that two versions of gpyrn_amd/meanfield.py can be compared call for call.

A recording stand-in takes the place of ``_hip.Context`` on an ``inference`` object.  Every method the host layer calls on it
is noted as (method name, sha256 of each array argument's bytes with dtype and shape, scalars), and answers with arrays of
the right shapes drawn from a generator seeded by that very note: the answer depends on everything that was handed over, so
a wrong pairing or order shows in whatever follows.  A vector whose first jitter is ``BAD_LOOP`` gets the verdict info = 3
from its loop (side by side or alone); one whose first jitter is ``BAD_DRAW`` the verdict 7 from its draws.

The public methods are driven over: the side-by-side entry answering / answering None / ``batch_max_N = 0`` (the one-by-one
forms); forced sweeps from a start state / the stop rule from the stored state / the stop rule with no stored state; all
parameters free / one frozen / one frozen and full-length vectors; constant means / Linear means with ``device_means`` / a
user-defined mean without a device program; no failed vector / a failed loop in the middle / a failed draw.  Per case the
record holds the names of the context calls in order, the trace, and as digests the return value (or the exception's
type and text) and the object's ``_mu``, ``_var``, ``last_info``, ``last_nuggets`` and ``get_parameters()`` afterwards.
The file written holds one digest per case over all of that (``condense``; ``--full``: the records themselves, trace
included).  Of every sha256 the first 16 hex digits are kept.

Shapes: p = q = 2, N = 20, B = 3, n* = 7.

usage: python profiles/host_layer_trace.py [--out FILE] [--full] [--tree DIR]
(--tree: import gpyrn_amd from that checkout instead of this one -- run it on the parent commit and on this one: the files
must be byte-identical)"""
import argparse
import contextlib
import hashlib
import io
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, N, B, NS = 2, 2, 20, 3, 7
BAD_LOOP, BAD_DRAW = 0.7531, 0.1357
DIGITS = 16                    # hex digits kept of every sha256 in the record


def _plain(a):
    """`a` as something json can write: scalars as they are, arrays as a digest."""
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if isinstance(a, (np.bool_, np.integer, np.floating)):
        return a.item()
    if type(a).__name__ == 'MeanParams':
        return ['MeanParams', _plain(a.params), _plain(a.y_raw), a.want_mean_grad]
    if isinstance(a, tuple) and hasattr(a, '_fields'):
        return {k: _plain(v) for k, v in a._asdict().items()}
    if isinstance(a, (list, tuple)) and any(isinstance(v, np.ndarray) or v is None for v in a):
        return [_plain(v) for v in a]
    arr = np.ascontiguousarray(a)
    if arr.dtype == object:
        return [_plain(v) for v in a]
    return '%s%s:%s' % (arr.dtype.str, list(arr.shape), hashlib.sha256(arr.tobytes()).hexdigest()[:DIGITS])


def _noted(name):
    def method(self, *args, **kw):
        self._note(name, *args, **kw)
    return method


class Recorder:
    """Stands in for _hip.Context: notes every call, answers deterministically from the note."""
    rank, last_info_gp = 0, 0

    def __init__(self, g, trace, side_by_side):
        self.p, self.q, self.N, self.G = g.p, g.q, g.N, g.q * (g.p + 1)
        self.shape, self.d = (g.p + 1, g.q, g.N), (g.p + 1) * g.q * g.N
        self.trace, self.side_by_side = trace, side_by_side
        self.jit = np.zeros(g.p)

    def _note(self, name, *args, **kw):
        note = [name] + [_plain(a) for a in args] + [[k, _plain(v)] for k, v in sorted(kw.items())]
        self.trace.append(note)
        seed = hashlib.sha256(json.dumps(self.trace[-1]).encode()).digest()
        return np.random.default_rng(int.from_bytes(seed[:8], 'little'))

    # -- what only has to be noted
    def option(self, name, value=-1):
        self._note('option', name, value)
        return 0

    set_sweep_order, set_mask, set_kernel, upload_K = map(_noted, ('set_sweep_order', 'set_mask', 'set_kernel', 'upload_K'))
    set_y_resid, set_muvar, set_mean, keep_sigma = map(_noted, ('set_y_resid', 'set_muvar', 'set_mean', 'keep_sigma'))

    def set_jitters(self, jitters):
        self._note('set_jitters', jitters)
        self.jit = np.array(jitters, dtype=float).ravel()

    def owner_of(self, gp):
        return 0

    def factor_priors(self):
        self._note('factor_priors')
        return 0

    # -- one vector
    def _state(self, rng, lead=()):
        return rng.standard_normal(lead + self.shape), rng.uniform(0.5, 1.5, lead + self.shape)

    def _loop_verdict(self, jit):
        return 3 if abs(float(np.ravel(jit)[0]) - BAD_LOOP) < 1e-12 else 0

    def sweep(self, n=1, commit=True):
        rng = self._note('sweep', n, commit)
        return rng.standard_normal(n), rng.standard_normal((n, 3)), self._loop_verdict(self.jit)

    def get_muvar(self):
        return self._state(self._note('get_muvar'))

    def elbocalc(self, max_iter, setup=False, y_resid=None, jitters=None, mu=None, var=None):
        rng = self._note('elbocalc', max_iter, setup, y_resid, jitters, mu, var)
        if jitters is not None:
            self.jit = np.array(jitters, dtype=float).ravel()
        info = self._loop_verdict(self.jit)
        return (rng.standard_normal(4), 3, not info, info) + self._state(rng)

    def predict(self, tstar):
        rng = self._note('predict', tstar)
        ns = np.size(tstar)
        return rng.standard_normal((self.G, ns)), rng.uniform(0.1, 1.0, (self.G, ns)), 0

    def _draw_verdict(self, jit):
        return 7 if abs(float(np.ravel(jit)[0]) - BAD_DRAW) < 1e-12 else 0

    def predict_draws(self, tstar, z, outputs=True):
        rng = self._note('predict_draws', tstar, z, outputs)
        nd, ns = np.shape(z)[1], np.size(tstar)
        return (rng.standard_normal((self.G, nd, ns)), rng.standard_normal((self.p, nd, ns)), rng.uniform(1e-12, 1e-6, self.G),
                self._draw_verdict(self.jit))

    def grad_elbo(self, n_params):
        return self._note('grad_elbo', n_params).standard_normal(int(n_params))

    def eval_mean(self, mean_params, t=None):
        rng = self._note('eval_mean', mean_params, t)
        return rng.standard_normal((np.atleast_2d(mean_params).shape[0], self.p, self.N if t is None else np.size(t)))

    def eval_mean_grad(self, mean_params, t=None):
        rng = self._note('eval_mean_grad', mean_params, t)
        mp = np.atleast_2d(mean_params)
        return rng.standard_normal((mp.shape[0], mp.shape[1], self.N if t is None else np.size(t)))

    # -- B vectors side by side
    def _head(self, rng, jt, forced):
        jt = np.reshape(jt, (-1, self.p))
        n = jt.shape[0]
        info = np.array([self._loop_verdict(j) for j in jt])
        conv = (info == 0) & (not forced)
        conv[-1] = False                                       # (the last vector's loop ran out of trips)
        return (rng.standard_normal(n), np.full(n, 3), conv, info) + self._state(rng, (n,))

    def elbocalc_batch(self, kp, yr, jt, m0, v0, max_iter, want_state=False, want_grad=False, forced=False):
        rng = self._note('elbocalc_batch', kp, yr, jt, m0, v0, max_iter, want_state, want_grad, forced)
        if not self.side_by_side:
            return None
        out = self._head(rng, jt, forced)
        n = out[0].size
        if type(yr).__name__ == 'MeanParams':
            yr.resid = rng.standard_normal((n, self.p * self.N))
            yr.mean_grad = rng.standard_normal((n, yr.params.shape[1])) if yr.want_mean_grad and want_grad else None
        out = out if want_state else out[:4]
        return out + (rng.standard_normal(np.shape(kp)),) if want_grad else out

    def elbocalc_batch_predict(self, kp, yr, jt, m0, v0, max_iter, tstar, forced=False, latent=True, outputs=True):
        rng = self._note('elbocalc_batch_predict', kp, yr, jt, m0, v0, max_iter, tstar, forced, latent, outputs)
        if not self.side_by_side:
            return None
        out = self._head(rng, jt, forced)
        n, ns = out[0].size, np.size(tstar)
        lm, lv = (rng.standard_normal((n, self.G, ns)) if latent else None for _ in range(2))
        return out + (lm, lv, rng.standard_normal((n, self.p, ns)), rng.uniform(0.1, 1.0, (n, self.p, ns)))

    def elbocalc_batch_draws(self, kp, yr, jt, m0, v0, max_iter, tstar, z, forced=False, latent=True, outputs=True):
        rng = self._note('elbocalc_batch_draws', kp, yr, jt, m0, v0, max_iter, tstar, z, forced, latent, outputs)
        if not self.side_by_side:
            return None
        out = self._head(rng, jt, forced)
        n, nd, ns = out[0].size, np.shape(z)[2], np.size(tstar)
        lat = rng.standard_normal((n, self.G, nd, ns)) if latent else None
        dinfo = np.array([self._draw_verdict(j) for j in np.reshape(jt, (n, self.p))])
        return out + (lat, rng.standard_normal((n, self.p, nd, ns)), rng.uniform(1e-12, 1e-6, (n, self.G)), dinfo)

    def elbocalc_batch_heldout(self, kp, yr, jt, m0, v0, max_iter, fit_masks, forced=False, rows=True):
        rng = self._note('elbocalc_batch_heldout', kp, yr, jt, m0, v0, max_iter, fit_masks, forced, rows)
        if not self.side_by_side:
            return None
        out = self._head(rng, jt, forced)
        n = out[0].size
        held = ~np.asarray(fit_masks, dtype=bool)
        return out + (np.where(held, rng.standard_normal(held.shape), 0.0), np.where(held, rng.uniform(0.1, 1.0, held.shape), 0.0),
                      rng.standard_normal((n, self.p)), held.sum(axis=2))

    def predict_batch(self, kp, mu, var, tstar, jitters=None, latent=True, outputs=True):
        rng = self._note('predict_batch', kp, mu, var, tstar, jitters, latent, outputs)
        if not self.side_by_side:
            return None
        n, ns = np.shape(kp)[0], np.size(tstar)
        lm, lv = (rng.standard_normal((n, self.G, ns)) if latent else None for _ in range(2))
        info = np.array([self._loop_verdict(j) for j in np.reshape(jitters, (n, self.p))])
        return lm, lv, rng.standard_normal((n, self.p, ns)), rng.uniform(0.1, 1.0, (n, self.p, ns)), info


def _object(gpyrn, covfunc, meanfunc, means, **kw):
    """tests/test_varpred_batch.py's small problem, restated."""
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0, 50, N))
    args = []
    for _ in range(P):
        args += [np.sin(t / 6) + 0.1 * rng.standard_normal(N), np.full(N, 0.2)]
    g = gpyrn.inference(Q, t, *args, **kw)
    nodes = [covfunc.SquaredExponential(1.0 + 0.1 * j, 10.0) for j in range(Q)]
    weights = [covfunc.SquaredExponential(0.8 + 0.05 * k, 20.0) for k in range(Q * P)]
    g.set_components(nodes, weights, means, [0.3] * P)
    return g


def _means(meanfunc, kind):
    if kind == 'constant':
        return [meanfunc.Constant(0.1 * (i + 1)) for i in range(P)]
    if kind == 'linear':
        return [meanfunc.Linear(0.01 * (i + 1), 0.1 * (i + 1)) for i in range(P)]

    class Ramp(meanfunc.meanFunction):                         # (defined outside the package: no device program)
        _param_names = ('slope', 'offset')
        _parsize = 2

        def __call__(self, t):
            return self.pars[0] * np.asarray(t, dtype=float) + self.pars[1]
    return [Ramp(0.01 * (i + 1), 0.1 * (i + 1)) for i in range(P)]


def _paths():
    """name -> (constructor keywords, whether the path takes sweeps / start, call)"""
    ts = np.linspace(-5.0, 60.0, NS)
    var_kw, ref_kw = dict(predict='variational'), dict(predict='reference')

    def states(g):
        rng = np.random.default_rng(11)
        shape = (B, g.p + 1, g.q, g.N)
        return rng.standard_normal(shape), rng.uniform(0.5, 1.5, shape)

    def folds(g):
        return g.cv_folds(2, rng=0)

    return {
        'nELBO_batch': (ref_kw, False, lambda g, sets, kw: g.nELBO_batch(sets, max_iter=kw.get('max_iter'))),
        'predict_batch': (ref_kw, False, lambda g, sets, kw: g.predict_batch(sets, tstar=ts, max_iter=kw.get('max_iter'),
                                                                            separate=True)),
        'predict_batch_states': (ref_kw, False, lambda g, sets, kw: g.predict_batch(sets, tstar=ts, states=states(g))),
        'predict_batch_from_sweeps': (var_kw, True, lambda g, sets, kw: g.predict_batch(sets, tstar=ts, from_sweeps=True,
                                                                                        separate=True, **kw)),
        'sample_posterior_batch': (var_kw, True, lambda g, sets, kw: g.sample_posterior_batch(sets, tstar=ts, n=2, noise=True,
                                                                                              separate=True, rng=1, **kw)),
        'nELBO_and_grad_batch_reference': (dict(elbo='reference'), True, lambda g, sets, kw: g.nELBO_and_grad_batch(sets, **kw)),
        'nELBO_and_grad_batch_bound': (dict(elbo='bound'), True, lambda g, sets, kw: g.nELBO_and_grad_batch(sets, **kw)),
        'heldout_batch': (ref_kw, True, lambda g, sets, kw: g.heldout_batch(sets, np.tile(folds(g), (2, 1, 1))[:B], **kw)),
        'cross_validate': (ref_kw, True, lambda g, sets, kw: g.cross_validate(folds(g), sets[:2], **kw)),
        'posterior_predictive_draws': (var_kw, True, lambda g, sets, kw: g.posterior_predictive(sets, tstar=ts, draws=2, rng=3,
                                                                                                **kw)),
    }


def run(tree=None, full=False):
    sys.path.insert(0, os.path.abspath(tree) if tree else HERE)
    import gpyrn_amd as gpyrn
    from gpyrn_amd import covfunc, meanfunc
    record = {'shapes': dict(p=P, q=Q, N=N, B=B, n_star=NS), 'cases': {}}
    for path, (obj_kw, takes_sweeps, call) in _paths().items():
        for mean_kind in ('constant', 'linear', 'user'):
            for vectors in ('free', 'frozen', 'full'):
                for fail in ('none', 'loop', 'draw'):
                    if fail != 'none' and vectors != 'free':
                        continue
                    if fail == 'draw' and 'draw' not in path and 'sample' not in path:
                        continue
                    plainest = (mean_kind, vectors, fail) == ('constant', 'free', 'none')
                    for mode in ('side_by_side', 'entry_none', 'max_N_0'):
                        if mode != 'side_by_side' and path in ('heldout_batch', 'cross_validate') and not plainest:
                            continue                           # (no one-by-one form there: the refusal, once)
                        for loop in (('forced', 'stop_rule', 'no_state') if takes_sweeps else ('stop_rule', 'no_state')):
                            if loop == 'no_state' and (vectors, fail) != ('free', 'none'):
                                continue
                            key = '/'.join((path, mean_kind, vectors, fail, mode, loop))
                            g = _object(gpyrn, covfunc, meanfunc, _means(meanfunc, mean_kind), device_means=mean_kind == 'linear',
                                        **obj_kw)
                            if vectors != 'free':
                                g.freeze_parameter(index=1)
                            if mode == 'max_N_0':
                                g.batch_max_N = 0
                            trace = []
                            g._ctx = Recorder(g, trace, mode == 'side_by_side')
                            g._predict_sent = 'reference'
                            rng = np.random.default_rng(5)
                            x0 = np.array(g.get_parameters(include_frozen=vectors == 'full'), dtype=float)
                            sets = [x0 * rng.uniform(0.9, 1.1, x0.size) for _ in range(B)]
                            if fail != 'none':
                                sets[B // 2][-P] = BAD_LOOP if fail == 'loop' else BAD_DRAW
                            shape = (g.p + 1, g.q, g.N)
                            start = (rng.standard_normal(shape), rng.uniform(0.5, 1.5, shape))
                            kw = dict(max_iter=30)
                            if loop == 'forced':
                                kw = dict(sweeps=2, start=start)
                            elif loop == 'stop_rule':
                                g._mu, g._var = start
                            case = {}
                            with contextlib.redirect_stdout(io.StringIO()) as printed:
                                try:
                                    case['returns'] = _plain(call(g, sets, kw))
                                except (ValueError, NotImplementedError, np.linalg.LinAlgError) as exc:
                                    case['raises'] = [type(exc).__name__, str(exc)]
                            case['printed'] = hashlib.sha256(''.join(c for c in printed.getvalue() if not c.isdigit() and c != '.')
                                                             .encode()).hexdigest()[:16]
                            runs = [(name, len(list(run_))) for name, run_ in itertools.groupby(note[0] for note in trace)]
                            case['calls'] = ' '.join(name if n == 1 else '%s*%d' % (name, n) for name, n in runs)
                            case['trace'] = trace if full else hashlib.sha256(json.dumps(trace).encode()).hexdigest()[:DIGITS]
                            case['after'] = {'mu': _plain(g._mu), 'var': _plain(g._var), 'last_info': _plain(g.last_info),
                                             'last_nuggets': _plain(getattr(g, 'last_nuggets', None)),
                                             'parameters': _plain(np.array(g.get_parameters(), dtype=float))}
                            record['cases'][key] = case
    return record


def condense(record):
    """What the committed file holds of a record: per case ONE digest over everything recorded for it (the return value or
    the refusal, the printed text, the whole trace, the state afterwards), grouped as path -> means/vectors/failure ->
    "mode/loop=digest ..."; the context methods that were called at all; how many cases raised and how many left a
    positive ``last_info``.  ``--full`` writes the records themselves, to find what a differing digest is about."""
    cases = record['cases']
    digests = {}
    for key in sorted(cases):
        path, mean_kind, vectors, fail, mode, loop = key.split('/')
        digest = hashlib.sha256(json.dumps(cases[key], sort_keys=True).encode()).hexdigest()[:DIGITS]
        group = digests.setdefault(path, {}).setdefault('/'.join((mean_kind, vectors, fail)), [])
        group.append('%s/%s=%s' % (mode, loop, digest))
    return {'shapes': record['shapes'], 'cases': len(cases),
            'raised': sum('raises' in c for c in cases.values()),
            'left_last_info': sum(bool(c['after']['last_info']) for c in cases.values()),
            'calls_seen': sorted({name.split('*')[0] for c in cases.values() for name in c['calls'].split()}),
            'digests': {path: {k: ' '.join(v) for k, v in groups.items()} for path, groups in digests.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'host_layer_trace.json'))
    ap.add_argument('--full', action='store_true')
    ap.add_argument('--tree', default=None)
    a = ap.parse_args()
    record = run(a.tree, a.full)
    with open(a.out, 'w') as f:
        json.dump(record if a.full else condense(record), f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d cases, %d raised' % (len(record['cases']), sum('raises' in c for c in record['cases'].values())))


if __name__ == '__main__':
    main()
