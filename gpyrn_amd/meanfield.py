"""Mean-field variational inference for GP regression networks on MI355X.

Drop-in for the reference's ``gpyrn.meanfield.inference`` on its hot path:
``ELBO`` / ``ELBOcalc`` / ``ELBOaux`` / ``nELBO`` / ``optimize`` and the whole
component / parameter API (meanfield.py:92-379, 556-710, 1095-1152), same
names, argument meaning, return shapes and error types.  What differs is where
the work happens: covariance assembly, every Cholesky / triangular inverse and
all ELBO reductions run in libgprn_hip.so (include/gprn_hip.h) on the GPU,
device-resident across sweeps; per sweep only the ELBO scalar returns to the
host for the reference's stop rule (meanfield.py:640-646).

There is no CPU fallback: without the built library and a GPU, anything that
needs the ELBO raises ``_hip.BackendUnavailable``.  Host-side work that remains
is O(#parameters) bookkeeping, O(pN) mean functions and the O(pqN)
``_initMuVar`` start point.

Reference behaviours kept because results must match: the
first ``ELBOaux`` of ``ELBOcalc`` is evaluated and discarded (its ELBO is
``elboArray[0]``); ``max_iter`` defaults to 10000; ``_mu``/``_var`` are cached only
on the converged return; ``_initMuVar`` uses the first p weight amplitudes and
emits the weight block node-major; ELBO = (LogL + LogP + Ent) / q.
"""
import os
import time as time_module
from collections import namedtuple
from itertools import chain

import numpy as np

from . import _hip, covfunc, meanfunc, sharding
from ._utils import Array, _array_input  # noqa: F401

__all__ = ['inference']

_NUGGET = 1e-6          # meanfield.py:433
_TINY_NUGGET = 1.25e-12 # meanfield.py:450
_TWO_ARGUMENT = (covfunc.HarmonicPeriodic, covfunc.QuasiHarmonicPeriodic,
                 covfunc.Polynomial)          # meanfield.py:426-428
_NOT_SET = 'GPRN components not set, use set_components'

# what inference.heldout_batch and inference.cross_validate return (see there)
HeldOut = namedtuple('HeldOut', 'lpd n_held mean var elbo iterations converged info state_mu state_var')
CrossValidation = namedtuple('CrossValidation', 'lpd elpd n_held mean var elbo iterations converged info')


class _Folds(np.ndarray):
    """The (k, p, N) fit masks of ``inference.cv_folds`` with ``n_never_held``: observed entries that no fold holds out."""
    n_never_held = 0

    def __array_finalize__(self, obj):
        self.n_never_held = getattr(obj, 'n_never_held', 0)


def _max_trips(max_iter):
    """ELBOcalc's cap on the loop's trips, its default included (meanfield.py:615-616)."""
    return 10000 if max_iter is None else int(max_iter)


def _first_verdict(info):
    """``last_info`` from the verdicts of B evaluations: the first positive one, else 0."""
    return int(info[np.flatnonzero(info)[0]]) if np.any(info) else 0


class inference:
    """
    Mean-field variational inference for GPRNs (Nguyen & Bonilla 2013).

    Args:
        q: int
            Number of latent node functions f(x)
        time: array
            Time coordinates
        *args: arrays
            The observed data in the following order:
                y1, y1error, y2, y2error, ...
        device: int, keyword only
            GPU ordinal (default: LOCAL_RANK when sharded, else 0)
        comm: ``sharding.Comm``, keyword only
            Shard the q + q*p latent GPs over the ranks of one node
        mask: array-like (p, N) or None, keyword only
            Truthy where output i was observed at time n (not in the reference, whose outputs are observed at every
            time).  A masked entry has zero precision: it is left out of the updates and of the expected
            log-likelihood, and its y / yerr may hold anything (NaN, inf): they are replaced by 0 / 1 here and never
            reach arithmetic.  ``_initMuVar`` reads a masked y as 0.  Every latent GP still lives on all N times;
            ``predict`` at a masked time is the imputation.  ``inference.from_series`` builds a mask from series on
            different time grids.
        sweep_order: 'reference' (default) or 'sequential', keyword only
            The order of a sweep's mean updates (not in the reference).  'reference' is the reference's own: every node
            mean from the OLD means of the other nodes, every weight mean from the OLD weight means of the other nodes of
            its output -- an iteration that diverges at q >= 3.  'sequential' updates the node means in turn, node j from
            the NEW means of the nodes before it, then the weight means in turn over the node index: a proper coordinate
            ascent.  With q = 1 the two are the same computation.  Everything
            that sweeps follows it (``ELBOcalc``, ``nELBO``, ``optimize``, ``mcmc``, ``nELBO_batch``, ``grad_ELBO``, ...)
            except ``ELBOaux`` and ``_updateSigMu``, which restate reference functions.  Not with ``comm``; with ``mask``
            only when ``sequential_under_mask`` is set.
        sequential_under_mask: bool (default False), keyword only
            Whether ``sweep_order='sequential'`` is accepted on an object with a data mask (option ``"order_mask"`` of the
            library).  Off, the two refuse each other as they always have; on, every sweep under the mask runs in the
            sequential order -- what series on different time grids (``from_series``) with q >= 3 nodes need, where the
            reference's order diverges.  An attribute that may be set later (before the order is): it goes to the device
            with every set-up.
        batch_under_mask: bool (default False), keyword only
            Whether the side-by-side forms (``nELBO_batch``, ``mcmc(batch=True)``, ``nELBO_and_grad_batch`` and the states
            behind ``predict_batch`` / ``posterior_predictive``) also run under a data mask.  Off, a masked object
            evaluates one vector after the other, each from its predecessor's state; on, all of them start from one
            shared state, which moves rule-stopped values within the stop rule's 1e-3.  An attribute that may be set
            later, as ``batch_max_N``.  Without a mask it changes nothing.
        exact_derivatives: bool (default False), keyword only
            Whether the gradients (``grad_ELBO`` in both forms, ``nELBO_and_grad``, ``nELBO_and_grad_batch``,
            ``optimize(jac=True, ...)``) differentiate every kernel with a device program exactly on the GPU (option
            ``"grad_exact"`` of the library: Matern, RationalQuadratic, ..., every Sum / Multiplication) where they take
            Richardson-extrapolated central differences of the program by default.  A single SquaredExponential, Periodic
            or QuasiPeriodic keeps its closed form and its bits; kernels without a device program (user subclasses, a Sum
            that holds a two-argument kernel) are contracted on the host as before.  An attribute that may be set later:
            it goes to the device with every set-up.
        device_means: bool (default False), keyword only
            Whether the side-by-side forms evaluate the mean functions of all their parameter vectors on the GPU.
            ``nELBO_batch``, ``mcmc(batch=True)`` and ``nELBO_and_grad_batch`` then hand the library the mean columns of the
            B full vectors (a third layout of ``_batch_stage``: kernel, mean and jitter columns sliced in one go, no
            per-vector ``set_parameters``) and ``gprn_elbocalc_batch_means`` forms ``y - mean`` where the batch keeps it;
            with ``elbo='bound'`` the mean entries of the gradient come back from the same call.  ``predict_batch`` /
            ``posterior_predictive`` take the means at t* from one ``gprn_eval_mean`` call, and
            ``predict_batch(from_sweeps=True)`` its ``y - mean`` likewise.  All of it where every mean has a device program
            (``meanfunc``'s ``_device_program``: Constant, Linear, Parabola, Cubic, Sine, Keplerian and their sums and
            products).  Off, or where a program is missing (``MultiConstant``, user subclasses), anything but Constant means
            is evaluated on the host, one vector after the other, as before.  An attribute that may be set later.  Not
            with ``comm``.
        elbo: 'reference' (default) or 'bound', keyword only
            WHICH function is reported as the ELBO (option ``"elbo_form"`` of the library; not in the reference).
            'reference': the reference's number, quirk for quirk -- node j >= 1 paired with the cumulative covariance
            ``Sigma_f0 + ... + Sigma_fj`` (Q1), weight (j, i) with the raw-reshape row of ``mu_w`` (Q2), the raw ``y`` in the
            likelihood term (Q3), the sum divided by q (Q5) -- which is not the function the updates ascend.  'bound': the
            mean-field lower bound on ``log p(y)`` itself -- every latent GP with its OWN mean and covariance, ``y - mean``
            in the likelihood term, no division -- the objective the coordinate ascent maximises: it rises on every sweep
            of the sequential order and is stationary in the variational state at convergence, so its fixed-state gradient
            IS the total gradient, mean-function parameters included.  The updates, ``_initMuVar``, both sweep orders, the
            stop rule (applied to the new values) and the state are unchanged: the two forms leave the same ``mu`` /
            ``var`` from the same start.  ``ELBOcalc``, ``ELBO``, ``nELBO``, ``nELBO_batch``, ``optimize``, ``mcmc`` and
            the gradients follow it; ``ELBOaux`` and the four step methods restate reference functions and stay in the
            reference's form.  Not with ``comm``.  An attribute that may be set later: it goes to the device with every
            set-up, and a change drops the cached set-up and the stored state.
        predict: 'reference' (default) or 'variational', keyword only
            WHAT ``predict``, ``_Prediction``, ``predict_cov`` and ``sample_posterior`` compute (option ``"predict_form"`` of
            the library; not in the reference; the attribute is ``predict_form``).  'reference': the reference's
            ``_gp.GP.prediction`` -- the variational variances treated as observation noise on ``K + 1.25e-12 I``, factored
            per call, the jitter added once per node.  'variational': the predictive of the posterior the sweeps computed,
            ``q(f_g) = N(mu_g, Sigma_g)``: ``mean* = K* S c``, ``C* = K** - W W^T`` from the factors of the last committed
            sweep, with the set-up's nugget and the jitter added once.  At the data times it returns the stored state --
            the imputation under a data mask included.  Not with ``comm``, not for user-defined kernels, and not (yet) for
            ``predict_batch`` / ``posterior_predictive``.  An attribute that may be set later.
    """

    _SWEEP_ORDERS = {'reference': _hip.ORDER_REFERENCE, 'sequential': _hip.ORDER_SEQUENTIAL}
    _ELBO_FORMS = {'reference': _hip.ELBO_REFERENCE, 'bound': _hip.ELBO_BOUND}
    _PREDICT_FORMS = {'reference': _hip.PREDICT_REFERENCE, 'variational': _hip.PREDICT_POSTERIOR}

    def __init__(self, q: int, time: Array, *args, device=None, comm=None, mask=None, sweep_order='reference',
                 batch_under_mask=False, exact_derivatives=False, sequential_under_mask=False, elbo='reference',
                 predict='reference', device_means=False):
        self.q = q
        self.time = time
        self.N = self.time.size

        assert len(args) > 0 and len(args) % 2 == 0, \
            'Number of observed data arrays should be even: y1, y1error, ...'
        assert np.all(np.array([len(a) for a in args]) == self.N), \
            'Output arrays should all have the same dimensions as time'

        self.p = int(len(args) / 2)
        self.qp = self.q * self.p
        self.d = self.N * self.q * (self.p + 1)

        self.tt = np.tile(time, self.p)                 # "extended" time
        self.y = np.concatenate([args[::2]])            # (p, N)
        self.yerr = np.concatenate([args[1::2]])
        self.mask = None if mask is None else self._check_mask(mask, comm)
        if self.mask is not None:
            # (masked entries never reach arithmetic: the device selects them away, and these values fill them)
            self.y = np.where(self.mask, self.y, 0.0)
            self.yerr = np.where(self.mask, self.yerr, 1.0)
        self.yerr2 = self.yerr**2
        self.batch_under_mask = bool(batch_under_mask)
        self.exact_derivatives = bool(exact_derivatives)
        self.sequential_under_mask = bool(sequential_under_mask)
        self.device_means = bool(device_means)

        self._components_set = False
        self._frozen_mask = np.array([])
        self._mu, self._var = None, None
        self._mu_var_iters = 0
        self.update_muvar_after = 50
        self.elbo_max_iter = 5000

        self._device = device
        self._comm = comm
        self._ctx = None
        self._sweep_order = self._check_sweep_order(sweep_order)
        self._elbo = self._check_elbo(elbo)
        self._predict_form = self._check_predict_form(predict)
        self._predict_sent = 'reference'   # what the context was last told (a new context is in the reference form)
        self._swept = None                 # (the stored state, the parameters, the set-up's key): whose committed sweep the device holds
        self._prior_key = None
        self.last_info = 0

    def _check_mask(self, mask, comm):
        """The (p, N) bool mask, validated before anything touches a device."""
        m = np.asarray(mask)
        if m.shape != (self.p, self.N):
            raise ValueError(f'mask must have shape (p, N) = {(self.p, self.N)}, got {m.shape}')
        m = m.astype(bool)
        empty = np.flatnonzero(~m.any(axis=1))
        if empty.size:
            raise ValueError(f'mask: output(s) {empty.tolist()} have no observed entry')
        if self.q >= 2:
            gaps = np.flatnonzero(~m.any(axis=0))
            if gaps.size:
                raise ValueError(f'mask: with q >= 2 every time needs at least one observed output; no output is '
                                 f'observed at time index(es) {gaps[:10].tolist()}: drop those times from the data '
                                 f'(predict still reaches them)')
        if comm is not None:
            raise NotImplementedError('mask: a sharded inference object does not support a data mask')
        return m

    def _check_sweep_order(self, order):
        """'reference' or 'sequential', validated before anything touches a device."""
        if not isinstance(order, str) or order not in self._SWEEP_ORDERS:
            raise ValueError(f"sweep_order must be 'reference' or 'sequential', got {order!r}")
        if order != 'reference':
            if self.mask is not None and not self.sequential_under_mask:
                raise NotImplementedError('sweep_order: the sequential order is not supported under a data mask')
            if self._comm is not None:
                raise NotImplementedError('sweep_order: the sequential order is not supported on a sharded inference object')
        return order

    @property
    def sweep_order(self):
        """ 'reference' or 'sequential': the order of a sweep's mean updates """
        return self._sweep_order

    @sweep_order.setter
    def sweep_order(self, order):
        self._sweep_order = self._check_sweep_order(order)
        if self._ctx is not None:
            # (the device lets "order_mask" go only once the mask and the sequential order are no longer both in force)
            if self._sweep_order != 'reference':
                self._send_order_mask(self._ctx)
            self._ctx.set_sweep_order(self._SWEEP_ORDERS[self._sweep_order])
            if self._sweep_order == 'reference':
                self._send_order_mask(self._ctx)

    def _check_elbo(self, form):
        """'reference' or 'bound', validated before anything touches a device."""
        if not isinstance(form, str) or form not in self._ELBO_FORMS:
            raise ValueError(f"elbo must be 'reference' or 'bound', got {form!r}")
        if form != 'reference' and self._comm is not None:
            raise NotImplementedError('elbo: the bound form is not supported on a sharded inference object')
        return form

    @property
    def elbo(self):
        """ 'reference' or 'bound': which function is reported as the ELBO """
        return self._elbo

    @elbo.setter
    def elbo(self, form):
        form = self._check_elbo(form)
        if form != self._elbo:
            # (the device's set-up belongs to the other form, and a stored state was accepted by the other form's stop rule)
            self._prior_key = None
            self._mu, self._var = None, None
            self._swept = None
        self._elbo = form
        if self._ctx is not None:
            self._send_elbo_form(self._ctx)

    def _send_elbo_form(self, ctx, form=None):
        """Option "elbo_form" from the object's form (or `form`: the reference restatements ask for 'reference').  A change
        clears the device's set-up: the cached key goes with it."""
        want = self._ELBO_FORMS[self._check_elbo(self._elbo if form is None else form)]
        if ctx.option('elbo_form', want) != want:
            self._prior_key = None

    @property
    def _prior_key(self):
        """What names the kernels whose factors the device holds (None: nothing does)."""
        return self._prior_key_value

    @_prior_key.setter
    def _prior_key(self, key):
        # (whoever touches the device's kernels or their factors -- a set-up, ELBOaux and the step methods with their uploaded
        # matrices, a prediction with other components -- assigns here: the committed sweep the marker vouched for is gone)
        self._prior_key_value = key
        self._swept = None

    def _check_predict_form(self, form):
        """'reference' or 'variational', validated before anything touches a device."""
        if not isinstance(form, str) or form not in self._PREDICT_FORMS:
            raise ValueError(f"predict must be 'reference' or 'variational', got {form!r}")
        if form != 'reference' and self._comm is not None:
            raise NotImplementedError('predict: the variational form is not supported on a sharded inference object')
        return form

    @property
    def predict_form(self):
        """ 'reference' or 'variational': what predict, _Prediction, predict_cov and sample_posterior compute """
        return self._predict_form

    @predict_form.setter
    def predict_form(self, form):
        self._predict_form = self._check_predict_form(form)

    def _send_predict_form(self, ctx):
        """Option "predict_form" from the object's form, before every prediction (nothing on the device changes with it).
        A context that never left the reference form is not asked."""
        form = self._check_predict_form(self._predict_form)
        if form != self._predict_sent:
            ctx.option('predict_form', self._PREDICT_FORMS[form])
            self._predict_sent = form

    def _mark_swept(self, nodes, weights, means, jitters):
        """The private marker of the variational form of prediction: the device's committed sweep is the one that produced
        the stored state -- kept as (that very state array, the parameter vector it belongs to, the key of the set-up), so
        that a new stored state, ``set_parameters``, ``set_components`` or a component changed in place all make it stale;
        every assignment to ``_prior_key`` drops it (a set-up, ``ELBOaux`` and the step methods, a prediction with other
        components), as does a new context; what else stages another state on the device shows in the library's read-only
        option "state_ready"."""
        own = self._components_set and nodes is self.nodes and weights is self.weights and means is self.means \
            and jitters is self.jitters
        ok = own and self._mu is not None and self._prior_key is not None
        self._swept = (self._mu, self._parameter_snapshot(), self._prior_key) if ok else None

    def _parameter_snapshot(self):
        """Every parameter value of the object's components (a mean function may be None), as one vector."""
        pieces = [np.ravel(np.asarray(c.pars, dtype=float)) for c in self._component_chain() if c is not None and hasattr(c, 'pars')]
        pieces.append(np.ravel(np.asarray(self.jitters, dtype=float)))
        return np.concatenate(pieces)

    def _is_swept(self, ctx):
        if self._swept is None or self._mu is None or self._swept[0] is not self._mu:
            return False
        if not np.array_equal(self._swept[1], self._parameter_snapshot()):
            return False
        if self._prior_key is None or self._swept[2] != self._prior_key:
            return False
        return ctx.option('state_ready') == 1

    def _send_order_mask(self, ctx):
        """Option "order_mask" from ``sequential_under_mask``, the object's order validated against it first (the attribute
        may have changed since the order was set)."""
        self._check_sweep_order(self._sweep_order)
        ctx.option('order_mask', 1 if self.sequential_under_mask else 0)

    @classmethod
    def from_series(cls, q, series, **kwargs):
        """
        An inference object from p series on their own time grids: ``series`` = [(t1, y1, e1), (t2, y2, e2), ...].
        The time vector is the sorted union of the grids (a time that several series share appears once), and the
        mask marks which output was observed at which time.  Keyword arguments go to the constructor.
        """
        series = [tuple(np.asarray(a, dtype=float).ravel() for a in s) for s in series]
        if not series:
            raise ValueError('from_series: no series given')
        for t, y, e in series:
            if not (t.size == y.size == e.size):
                raise ValueError('from_series: t, y and yerr of a series must have the same length')
            if np.unique(t).size != t.size:
                raise ValueError('from_series: a series has a repeated time')
        time = np.unique(np.concatenate([s[0] for s in series]))
        p, N = len(series), time.size
        y, e = np.zeros((p, N)), np.ones((p, N))
        mask = np.zeros((p, N), dtype=bool)
        for i, (t, yi, ei) in enumerate(series):
            idx = np.searchsorted(time, t)
            y[i, idx], e[i, idx], mask[i, idx] = yi, ei, True
        args = [a for i in range(p) for a in (y[i], e[i])]
        return cls(q, time, *args, mask=mask, **kwargs)

    def _refuse_masked(self, what):
        if self.mask is not None:
            raise NotImplementedError(f'{what} is not supported under a data mask')

    # ------------------------------------------------------------ components
    def set_components(self, nodes, weights, means, jitters):
        """
        Set the GPRN components: q node kernels, q*p weight kernels (flat
        order node-major: weight of node j and output i at index j*p + i),
        p mean functions and p jitters.  Bare objects are accepted for
        single-element lists.
        """
        if isinstance(nodes, covfunc.covFunction):
            nodes = [nodes]
        if len(nodes) != self.q:
            raise ValueError('Wrong number of nodes provided, '
                             f'expected {self.q} got {len(nodes)}')
        if isinstance(weights, covfunc.covFunction):
            weights = [weights]
        if len(weights) != self.qp:
            raise ValueError('Wrong number of weights provided, '
                             f'expected {self.qp} got {len(weights)}')
        if isinstance(means, (int, float, meanfunc.meanFunction)):
            means = [means]
        if isinstance(jitters, (int, float)):
            jitters = [jitters]

        self.nodes = nodes
        self.weights = weights
        self.means = means
        self.jitters = np.array(jitters, dtype=float)
        self._components_set = True
        self._swept = None

    def _component_chain(self):
        return chain.from_iterable([self.nodes, self.weights, self.means])

    def get_parameters(self, nodes=None, weights=None, means=None,
                       jitters=None, include_frozen=False):
        """ Values of all the GPRN parameters: nodes, weights, means, jitters """
        given = (nodes, weights, means, jitters)
        if not self._components_set and all(g is None for g in given):
            raise ValueError('Cannot get parameters. '
                             'Provide arguments or run set_components before.')
        if self._components_set:
            nodes, weights, means, jitters = (self.nodes, self.weights,
                                              self.means, self.jitters)
        pieces = []
        for group in (nodes, weights, means):
            if group is not None:
                pieces += [c.get_parameters() for c in group]
        if jitters is not None:
            pieces += [np.array([j]) for j in jitters]
        flat = np.concatenate(pieces).ravel()
        return flat if include_frozen else flat[~self.frozen_mask]

    @_array_input
    def set_parameters(self, parameters: Array):
        """ Set all parameters (full vector, or only the non-frozen ones) """
        assert self._components_set, _NOT_SET
        current = self.get_parameters(include_frozen=True)
        n_all = self.n_parameters
        n_free = n_all - self.frozen_mask.sum()

        if parameters.size == n_all:
            parameters[self.frozen_mask] = current[self.frozen_mask]
        elif parameters.size == n_free:
            for i, value in enumerate(current):
                if self.frozen_mask[i]:
                    parameters = np.insert(parameters, i, value)
        else:
            msg = f'Wrong number of parameters provided: got {parameters.size}, '
            msg += f'expected {n_all}' if n_all == n_free else \
                f'expected {n_all} (all) or {n_free} (not frozen)'
            raise ValueError(msg)

        for component in self._component_chain():
            parameters = component.set_parameters(parameters)
        self.jitters = parameters
        self._swept = None

    @property
    def n_parameters(self):
        """ Total number of parameters """
        assert self._components_set, _NOT_SET
        return sum(c.pars.size for c in self._component_chain()) + self.jitters.size

    @property
    def parameters_dict(self):
        """ Dictionary with parameters names and values """
        assert self._components_set, _NOT_SET
        out = {}
        for label, group in (('node', self.nodes), ('weight', self.weights),
                             ('mean', self.means)):
            for i, comp in enumerate(group, start=1):
                for name, value in zip(comp._param_names, comp.pars):
                    out[f'{label}{i}.{name}'] = value
        for i, jit in enumerate(self.jitters, start=1):
            out[f'jitter{i}'] = jit
        return out

    def _set_frozen(self, value, index, name):
        self.frozen_mask        # materialise the mask
        if index is None and name is None:
            raise ValueError('Provide either index or name')
        if name is None:
            self._frozen_mask[index] = value
        elif index is None:
            names = list(self.parameters_dict.keys())
            if '*' in name:
                stem = name.replace('*', '')
                for i, known in enumerate(names):
                    if stem in known:
                        self._frozen_mask[i] = value
            else:
                assert name in names, f'Name "{name}" not found in parameters_dict'
                self._frozen_mask[names.index(name)] = value

    def freeze_parameter(self, index=None, name=None):
        """ Freeze (do not fit for) a parameter by index or name; a "*" in
        `name` matches every parameter whose name contains the rest. """
        self._set_frozen(True, index, name)

    def thaw_parameter(self, index=None, name=None):
        """ Thaw (free) a parameter by index or name ("*" as in freeze). """
        self._set_frozen(False, index, name)

    def freeze_all_parameters(self):
        self._frozen_mask = np.ones(self._frozen_mask.size, dtype=bool)

    def thaw_all_parameters(self):
        self._frozen_mask = np.zeros(self._frozen_mask.size, dtype=bool)

    fix_parameter = freeze_parameter
    fix_all_parameters = freeze_all_parameters
    free_parameter = thaw_parameter
    free_all_parameters = thaw_all_parameters

    @property
    def frozen_mask(self):
        """ Boolean mask for the frozen parameters """
        assert self._components_set, _NOT_SET
        if self._frozen_mask.size == 0:
            self._frozen_mask = np.full(self.n_parameters, False, dtype=bool)
        return self._frozen_mask

    @frozen_mask.setter
    def frozen_mask(self, mask):
        raise NotImplementedError(
            'Do not set frozen_mask, use thaw_parameter/freeze_parameter')

    # ------------------------------------------------------------- host glue
    def _mean(self, means, time=None):
        """ Mean functions evaluated at `time` (default: the data), flat (p*N,) """
        t = self.time if time is None else time
        n = t.size
        m = np.zeros(n * self.p)
        for i, fun in enumerate(means):
            if fun is not None:
                m[i * n:(i + 1) * n] = fun(t)
        return m

    def _u_to_fhatW(self, u):
        """ Split a flat variational vector: nodes (1,q,N), weights (p,q,N) """
        f = u[:self.q * self.N].reshape((1, self.q, self.N))
        w = u[self.q * self.N:].reshape((self.p, self.q, self.N))
        return f, w

    def _initMuVar(self, nodes, weights, jitter):
        """ Data-driven start point of the coordinate ascent (meanfield.py:491-510) """
        jitter = np.asarray(jitter, dtype=float)
        w_amp = np.array([w.pars[0] for w in weights][:self.p])[:, None]
        absy, sgn = np.abs(self.y), np.sign(self.y)
        mu_f, mu_w, var_f, var_w = [], [], [], []
        for node in nodes:
            a = node.pars[0]
            mu_f.append(np.mean(np.sqrt(absy * a / w_amp) * sgn, axis=0))
            mu_w.append(np.sqrt(absy * w_amp / a))
            var_f.append(np.full(self.N, np.mean(jitter)))
            var_w.append(jitter[:, None] * np.ones((self.p, self.N)))
        mu = np.concatenate((mu_f, mu_w), axis=None)
        var = np.concatenate((var_f, var_w), axis=None)
        return mu, var

    def _randomMuVar(self):
        return np.random.randn(self.d, 1), np.random.rand(self.d, 1)

    def _get_components(self, nodes=None, weights=None, means=None,
                        jitters=None):
        if all(i is None for i in (nodes, weights, means, jitters)) \
                and not self._components_set:
            raise ValueError(_NOT_SET)
        nodes = self.nodes if nodes is None else nodes
        weights = self.weights if weights is None else weights
        means = self.means if means is None else means
        jitters = self.jitters if jitters is None else jitters
        return nodes, weights, means, jitters

    # ---------------------------------------------------------------- device
    def _backend(self):
        """The GPU context of this problem (created on first use, after fork)."""
        if self._ctx is None:
            comm = self._comm
            device = self._device
            if device is None:
                # one rank per GPU; with fewer GPUs than ranks (rehearsals) ranks share devices
                device = comm.local_rank % max(1, _hip.device_count()) if comm is not None else 0
            ctx = _hip.Context(device)
            self._predict_sent = 'reference'                      # (a new context is in the reference form)
            self._prior_key = None                                # (... holds no set-up and no sweep: the marker goes too)
            forced = bool(os.environ.get('GPRN_FORCE_RCCL'))      # one-rank communicator, for tests
            if comm is not None and (comm.world > 1 or forced):
                ctx.comm_init(comm.world, comm.rank, comm.unique_id())
                comm.done()
            ctx.set_data(np.asarray(self.time, dtype=float), self.y, self.yerr, self.q)
            self._send_order_mask(ctx)                            # (before the order and the mask: each asks for it)
            if self._sweep_order != 'reference':
                ctx.set_sweep_order(self._SWEEP_ORDERS[self._sweep_order])
            if self.mask is not None and not self.mask.all():     # (an all-True mask is no mask: the same kernels run)
                ctx.set_mask(self.mask)
            if self._elbo != 'reference':
                self._send_elbo_form(ctx)
            if self._predict_form != 'reference':
                self._send_predict_form(ctx)
            if comm is not None and comm.world > 1:
                ctx.set_owners(sharding.owners(self.p, self.q, comm.world))
            self._ctx = ctx
        return self._ctx

    def _host_K(self, kernel, time):
        """Kernel matrix evaluated in Python: the path for user-defined kernels."""
        if isinstance(kernel, _TWO_ARGUMENT):
            return kernel(time[:, None], time[None, :])
        r = time[:, None] - time[None, :]
        return kernel(r) + _NUGGET * np.eye(time.size)

    def _kernel_spec(self, kernel):
        """How a kernel reaches the device: a postfix program for the fused fill
        (built-ins and their sums/products), or a host-evaluated matrix."""
        program = kernel._device_program() if isinstance(kernel, covfunc.covFunction) else None
        if program is None:
            K = np.asarray(self._host_K(kernel, np.asarray(self.time, dtype=float)), dtype=float)
            return ('host', K)
        ops, params = program
        return ('device', tuple(ops), np.asarray(params, dtype=float),
                not isinstance(kernel, _TWO_ARGUMENT))

    @staticmethod
    def _spec_key(spec):
        if spec[0] == 'host':
            return ('host', spec[1].tobytes())
        return ('device', spec[1], spec[2].tobytes(), spec[3])

    @staticmethod
    def _send_spec(ctx, gp, spec):
        if spec[0] == 'host':
            ctx.upload_K(gp, spec[1])
        else:
            ctx.set_kernel(gp, spec[1], spec[2], spec[3])

    def _device_K(self, kernel, time, nugget):
        """K = kernel at the data times + nugget on the diagonal through the fused HIP fill (built-in kernels
        and their sums / products at the data's own time stamps), else None."""
        if not (time is self.time or (np.shape(time) == np.shape(self.time)
                                      and np.array_equal(time, self.time))):
            return None
        program = kernel._device_program() if isinstance(kernel, covfunc.covFunction) else None
        if program is None:
            return None
        ops, params = program
        two = isinstance(kernel, _TWO_ARGUMENT)        # evaluated without a nugget (meanfield.py:426-431)
        return self._backend().eval_kernel(ops, params, 0.0 if two else nugget)

    def _KMatrix(self, kernel, time=None):
        """
        Covariance matrix of `kernel` at the data times, with the reference's
        1e-6 nugget (meanfield.py:413-434).  Built by the fused HIP fill kernel
        for built-in kernels when `time` is the data's own time vector.
        """
        time = self.time if time is None else time
        K = self._device_K(kernel, time, _NUGGET)
        return self._host_K(kernel, np.asarray(time, dtype=float)) if K is None else K

    def _tinyNuggetKMatrix(self, kernel, time=None):
        """Covariance matrix with the tiniest stability nugget, 1.25e-12 (meanfield.py:436-452)."""
        time = self.time if time is None else time
        K = self._device_K(kernel, time, _TINY_NUGGET)
        if K is not None:
            return K
        time = np.asarray(time, dtype=float)
        if isinstance(kernel, _TWO_ARGUMENT):
            return kernel(time[:, None], time[None, :])
        r = time[:, None] - time[None, :]
        return kernel(r) + _TINY_NUGGET * np.eye(time.size)

    def _predictKMatrix(self, kernel, time):
        """Cross-covariance between new times and the data times (meanfield.py:455-471; _gp.py:52-63 for
        the two-argument kernels), evaluated in Python: the path of user-defined kernels in prediction."""
        time = np.atleast_1d(np.asarray(time, dtype=float))
        data_t = np.asarray(self.time, dtype=float)
        if isinstance(kernel, _TWO_ARGUMENT):
            return kernel(time[:, None], data_t[None, :])
        return kernel(time[:, None] - data_t[None, :])

    def _sample_from_gp(self, kernel, time=None):
        """
        One draw from the GP prior of `kernel` at `time` (meanfield.py:517-531).  The reference hands the
        tiny-nugget matrix to scipy's ``multivariate_normal(..., allow_singular=True)``; here the draw is
        ``L z`` with ``z`` from NumPy's global generator and ``K + nugget I = L L^T`` factored on the GPU,
        the nugget growing from 1.25e-12 by factors of 100 (to 1.25e-6 at most) while fp64 finds the matrix
        not positive definite -- what ``allow_singular`` papers over on the CPU.  Same distribution, not
        the same stream of numbers.  Kernels without a device program are factored on the host.
        """
        time = self.time if time is None else time
        n = np.size(time)
        z = np.random.standard_normal(n)
        program = kernel._device_program() if isinstance(kernel, covfunc.covFunction) else None
        same_t = time is self.time or (np.shape(time) == np.shape(self.time) and np.array_equal(time, self.time))
        nugget = _TINY_NUGGET
        while True:
            if program is not None and same_t and not isinstance(kernel, _TWO_ARGUMENT):
                out, info = self._backend().sample_prior(program[0], program[1], nugget, z[None])
                if info == 0:
                    return out[0]
            else:
                K = self._tinyNuggetKMatrix(kernel, np.asarray(time, dtype=float))
                K = K + (nugget - _TINY_NUGGET) * np.eye(n)
                try:
                    return np.linalg.cholesky(K) @ z
                except np.linalg.LinAlgError:
                    pass
            if nugget >= 1e-6:
                raise np.linalg.LinAlgError('prior covariance is not positive definite even with a 1e-6 nugget')
            nugget *= 100.0

    def sample(self, time=None):
        """Draws of every node and weight GP from its prior (meanfield.py:533-539; it prints the two
        shapes, so does this).  Returns (node_samples (q, N), weight_samples (q*p, N))."""
        nodes, weights, means, jitters = self._get_components()
        node_samples = np.array([self._sample_from_gp(node) for node in nodes])
        weight_samples = np.array([self._sample_from_gp(weight) for weight in weights])
        print(node_samples.shape)
        print(weight_samples.shape)
        return node_samples, weight_samples

    def _setup_device(self, nodes, weights, means, jitters):
        """The setup block of ELBOcalc (meanfield.py:618-624) on the GPU."""
        ctx = self._backend()
        ctx.option('grad_exact', 1 if self.exact_derivatives else 0)   # (every set-up: the attribute may have changed)
        self._send_order_mask(ctx)
        self._send_elbo_form(ctx)
        specs = [self._kernel_spec(k) for k in chain(nodes, weights)]
        key = tuple(self._spec_key(s) for s in specs)
        if key != self._prior_key:             # unchanged hyper-parameters keep their factors
            self._prior_key = None             # (nothing names the device's kernels until the set-up has succeeded)
            for gp, spec in enumerate(specs):
                self._send_spec(ctx, gp, spec)
            self.last_info = ctx.factor_priors()
            self._prior_key = key
        y = np.concatenate(self.y) - self._mean(means)
        ctx.set_y_resid(np.array(np.array_split(y, self.p)))
        ctx.set_jitters(np.asarray(jitters, dtype=float))
        return ctx

    # ------------------------------------------------------------------ ELBO
    @property
    def ELBO(self):
        """ The evidence lower bound for the GPRN """
        return self.ELBOcalc()[0]

    def ELBOcalc(self, nodes=None, weights=None, means=None, jitters=None,
                 max_iter=None, mu=None, var=None):
        """
        Calculate the evidence lower bound by coordinate ascent on the
        variational means/variances.

        Args:
            nodes, weights, means, jitters: optional overrides of the components
            max_iter: int, default 10000
            mu, var: arrays (flat d or (p+1,q,N)), or 'init', 'random', 'previous'

        Returns:
            ELBO (float), mu (p+1,q,N), var (p+1,q,N), iterNumber (int)
        """
        nodes, weights, means, jitters = self._get_components(
            nodes, weights, means, jitters)

        if mu is None or var is None:
            mu = var = 'init'
        mu_s = mu if isinstance(mu, str) else None
        var_s = var if isinstance(var, str) else None
        if mu_s == 'previous' or var_s == 'previous':
            if self._mu is not None:
                mu, var = self._mu, self._var
            else:
                mu, var = self._initMuVar(nodes, weights, jitters)
        elif mu_s == 'random' and var_s == 'random':
            mu, var = self._randomMuVar()
        elif mu_s == 'init' and var_s == 'init':
            mu, var = self._initMuVar(nodes, weights, jitters)

        if max_iter is None:
            max_iter = 10000

        # meanfield.py:618-649 in ONE call of the library: the set-up (when a hyper-parameter of a kernel has changed:
        # unchanged ones keep their factors), y - mean and the jitters, the starting state, then the loop -- the first
        # sweep's update thrown away and only its ELBO kept, sweeps to the stop rule or max_iter
        ctx = self._backend()
        self._send_elbo_form(ctx)
        self._swept = None
        specs = [self._kernel_spec(k) for k in chain(nodes, weights)]
        key = tuple(self._spec_key(s) for s in specs)
        setup = key != self._prior_key
        if setup:
            # (from here to the end of a successful set-up the device holds kernels -- possibly factors -- that no key
            # names: a call that raises in between must not leave the old key standing for them)
            self._prior_key = None
            for gp, spec in enumerate(specs):
                self._send_spec(ctx, gp, spec)
            self.last_info = 0
        y = np.concatenate(self.y) - self._mean(means)
        history, iterNumber, converged, info, mu, var = ctx.elbocalc(
            max_iter, setup=setup, y_resid=y, jitters=np.asarray(jitters, dtype=float),
            mu=np.asarray(mu, dtype=float), var=np.asarray(var, dtype=float))
        if setup:
            self._prior_key = key
        self.last_info = self.last_info or info
        self._elbo_history = history
        ELBO = np.float64(history[-1])
        if converged:
            self._mu, self._var = mu, var
            if info == 0 and iterNumber >= 1:
                self._mark_swept(nodes, weights, means, jitters)
            return ELBO, mu, var, iterNumber

        print('\nMax iterations reached')
        return ELBO, mu, var, iterNumber

    def ELBOaux(self, Kf, Kw, Lf, Lw, y, jitt2, mu, var):
        """
        One coordinate-ascent sweep + ELBO from explicit host matrices
        (compatibility with meanfield.py:651-710; `Lf`/`Lw` are recomputed on the
        device and ignored).  Returns ELBO, new_mu, new_var, sigmaF (q,N,N),
        sigmaW (q,p,N,N).
        """
        self._refuse_masked('ELBOaux')
        ctx = self._backend()
        self._send_elbo_form(ctx, 'reference')             # (a restatement of the reference's function: its form, always)
        Kf = np.asarray(Kf, dtype=float).reshape(self.q, self.N, self.N)
        Kw = np.asarray(Kw, dtype=float).reshape(self.qp, self.N, self.N)
        for gp, K in enumerate(chain(Kf, Kw)):
            ctx.upload_K(gp, K)
        self._prior_key = None
        self.last_info = ctx.factor_priors()
        ctx.set_y_resid(np.asarray(y, dtype=float).reshape(self.p, self.N))
        ctx.set_jitters(np.sqrt(np.asarray(jitt2, dtype=float)))
        ctx.set_muvar(np.asarray(mu, dtype=float), np.asarray(var, dtype=float))
        ctx.keep_sigma(True)
        ctx.set_sweep_order(_hip.ORDER_REFERENCE)          # (a restatement of the reference's function: its order, always)
        try:
            e, _, info = ctx.sweep(1, commit=True)
            sigmaF = np.array([ctx.get_matrix(_hip.M_SIGMA, j) for j in range(self.q)])
            sigmaW = np.array([ctx.get_matrix(_hip.M_SIGMA, self.q + k)
                               for k in range(self.qp)]).reshape(self.q, self.p, self.N, self.N)
            new_mu, new_var = ctx.get_muvar()
        finally:
            ctx.keep_sigma(False)
            ctx.set_sweep_order(self._SWEEP_ORDERS[self._sweep_order])
            self._send_elbo_form(ctx)
        self.last_info = self.last_info or info
        return np.float64(e[0]), new_mu, new_var, sigmaF, sigmaW

    # ------------------------------------------------- the four step methods ELBOaux is made of (meanfield.py:713, 895, 992, 1069)
    # Private in the reference, but part of its class: a script that calls them finds them here with the reference's
    # signatures and return shapes, computed on the device -- the sweep itself for _updateSigMu, the factorisation for
    # _entropy, the resident factors plus one triangular product per latent GP for _expectedLogPrior, the ELBO assembly's own
    # kernel for _expectedLogLike.  Each invalidates the object's cached set-up (the next ELBOcalc refactors).
    def _updateSigMu(self, Kf, Kw, Lf, Lw, y, jitt2, muF, varF, muW, varW):
        """Closed-form updates of the variational covariances and means (meanfield.py:713-893; eqs. 16-19 of Nguyen &
        Bonilla 2013): ``(sigma_f (q, N, N), mu_f (q, N), sigma_w (q, p, N, N), mu_w (p, q, N))`` from the prior
        matrices, ``y - mean``, the squared jitters and the current state split as ``_u_to_fhatW`` splits it.  One device
        sweep with the explicit covariances kept (as ``ELBOaux``); ``Lf`` / ``Lw`` are recomputed there."""
        self._refuse_masked('_updateSigMu')
        q, p, N = self.q, self.p, self.N
        mu = np.concatenate((np.reshape(muF, (1, q, N)), np.reshape(muW, (p, q, N))))
        var = np.concatenate((np.reshape(varF, (1, q, N)), np.reshape(varW, (p, q, N))))
        _, new_mu, _, sigma_f, sigma_w = self.ELBOaux(Kf, Kw, Lf, Lw, y, jitt2, mu, var)
        return sigma_f, new_mu[0], sigma_w, new_mu[1:]

    def _entropy(self, sigma_f, sigma_w):
        """Entropy of the variational distribution (meanfield.py:1069-1093): ``sum log diag chol(Sigma)`` over the q + q p
        covariances ``+ q (p + 1) N (1 + log 2 pi) / 2``.  The Choleskys run on the device (the covariances go in as the
        latent GPs' matrices, the set-up's factorisation returns ``log det``); a covariance that is not positive definite
        gives NaN, as jax's cholesky does."""
        self._refuse_masked('_entropy')
        q, p, N = self.q, self.p, self.N
        sigma_f = np.asarray(sigma_f, dtype=float).reshape(q, N, N)
        sigma_w = np.asarray(sigma_w, dtype=float).reshape(q, p, N, N)
        ctx = self._backend()
        self._prior_key = None
        for j in range(q):
            ctx.upload_K(j, sigma_f[j])
            for i in range(p):
                ctx.upload_K(q + j * p + i, sigma_w[j, i])
        info = ctx.factor_priors()
        self.last_info = info
        if info:
            return np.float64(np.nan)
        return np.float64(0.5 * np.sum(ctx.get_logdet_K()) + 0.5 * q * (p + 1) * N * (1.0 + np.log(2.0 * np.pi)))

    def _expectedLogPrior(self, Kf, Kw, Lf, Lw, sigma_f, mu_f, sigma_w, mu_w):
        """Expectation of the log prior under q(f, w) (meanfield.py:992-1067; eq. 15): per latent GP
        ``-log det K / 2 - (m^T K^-1 m + tr(K^-1 S)) / 2``, node j with the CUMULATIVE ``S = Sigma_f0 + ... + Sigma_fj``
        (:1025, 1039: quirk Q1), weight (j, i) with the raw reshape ``mu_w.reshape(q, p, N)[j, i]`` (:1021: quirk Q2),
        ``- N q (p + 1) log(2 pi) / 2``.  The matrices are factored on the device (``Lf`` / ``Lw`` are recomputed there) and
        every term comes from the resident factor (``gprn_prior_terms``: tr(K^-1 S) as one triangular product, N^3)."""
        self._refuse_masked('_expectedLogPrior')
        q, p, N = self.q, self.p, self.N
        Kf = np.asarray(Kf, dtype=float).reshape(q, N, N)
        Kw = np.asarray(Kw, dtype=float).reshape(q * p, N, N)
        sigma_f = np.asarray(sigma_f, dtype=float).reshape(q, N, N)
        sigma_w = np.asarray(sigma_w, dtype=float).reshape(q, p, N, N)
        mf = np.asarray(mu_f, dtype=float).reshape(q, N)
        mw = np.asarray(mu_w, dtype=float).reshape(q, p, N)              # quirk Q2
        ctx = self._backend()
        self._prior_key = None
        for gp, K in enumerate(chain(Kf, Kw)):
            ctx.upload_K(gp, K)
        info = ctx.factor_priors()
        self.last_info = info
        if info:
            return np.float64(np.nan)
        total = 0.0
        cumulative = np.zeros((N, N))
        for j in range(q):
            cumulative = cumulative + sigma_f[j]                          # quirk Q1
            ld, quad, tr = ctx.prior_terms(j, cumulative, mf[j])
            total += -0.5 * ld - 0.5 * (quad + tr)
            for i in range(p):
                ld, quad, tr = ctx.prior_terms(q + j * p + i, sigma_w[j, i], mw[j, i])
                total += -0.5 * ld - 0.5 * (quad + tr)
        return np.float64(total - 0.5 * N * q * (p + 1) * np.log(2.0 * np.pi))

    def _expectedLogLike(self, y, jitt2, sigma_f, mu_f, sigma_w, mu_w):
        """Expected log-likelihood (meanfield.py:895-990; eq. 14).  As in the reference the argument ``y`` is NOT what
        enters: the residual is taken against the raw data ``self.y`` (:940, quirk Q3), and of the covariances only the
        diagonals (:956-957).  Computed by the kernel of the device's own ELBO assembly from the state
        ``(mu_f, mu_w)`` / ``(diag Sigma_f, diag Sigma_w)`` and the jitters."""
        self._refuse_masked('_expectedLogLike')
        q, p, N = self.q, self.p, self.N
        sigma_f = np.asarray(sigma_f, dtype=float).reshape(q, N, N)
        sigma_w = np.asarray(sigma_w, dtype=float).reshape(q, p, N, N)
        mu = np.concatenate((np.reshape(mu_f, (1, q, N)), np.reshape(mu_w, (p, q, N))))
        var = np.empty((p + 1, q, N))
        for j in range(q):
            var[0, j] = np.diag(sigma_f[j])
            for i in range(p):
                var[1 + i, j] = np.diag(sigma_w[j, i])
        ctx = self._backend()
        self._send_elbo_form(ctx, 'reference')             # (the reference's term: raw y, quirk Q3)
        try:
            ctx.set_jitters(np.sqrt(np.asarray(jitt2, dtype=float)))
            ctx.set_muvar(mu, var)
            return np.float64(ctx.expected_loglike())
        finally:
            self._send_elbo_form(ctx)

    def nELBO(self, parameters, max_iter=None):
        """ Negative ELBO at `parameters` (warm-started, meanfield.py:1095-1111) """
        assert self._components_set, _NOT_SET
        self.set_parameters(parameters)
        start = time_module.time()
        elbo, _, _, _ = self.ELBOcalc(self.nodes, self.weights, self.means,
                                      self.jitters, max_iter=max_iter,
                                      mu='previous', var='previous')
        took = 1e3 * (time_module.time() - start)
        print(f'ELBO={elbo:7.2f} (took {took:5.2f} ms)' + 20 * ' ', end='\r', flush=True)
        return -elbo

    def optimize(self, vars=None, **kwargs):
        """
        Maximise the ELBO over the free parameters with scipy.optimize.minimize
        (Nelder-Mead unless `method` is given).  `vars`: 'name' optimises only
        that parameter, '-name' all but it, a list optimises those named.
        ``jac=True`` hands scipy the gradient too (``nELBO_and_grad``; not in the reference, whose optimiser is
        derivative-free).  NOTE that the objective is then a different one: the negative ELBO after a FIXED number of
        forced sweeps (``sweeps=``, default 40) from the state this call starts at, a smooth function of the parameters
        -- ``optimize()`` itself minimises ``nELBO``, the warm-started ELBOcalc under the reference's 1e-3 stop rule,
        which jumps whenever the trip count changes.  The result says so: ``res.objective`` names what ``res.fun`` is,
        and ``res.fun_reference`` is ``nELBO(res.x)``, the reference's objective at the point found.
        ``fused=True`` (with ``jac=True``): the gradient through ``grad_ELBO(fused=True)`` -- one device call per
        evaluation, and the only gradient there is under a data mask (``from_series``).
        With ``elbo='bound'`` everything follows that form, and ``jac=True`` needs no ``fused=`` (the B-form is the only
        one) and no finite differences: the gradient handed to scipy is the fixed-state one, exact at a converged state.
        """
        from scipy.optimize import minimize
        self._select_vars(vars)
        kwargs.setdefault('method', 'Nelder-Mead')
        # jac=True (not in the reference, which is derivative-free): the analytic gradient of grad_ELBO,
        # e.g. optimize(method='L-BFGS-B', jac=True)
        # ... over a SMOOTH objective: the ELBO after a fixed number of forced sweeps (`sweeps=`, default 40) from the
        # state this call starts at -- the reference's own objective (ELBOcalc under its 1e-3 stop rule, warm-started
        # from the previous evaluation) jumps by 1e-3 relative whenever the trip count changes, which a line search
        # cannot work with
        fused = bool(kwargs.pop('fused', self._elbo == 'bound' and kwargs.get('jac') is True))
        if fused and kwargs.get('jac') is not True:
            raise ValueError('optimize(fused=True) chooses the form of the gradient: it needs jac=True')
        if kwargs.get('jac') is True:
            if fused:
                if self._comm is not None:
                    raise NotImplementedError('optimize(jac=True, fused=True) is not available on a sharded inference object')
            else:
                self._refuse_masked('optimize(jac=True)')
            sweeps = int(kwargs.pop('sweeps', 40))
            nodes, weights, means, jitters = self._get_components()
            start = (self._mu, self._var) if self._mu is not None else self._initMuVar(nodes, weights, jitters)
            start = (np.array(start[0], dtype=float), np.array(start[1], dtype=float))
            fun = lambda x: self.nELBO_and_grad(x, sweeps=sweeps, start=start, fused=fused)
        else:
            fun = self.nELBO
        smooth = kwargs.get('jac') is True
        res = minimize(fun, self.get_parameters(), **kwargs)
        self.set_parameters(res.x)
        if smooth:
            res.objective = '-ELBO after %d forced sweeps from the state optimize() started at' % sweeps
            res.fun_reference = self.nELBO(res.x)
        else:
            res.objective = 'nELBO: -ELBO of the warm-started ELBOcalc under the 1e-3 stop rule (meanfield.py:1095-1111)'
            res.fun_reference = res.fun
        return res


    # ------------------------------------------------------------ prediction
    def _kss_diagonal(self, kernel, tstar):
        """diag of ``_tinyNuggetKMatrix(kernel, tstar)`` (what _gp.GP.prediction takes of K**, _gp.py:130-137) without
        forming the n* x n* matrix: point by point through the kernel's own ``__call__`` -- ``kernel(0)`` for the
        one-argument kernels (plus the 1.25e-12 nugget), ``kernel(t, t)`` for the two-argument ones."""
        tstar = np.atleast_1d(np.asarray(tstar, dtype=float))
        if isinstance(kernel, _TWO_ARGUMENT):                  # (no nugget for these: meanfield.py:447-450)
            return np.array([np.ravel(kernel(np.array([[ts]]), np.array([[ts]])))[0] for ts in tstar], dtype=float)
        return np.full(tstar.size, float(np.ravel(kernel(np.zeros((1, 1))))[0])) + _TINY_NUGGET

    def _Prediction(self, nodes=None, weights=None, means=None, jitters=None,
                    tstar=None, mu=None, var=None, separate=False):
        """
        GPRN predictive mean and variance at `tstar` (default: the data times)
        from variational means/variances `mu`, `var` (default: the converged
        ones of the last ELBOcalc, else the `_initMuVar` start point) --
        meanfield.py:1289-1381.  Every latent GP's conditional mean/variance
        (the reference's `_gp.GP.prediction`, one Cholesky + N* solves each) is
        computed on the GPU (`gprn_predict`; on a sharded object by the latent GP's
        owner, every rank receiving all rows); the O(p q N*) combination below is
        the reference's, including the jitter added once per node.

        The variational form (``predict='variational'``; not in the reference): every latent GP's mean and variance are
        those of the posterior the sweeps computed, ``mean* = K* S c`` and ``var* = k** - |X S K*^T e|^2`` from the
        factors a committed sweep leaves on the device (``_variational_sweep``), and the combination is
        ``mean_i + sum_j w_ij f_j`` and ``sum_j [w_ij^2 v_fj + v_wij (v_fj + f_j^2)] + jitter_i^2`` -- the jitter ONCE.
        With `mu`, `var` given, one sweep runs from that state, the prediction is of the state it leaves, and the
        stored state stays as it is.

        Returns (mean (N*, p), variance (N*, p)) and, with `separate`, the
        object array [node means (q, N*), weight means (q*p, N*)].
        """
        nodes, weights, means, jitters = self._get_components(nodes, weights, means, jitters)
        tstar = self.time if tstar is None else np.atleast_1d(np.asarray(tstar, dtype=float))
        if self._predict_form == 'variational':
            ctx = self._variational_sweep(nodes, weights, means, jitters, mu, var)
            gmean, gvar, _ = ctx.predict(tstar)
            return self._combine_prediction(gmean, gvar, means, jitters, tstar, separate, once=True)
        if mu is None and var is None:
            if self._mu is None and self._var is None:
                mu, var = self._initMuVar(nodes, weights, jitters)
            else:
                mu, var = self._mu, self._var

        specs = [self._kernel_spec(k) for k in chain(nodes, weights)]
        ctx = self._backend()
        key = tuple(self._spec_key(sp) for sp in specs)
        if key != self._prior_key:
            for gp, sp in enumerate(specs):
                self._send_spec(ctx, gp, sp)
            self._prior_key = None             # the priors must be refactored before the next sweep
        # a user-defined covFunction has no device form of its cross-covariance: its three matrices are
        # evaluated here, as the reference evaluates every kernel's (_gp.py:40-63, meanfield.py:436-471),
        # and handed over; the factorisation and the solves stay on the GPU (owner rank only when sharded)
        data_t = np.asarray(self.time, dtype=float)
        for gp, (sp, kernel) in enumerate(zip(specs, chain(nodes, weights))):
            if sp[0] != 'host' or ctx.owner_of(gp) != ctx.rank:
                continue
            ctx.predict_upload(gp, self._tinyNuggetKMatrix(kernel, data_t),
                               self._predictKMatrix(kernel, tstar), self._kss_diagonal(kernel, tstar))
        self._send_predict_form(ctx)
        ctx.set_muvar(np.asarray(mu, dtype=float), np.asarray(var, dtype=float))
        gmean, gvar, info = ctx.predict(tstar)
        self.last_info = info
        return self._combine_prediction(gmean, gvar, means, jitters, tstar, separate)

    def _combine_prediction(self, gmean, gvar, means, jitters, tstar, separate, once=False):
        """The O(p q N*) combination of _Prediction (meanfield.py:1346-1373) from the latent rows (G, N*): the jitter once
        per node as the reference has it, or -- `once`, the variational form -- once."""
        q, p = self.q, self.p
        nPred, nVar = gmean[:q], gvar[:q]
        wPred, wVar = gmean[q:], gvar[q:]
        wP, wV = wPred.reshape(q, p, tstar.size), wVar.reshape(q, p, tstar.size)
        meanVal = np.array(np.array_split(self._mean(means, tstar), p))
        jitt2 = np.array(jitters)**2
        predictives = np.zeros((tstar.size, p))
        predictivesVar = np.zeros((tstar.size, p))
        for i in range(p):
            predictives[:, i] += meanVal[i]
            for j in range(q):
                predictives[:, i] += nPred[j] * wP[j, i]
                if once:
                    predictivesVar[:, i] += wP[j, i] * wP[j, i] * nVar[j] + wV[j, i] * (nVar[j] + nPred[j] * nPred[j])
                else:
                    predictivesVar[:, i] += wP[j, i] * wP[j, i] * nVar[j] \
                        + wV[j, i] * (nVar[j] + nPred[j] * nPred[j]) + jitt2[i]
            if once:
                predictivesVar[:, i] += jitt2[i]
        if separate:
            return predictives, predictivesVar, np.array([nPred, wPred], dtype=object)
        return predictives, predictivesVar

    def _variational_sweep(self, nodes, weights, means, jitters, mu=None, var=None):
        """The device state the variational form of prediction reads: the factors of a committed sweep that produced the
        state the prediction is of.  Returns the context, the option ``"predict_form"`` set.

        * No stored state (``self._mu is None``): ``ELBOcalc()`` runs first.
        * The object knows that the device's committed sweep is the one that produced the stored state -- the private
          marker ``ELBOcalc`` / ``nELBO`` / ``grad_ELBO(fused=True)`` leave, stale after ``set_parameters``,
          ``set_components``, a new stored state or a changed component -- and the library's ``"state_ready"`` reads 1:
          NO sweep is run, the stored state is untouched.
        * Otherwise the set-up, ``set_muvar(stored state)`` and one committed sweep, exactly as ``grad_ELBO(fused=True)``
          does; the object keeps the state that sweep leaves and ``last_info`` is set.
        * `mu`, `var` given: one sweep from that state; the stored state is left alone (and the marker dropped: the device
          no longer holds the stored state's sweep).
        A non-positive pivot raises ``np.linalg.LinAlgError``; a user-defined kernel ``NotImplementedError``."""
        self._need_programs("predict='variational'", nodes, weights)
        explicit = mu is not None or var is not None
        if explicit and (mu is None or var is None):
            raise ValueError('_Prediction: give both mu and var, or neither')
        if not explicit:
            if self._mu is None:
                _, mu, var, _ = self.ELBOcalc(nodes, weights, means, jitters)
                if self._mu is not None:                 # (converged: the stored state; else the state the loop ended in)
                    mu, var = self._mu, self._var
            else:
                mu, var = self._mu, self._var
            ctx = self._backend()
            own = nodes is self.nodes and weights is self.weights and means is self.means and jitters is self.jitters
            if own and mu is self._mu and self._is_swept(ctx):
                self._send_predict_form(ctx)
                return ctx
        self._swept = None
        ctx = self._setup_device(nodes, weights, means, jitters)
        self._send_predict_form(ctx)
        ctx.set_muvar(np.array(mu, dtype=float), np.array(var, dtype=float))
        _, _, info = ctx.sweep(1, commit=True)
        self.last_info = info
        if info:
            raise np.linalg.LinAlgError(f'predict: the sweep met a non-positive pivot ({info}) in latent GP '
                                        f'{ctx.last_info_gp}')
        if not explicit:
            self._mu, self._var = ctx.get_muvar()
            self._mark_swept(nodes, weights, means, jitters)
        return ctx

    def _stage_posterior(self, nodes, weights, means, jitters, tstar):
        """What predict_cov / sample_posterior hand the device before their call: the kernels (as _Prediction does), the
        host-evaluated matrices of user-defined kernels -- K + 1.25e-12 I, K*, k** and the whole K** -- the state and the
        jitters.  Returns the context.  The variational form: ``_variational_sweep``'s context (the jitters are the
        sweep's)."""
        if self._predict_form == 'variational':
            return self._variational_sweep(nodes, weights, means, jitters)
        if self._mu is None and self._var is None:
            mu, var = self._initMuVar(nodes, weights, jitters)
        else:
            mu, var = self._mu, self._var
        specs = [self._kernel_spec(k) for k in chain(nodes, weights)]
        ctx = self._backend()                  # (a sharded context refuses the call itself: GPRN_E_UNSUPPORTED)
        key = tuple(self._spec_key(sp) for sp in specs)
        if key != self._prior_key:
            for gp, sp in enumerate(specs):
                self._send_spec(ctx, gp, sp)
            self._prior_key = None             # the priors must be refactored before the next sweep
        data_t = np.asarray(self.time, dtype=float)
        for gp, (sp, kernel) in enumerate(zip(specs, chain(nodes, weights))):
            if sp[0] != 'host':
                continue
            ctx.predict_upload(gp, self._tinyNuggetKMatrix(kernel, data_t),
                               self._predictKMatrix(kernel, tstar), self._kss_diagonal(kernel, tstar))
            ctx.predict_upload_kss(gp, self._tinyNuggetKMatrix(kernel, tstar))
        self._send_predict_form(ctx)
        ctx.set_muvar(np.asarray(mu, dtype=float), np.asarray(var, dtype=float))
        ctx.set_jitters(np.asarray(jitters, dtype=float))
        return ctx

    def predict_cov(self, tstar=None, joint=False, separate=False):
        """
        Full predictive covariance of the GPRN at `tstar` (default: the data times), from the state _Prediction uses.
        Not in the reference: its _gp.GP.prediction forms every latent GP's conditional covariance
        C_g = K** - K* (K + 1.25e-12 I + diag v)^-1 K*^T (_gp.py:125-137) and keeps only the diagonal.  Here the
        matrices stay, on the GPU (gprn_predict_cov), and are combined per output under the mean-field independence of
        the latent GPs:

            Cov(y_i(t), y_i(t')) = sum_j [w_ij w_ij' C_fj + C_wij (C_fj + f_j f_j')] + q jitter_i^2 delta(t, t')
            Cov(y_i(t), y_k(t')) = sum_j w_ij w_kj' C_fj(t, t')                    (i != k, `joint` only)

        whose diagonal is _Prediction's variance, quirk included (jitter_i^2 added once per node).

        The variational form (``predict='variational'``): C_g = K** - W W^T of the posterior the sweeps computed
        (``_variational_sweep``: no sweep where the device still holds the stored state's), the set-up's nugget as
        delta(t, t') -- between equal times of `tstar` too -- and ``jitter_i^2 delta(t, t')`` once instead of q times.
        At the data times the latent matrices are the Sigma_g of the stored state.

        Returns (mean (N*, p), cov): cov (p, N*, N*), or (p N*, p N*) with `joint` (row i N* + t); with `separate` also
        the node covariances (q, N*, N*) and the weight covariances (q p, N*, N*), weight (j, i) at j p + i.
        """
        nodes, weights, means, jitters = self._get_components()
        tstar = self.time if tstar is None else np.atleast_1d(np.asarray(tstar, dtype=float))
        ctx = self._stage_posterior(nodes, weights, means, jitters, tstar)
        gmean, lat, cov = ctx.predict_cov(tstar, joint=joint, latent=separate)
        q, p = self.q, self.p
        nPred, wP = gmean[:q], gmean[q:].reshape(q, p, tstar.size)
        meanVal = np.array(np.array_split(self._mean(means, tstar), p))
        predictives = np.zeros((tstar.size, p))
        for i in range(p):                     # (as _Prediction)
            predictives[:, i] += meanVal[i]
            for j in range(q):
                predictives[:, i] += nPred[j] * wP[j, i]
        if separate:
            return predictives, cov, lat[:q], lat[q:]
        return predictives, cov

    def sample_posterior(self, tstar=None, n=1, noise=False, separate=False, rng=None):
        """
        `n` joint draws of the GPRN's predictive distribution at `tstar` (default: the data times).  Not in the
        reference.  Every latent GP is drawn from N(mean_g, C_g) (predict_cov's C_g) as mean_g + L_g z, with
        C_g + nu_g I = L_g L_g^T factored on the GPU (gprn_predict_draws); nu_g starts at 1.25e-12 and grows by factors
        of 100, to 1.25e-6 at most, while fp64 finds the matrix not positive definite (the ladder of _sample_from_gp; the
        values used are left in ``self.last_nuggets``).  Output i is mean function_i + sum_j w_ij o f_j, and with `noise`
        also N(0, q jitter_i^2) per time (q: _Prediction's jitter counted once per node).  The first two moments of the
        draws are _Prediction's mean and variance.  The standard normals come from ``np.random.default_rng(rng)``.
        The variational form (``predict='variational'``): predict_cov's C_g of that form, and `noise` is N(0, jitter_i^2).

        Returns draws (n, N*, p); with `separate` also the node draws (q, n, N*) and weight draws (q p, n, N*).
        """
        nodes, weights, means, jitters = self._get_components()
        tstar = self.time if tstar is None else np.atleast_1d(np.asarray(tstar, dtype=float))
        gen = np.random.default_rng(rng)
        ctx = self._stage_posterior(nodes, weights, means, jitters, tstar)
        q, p, ns = self.q, self.p, tstar.size
        z = gen.standard_normal((q * (p + 1), int(n), ns))
        lat, out, nug, info = ctx.predict_draws(tstar, z)
        self.last_nuggets = nug
        if info:
            raise np.linalg.LinAlgError(f'predictive covariance of latent GP {ctx.last_info_gp} is not positive definite '
                                        f'even with a 1.25e-6 nugget (pivot {info})')
        meanVal = np.array(np.array_split(self._mean(means, tstar), p))
        draws = np.transpose(out, (1, 2, 0)) + meanVal.T[None]
        if noise:
            once = self._predict_form == 'variational'
            sd = (1.0 if once else np.sqrt(q)) * np.abs(np.asarray(jitters, dtype=float))
            draws = draws + gen.standard_normal(draws.shape) * sd
        if separate:
            return draws, lat[:q], lat[q:]
        return draws

    def predict(self, tstar=None, nn=1000):
        """
        GPRN prediction at `tstar`, or on `nn` points spanning the data padded by
        20 % on each side (meanfield.py:1383-1400).  Returns (tstar, mean,
        standard deviation, [node means, weight means]).  What is predicted follows ``predict_form`` (``_Prediction``).
        """
        if tstar is None:
            lo, hi = self.time.min(), self.time.max()
            span = np.ptp(self.time)
            tstar = np.linspace(lo - 0.2 * span, hi + 0.2 * span, nn)
        mean, variance, parts = self._Prediction(tstar=tstar, separate=True)
        return tstar, mean, np.sqrt(variance), parts

    #: largest N for which nELBO_batch / mcmc(batch=True) evaluate side by side on one GPU (beyond it a single evaluation
    #: already fills the device, and a chunk of evaluations would be a few matrices)
    batch_max_N = 2048
    _batch_last_done = -1            # position (in the last side-by-side list) of the evaluation whose state was kept

    def nELBO_batch(self, parameter_sets, max_iter=None, pool=None, batch=True):
        """
        ``nELBO`` for several free-parameter vectors: ``[nELBO(p) for p in
        parameter_sets]``.  With ``pool`` (``sharding.EvalPool``; every rank holds
        this same problem on its own GPU) the vectors are split over the ranks and
        every rank returns the full list.  Not in the reference, which evaluates
        optimiser populations and emcee walkers one by one (meanfield.py:1222-1260).
        The parameters of ``self`` end up at the last vector this rank evaluated.  With a pool AND the side-by-side form
        below, each rank evaluates its share side by side and the state every rank keeps is the same (that of the last
        evaluation of the whole list that converged): the values do not depend on the number of ranks.

        Without a pool, a problem whose kernels all have device programs evaluates the whole list SIDE BY SIDE on the GPU
        (``gprn_elbocalc_batch``): every evaluation with its own covariance matrices, state, loop and stop rule, all of
        them starting from the state the object holds (``nELBO``'s warm start) -- where one evaluation after the other
        starts each from its predecessor's result, which moves the values within the stop rule's 1e-3.  One-tile problems
        (N <= 128) run a half-sweep of all evaluations as ONE launch; larger ones (up to ``batch_max_N`` points) go
        through the large problems' launch schedule with its batch dimension = evaluations x latent GPs, in chunks that
        fit the library's memory budget.  ``batch=False`` forces the one-by-one form.
        """
        assert self._components_set, _NOT_SET
        sets = [np.array(x, dtype=float) for x in parameter_sets]
        if pool is None and batch and len(sets) > 1:
            out = self._nELBO_batch_device(sets, max_iter)
            if out is not None:
                return out
        if pool is not None and batch and sets and hasattr(pool, 'map_lists') and self._batchable():
            return self._nELBO_batch_pool(sets, max_iter, pool)
        f = lambda x: float(self.nELBO(x, max_iter=max_iter))
        return list(map(f, sets)) if pool is None else pool.map(f, sets)

    def _batchable(self):
        """Whether ``_nELBO_batch_device`` applies to this object at its current components -- a property of the problem,
        the same on every rank of a pool (so that all of them take the same branch, collectives included)."""
        if self._comm is not None or self.N > self.batch_max_N or self._mask_bars_batch():
            return False
        nodes, weights, _, _ = self._get_components()
        return all(self._kernel_spec(k)[0] == 'device' for k in chain(nodes, weights))

    def _mask_bars_batch(self):
        """A data mask keeps the side-by-side forms away unless ``batch_under_mask`` is set."""
        return self.mask is not None and not self.batch_under_mask

    def _nELBO_batch_pool(self, sets, max_iter, pool):
        """``nELBO_batch`` over the GPUs of a node: rank r evaluates ``sets[r::world]`` SIDE BY SIDE on its own GPU, all
        of them from the state the object holds on entry -- the same on every rank, because the state it holds on exit
        is again the same on every rank: that of the last evaluation OF THE WHOLE LIST whose loop converged
        (``nELBO_batch``'s rule), handed round by its owner.  The values therefore do not depend on the number of
        ranks (to the rounding of a batch's size-dependent launch shapes)."""
        n = len(sets)
        mine = list(range(pool.rank, n, pool.world))
        last = {'key': -1}

        def share(xs):
            out = self._nELBO_batch_device(xs, max_iter)
            if out is None:                                    # (vectors that change a kernel expression's shape)
                # one by one: the state to hand round is that of the last evaluation whose loop CONVERGED -- ELBOcalc
                # stores a state only then (a new array object) -- and only such a state is offered: with nothing stored
                # the ranks would meet in the collective with buffers of different sizes
                out = []
                for i, x in enumerate(xs):
                    before = self._mu
                    out.append(float(self.nELBO(x, max_iter=max_iter)))
                    if self._mu is not None and self._mu is not before:
                        last['key'] = mine[i]
            elif self._batch_last_done >= 0:
                last['key'] = mine[self._batch_last_done]
            return out

        mu0, var0 = self._mu, self._var
        vals = pool.map_lists(share, sets)
        shape = (self.p + 1, self.q, self.N)
        offer = [np.reshape(self._mu, shape), np.reshape(self._var, shape)] if last['key'] >= 0 else [np.zeros(shape), np.zeros(shape)]
        got = pool.take_from_highest(last['key'], offer)
        if got is not None:
            self._mu, self._var = got
        else:
            self._mu, self._var = mu0, var0
        self.set_parameters(sets[-1])
        return vals

    def _nELBO_batch_device(self, sets, max_iter):
        """``nELBO_batch`` through ``gprn_elbocalc_batch``, or None where that does not apply (larger problems, sharded
        objects, user-defined kernels, kernel expressions that change shape from one vector to the next, a data mask without
        ``batch_under_mask``)."""
        start = time_module.time()
        res = self._batch_run(sets, max_iter)
        if res is None:
            return None
        took = 1e3 * (time_module.time() - start)
        print(f'{len(sets)} ELBO evaluations side by side (took {took:5.2f} ms)' + 20 * ' ', end='\r', flush=True)
        return [float(-e) for e in res[0]]

    def _batch_run(self, sets, max_iter):
        """Stage, run every vector's loop side by side under the stop rule, keep (``_batch_keep``): what
        ``Context.elbocalc_batch(want_state=True)`` returned, or None where the side-by-side form does not apply."""
        staged = self._batch_stage(sets)
        if staged is None:
            return None
        ctx, kp, yr, jt, m0, v0 = staged
        res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, _max_trips(max_iter), want_state=True)
        return None if res is None else self._batch_keep(res)

    def _batch_keep(self, res):
        """What a side-by-side call leaves with the object: ``last_info``, and as the warm start of whatever comes next the
        state of the last evaluation whose loop converged (meanfield.py:644-646).  Returns ``res``."""
        info, conv, mu_f, var_f = res[3], res[2], res[4], res[5]
        self.last_info = _first_verdict(info)
        done = np.flatnonzero(conv)
        self._batch_last_done = int(done[-1]) if done.size else -1
        if done.size:
            self._mu, self._var = mu_f[done[-1]], var_f[done[-1]]
        return res

    def _full_vectors(self, sets):
        """``(full (B, n_all), n_k, n_m)``: every vector of `sets` as a full parameter vector (nodes, weights, means,
        jitters: meanfield.py:193-202) -- a free-length vector over the object's frozen values, a full-length one
        contributing its free entries, as ``set_parameters`` reads them (meanfield.py:223-259) -- with the columns where
        the mean parameters begin and how many they are.  None where a vector is neither length (the one-by-one forms
        raise the reference's ValueError)."""
        free = ~self.frozen_mask
        n_free, n_all = int(free.sum()), int(free.size)
        if any(x.ndim != 1 or x.size not in (n_free, n_all) for x in sets):
            return None
        if n_free != n_all and any(x.size == n_all for x in sets):
            sets = [x[free] if x.size == n_all else x for x in sets]
        full = np.tile(self.get_parameters(include_frozen=True), (len(sets), 1))
        full[:, free] = np.array(sets)
        n_k = sum(k.pars.size for k in chain(self.nodes, self.weights))
        return full, n_k, n_all - n_k - self.p

    def _need_programs(self, what, nodes, weights):
        for k in chain(nodes, weights):
            if not isinstance(k, covfunc.covFunction) or k._device_program() is None:
                raise NotImplementedError(f'{what} needs a device program for every kernel: user-defined kernels (and sums '
                                          'that hold a two-argument kernel) are not supported')

    def _scan_programs(self, ctx, shape_ref=None):
        """One vector's step of the scan both stagings make: ``(components, specs, shape)`` at the object's current
        parameters -- or None where a kernel has no device program, or the programs' shape is not `shape_ref`, the first
        vector's.  The first vector (no `shape_ref`) sends the programs the library substitutes the parameters into."""
        components = self._get_components()
        specs = [self._kernel_spec(k) for k in chain(components[0], components[1])]
        if any(sp[0] != 'device' for sp in specs):
            return None
        shape = tuple((sp[1], sp[3]) for sp in specs)
        if shape_ref is None:
            for gp, sp in enumerate(specs):
                self._send_spec(ctx, gp, sp)
            self._prior_key = None                             # (the object's own factors are stale now)
        elif shape != shape_ref:
            return None
        return components, specs, shape

    def _batch_stage(self, sets, start=None, own_masks=False):
        """The B problems of a side-by-side call laid out for ``Context.elbocalc_batch``: ``(ctx, kernel_params (B, n_kpar),
        y_resid (B, p N), jitters (B, p), mu (B, d), var (B, d))``, every evaluation starting from ``start`` = ``(mu, var)``,
        else the stored state, else ``_initMuVar`` of its own parameters -- or None where the side-by-side form does not
        apply.  The kernel programs go to the device; the object's parameters end at the last vector.  ``own_masks``: the
        call brings a fit mask per evaluation (``heldout_batch``), so a data mask does not bar it."""
        if self._comm is not None or self.N > self.batch_max_N or (self._mask_bars_batch() and not own_masks):
            return None
        ctx = self._backend()
        ctx.option('batch_mask', 1 if self.batch_under_mask else 0)   # (every call: the attribute may have changed)
        ctx.option('grad_exact', 1 if self.exact_derivatives else 0)
        self._send_order_mask(ctx)
        self._send_elbo_form(ctx)
        y_raw = np.concatenate(self.y)
        B = len(sets)
        state = (self._mu, self._var) if start is None else (np.asarray(start[0], dtype=float), np.asarray(start[1], dtype=float))
        laid = self._full_vectors(sets)
        if laid is None:
            return None
        full, n_k, n_m = laid
        # the first vector the ordinary way: it tells what the programs are and whether the rest can be laid out in one go
        self.set_parameters(full[0, ~self.frozen_mask])
        scanned = self._scan_programs(ctx)
        if scanned is None:
            return None
        (nodes, weights, means, jitters), specs, shape_ref = scanned
        kernels = list(chain(nodes, weights))
        plain_kernels = all(sp[2].size == k.pars.size and np.array_equal(sp[2], k.pars) for sp, k in zip(specs, kernels))
        plain_means = all(m_ is None or type(m_) is meanfunc.Constant for m_ in means)
        programs = None if plain_means else self._mean_programs(means)
        if plain_kernels and (plain_means or programs is not None) and state[0] is not None:
            # every program's parameters ARE its kernel's and the start is the stored state: the kernel, mean and jitter
            # columns of the B problems are slices of the B full parameter vectors
            kp, jt = full[:, :n_k], full[:, n_k + n_m:]
            if programs is not None:
                # (``device_means``: every mean has a device program, and y - mean of all B vectors is formed on the device
                # inside the batch call -- gprn_elbocalc_batch_means: `yr` carries the mean columns, not an array)
                for i, (ops, par) in enumerate(programs):
                    ctx.set_mean(i, ops, par)
                yr = _hip.MeanParams(full[:, n_k:n_k + n_m], y_raw, want_mean_grad=self._elbo == 'bound')
            else:                                              # (the means are constants: a column each)
                yr = np.tile(y_raw, (B, 1))
                col = n_k
                for i, m_ in enumerate(means):
                    if m_ is not None:
                        yr[:, i * self.N:(i + 1) * self.N] -= full[:, col:col + 1]
                        col += 1
            m0 = np.tile(np.ravel(state[0]), (B, 1))
            v0 = np.tile(np.ravel(state[1]), (B, 1))
            self.set_parameters(full[-1, ~self.frozen_mask])
        else:
            kp, yr, jt, m0, v0 = [], [], [], [], []
            for i in range(B):
                if i:
                    self.set_parameters(full[i, ~self.frozen_mask])
                    scanned = self._scan_programs(ctx, shape_ref)
                    if scanned is None:
                        return None
                    (nodes, weights, means, jitters), specs, _ = scanned
                kp.append(np.concatenate([sp[2] for sp in specs]))
                yr.append(y_raw - self._mean(means))
                jt.append(np.asarray(jitters, dtype=float))
                if state[0] is not None:
                    mu, var = state
                else:
                    mu, var = self._initMuVar(nodes, weights, jitters)
                m0.append(np.ravel(mu))
                v0.append(np.ravel(var))
        return ctx, np.array(kp), yr if isinstance(yr, _hip.MeanParams) else np.array(yr), np.array(jt), np.array(m0), np.array(v0)

    # ------------------------------------------------ prediction for many vectors
    def _predict_stage(self, sets, tstar):
        """The B problems of a side-by-side prediction laid out for ``Context.predict_batch``: ``(ctx, kernel_params (B,
        n_kpar), jitters (B, p), mean functions at tstar (B, p, n*))`` -- or None where the side-by-side form does not
        apply (a sharded object, N > ``batch_max_N``, a kernel without a device program, expressions that change shape from
        one vector to the next).  A data mask is no obstacle: prediction reads only the state.  The kernel programs go to
        the device; the object's parameters end at the last vector."""
        if self._comm is not None or self.N > self.batch_max_N:
            return None
        n_free, n_all = int((~self.frozen_mask).sum()), int(self.frozen_mask.size)
        if any(x.ndim != 1 or x.size not in (n_free, n_all) for x in sets):
            return None                                        # (the one-by-one form raises the reference's ValueError)
        ctx = self._backend()
        kp, jt, mv = [], [], []
        shape_ref = None
        for x in sets:
            self.set_parameters(x)
            scanned = self._scan_programs(ctx, shape_ref)
            if scanned is None:
                return None
            (_, _, means, jitters), specs, shape_ref = scanned
            kp.append(np.concatenate([sp[2] for sp in specs]))
            jt.append(np.asarray(jitters, dtype=float))
            mv.append(np.array(np.array_split(self._mean(means, tstar), self.p)))
        return ctx, np.array(kp), np.array(jt), np.array(mv)

    def _final_states(self, sets, max_iter):
        """Each vector's ``ELBOcalc`` loop as ``nELBO_batch`` runs it -- side by side from the state the object holds where
        ``_batchable()`` holds, else one after the other, each warm-started by its predecessor -- and the state each loop
        ended in: ``(mu (B, p+1, q, N), var)``.  The object keeps what ``nELBO_batch`` would keep."""
        res = self._batch_run(sets, max_iter) if len(sets) > 1 and self._batchable() else None
        if res is not None:
            return res[4], res[5]
        mus, vars_ = [], []
        for x in sets:
            self.set_parameters(x)
            _, mu, var, _ = self.ELBOcalc(self.nodes, self.weights, self.means, self.jitters, max_iter=max_iter,
                                          mu='previous', var='previous')
            mus.append(mu)
            vars_.append(var)
        return np.array(mus), np.array(vars_)

    def _times(self, what, tstar):
        """`tstar` as a non-empty vector of times, the data's by default."""
        tstar = np.asarray(self.time, dtype=float) if tstar is None else np.atleast_1d(np.asarray(tstar, dtype=float))
        if tstar.ndim != 1 or tstar.size < 1:
            raise ValueError(f'{what}: tstar must be a non-empty vector of times')
        return tstar

    def _batch_request(self, what, parameter_sets, max_iter, sweeps, start, no_trips, tstar=False, start_needs_sweeps=True,
                       empty_ok=False):
        """The arguments the side-by-side methods share, read before anything touches a device: ``(sets, forced, trips,
        tstar)`` -- the vectors as float arrays; whether ``sweeps`` forces the number of sweeps, and the trips either way
        (``sweeps``, else ``max_iter`` with ELBOcalc's default); `tstar` through ``_times`` (``False``: the method takes no
        times).  `what` names the method in the messages; `no_trips` is its message for fewer than one trip."""
        assert self._components_set, _NOT_SET
        sets = [np.array(x, dtype=float) for x in parameter_sets]
        if not sets and not empty_ok:
            raise ValueError(f'{what}: no parameter vector')
        forced = sweeps is not None
        if start_needs_sweeps and start is not None and not forced:
            raise ValueError(f'{what}: `start` goes with `sweeps`; the loop under the stop rule starts from the state the '
                             'object holds')
        trips = int(sweeps) if forced else _max_trips(max_iter)
        if trips < 1:
            raise ValueError(no_trips)
        return sets, forced, trips, tstar if tstar is False else self._times(what, tstar)

    def _one_by_one(self, sets, entry, forced, trips, each, variational, chain_info):
        """The one-by-one form of a side-by-side call.  Every vector starts from `entry` = ``(mu, var)`` -- ``(None, None)``:
        from ``_initMuVar`` of its own parameters -- and runs the set-up, then `trips` forced committed sweeps or the loop
        under the stop rule, `trips` at most; then ``each(b, ctx, components, info, history, mu, var)`` makes the vector's
        payload from what that left and returns ``(payload, failed)``, `failed` the verdict that bars keeping the state
        (the loop's `info`, or what the payload's own factorisation found).  Returns the payloads.  The object keeps the
        state of the last vector whose loop converged and did not fail.

        `variational`: the payload predicts from the posterior the sweeps leave -- a kernel without a device program is
        refused as ``predict='variational'`` refuses it, the marker of the stored state's sweep is dropped (the set-up
        drops it only where it sends kernels) and the predict form is sent.
        `chain_info`: ``last_info`` is carried from vector to vector, ``info or last_info`` with what the object held on entry
        and what each set-up left, and `each` is handed that; else ``last_info`` is this call's first positive `failed`."""
        payloads, keep, first = [], None, 0
        for b, x in enumerate(sets):
            self.set_parameters(x)
            components = nodes, weights, means, jitters = self._get_components()
            if variational:
                self._need_programs("predict='variational'", nodes, weights)
            mu0, var0 = entry if entry[0] is not None else self._initMuVar(nodes, weights, jitters)
            ctx = self._setup_device(nodes, weights, means, jitters)
            if variational:
                self._swept = None                             # (the device's committed sweep is no stored state's)
                self._send_predict_form(ctx)
            ctx.set_muvar(np.asarray(mu0, dtype=float), np.asarray(var0, dtype=float))
            if forced:
                history, _, info = ctx.sweep(trips, commit=True)
                conv = False
                mu, var = ctx.get_muvar()
            else:
                history, _, conv, info, mu, var = ctx.elbocalc(trips)
            if chain_info:
                info = self.last_info = info or self.last_info
            payload, failed = each(b, ctx, components, info, history, mu, var)
            payloads.append(payload)
            first = first or int(failed)
            if conv and not failed:
                keep = (mu, var)
        if not chain_info:
            self.last_info = first
        if keep is not None:
            self._mu, self._var = keep
        return payloads

    def predict_batch(self, parameter_sets, tstar=None, states=None, max_iter=None, separate=False, from_sweeps=False,
                      sweeps=None, start=None):
        """
        ``_Prediction`` for several free-parameter vectors -- the step that follows an ``mcmc`` run, whose posterior
        predictive averages the prediction over the hyper-parameter vectors the chain kept (the reference calls
        ``_Prediction`` once per vector, meanfield.py:1289-1381).  Not in the reference.

        ``states = (mu (B, ...), var (B, ...))`` predicts vector b from state b.  ``states=None`` first runs each vector's
        ``ELBOcalc`` loop exactly as ``nELBO_batch`` does (same shared warm start, same state and parameters kept by the
        object afterwards; side by side where that applies, else one by one) and predicts from each loop's final state.

        Where every kernel has a device program the B predictions run SIDE BY SIDE on the GPU (``gprn_predict_batch``):
        every latent GP of every vector is filled, factored and solved in the same launches, the times ``tstar`` going in
        blocks, and the per-output combination is formed on the device too.  A data mask is no obstacle.  Otherwise --
        user-defined kernels, expressions that change shape between vectors, a sharded object, N > ``batch_max_N`` -- one
        ``_Prediction`` per vector, same return value.  Mean functions are evaluated per vector on the host.

        ``from_sweeps=False`` (the default) is always the reference form of prediction: with ``predict='variational'`` it
        raises ``NotImplementedError``.

        ``from_sweeps=True`` (``predict='variational'`` only, else ``ValueError``): each vector's loop runs and the vector is
        predicted from the posterior ``q(f_g) = N(mu_g, Sigma_g)`` THAT loop leaves -- ``_Prediction``'s variational form
        per vector, the jitter once -- all vectors SIDE BY SIDE (``gprn_elbocalc_batch_predict``: a prediction pass at the
        end of each batch chunk, from the X, s and c every evaluation's last committed sweep left in the chunk's slabs).
        ``states`` is a ``ValueError`` (a state carries no X).  ``sweeps=n`` / ``start=(mu, var)`` mean what they mean in
        ``nELBO_and_grad_batch``: exactly n forced sweeps per vector from ``start``, else the stored state, else
        ``_initMuVar``; without ``sweeps`` the warm-started loop under the stop rule (``start`` without ``sweeps`` and
        ``sweeps < 1`` are ``ValueError``).  The object keeps what ``nELBO_batch`` keeps.  Where the side-by-side form does
        not apply (N > ``batch_max_N``, a mask without ``batch_under_mask``, expressions that change shape between
        vectors) the vectors go one by one with the same meaning: the loop (or n forced sweeps from the same start), then
        the posterior form of ``gprn_predict`` on what it left; a kernel without a device program raises what
        ``predict='variational'`` raises for it.  A vector whose factorisation meets a non-positive pivot gets NaN rows.
        Sharded objects: ``NotImplementedError``.

        Returns (mean (B, N*, p), variance (B, N*, p)) and, with `separate`, the latent means (B, G, N*): nodes first,
        then weight (j, i) at q + j p + i.
        """
        if from_sweeps:
            return self._predict_batch_from_sweeps(parameter_sets, tstar, states, max_iter, separate, sweeps, start)
        if sweeps is not None or start is not None:
            raise ValueError('predict_batch: `sweeps` and `start` go with from_sweeps=True')
        self._refuse_variational_batch('predict_batch')
        assert self._components_set, _NOT_SET
        sets = [np.array(x, dtype=float) for x in parameter_sets]
        B = len(sets)
        if B < 1:
            raise ValueError('predict_batch: no parameter vector')
        tstar = self._times('predict_batch', tstar)
        d = (self.p + 1) * self.q * self.N
        if states is None:
            states = self._final_states(sets, max_iter)
        try:
            mu_b, var_b = (np.asarray(a, dtype=float) for a in states)
        except (TypeError, ValueError) as exc:
            raise ValueError('predict_batch: states must be the pair (mu, var)') from exc
        if mu_b.size != B * d or var_b.size != B * d or mu_b.shape[0] != B or var_b.shape[0] != B:
            raise ValueError(f'predict_batch: states must be two arrays of {B} states of {d} values, got {mu_b.shape} and '
                             f'{var_b.shape}')
        mu_b, var_b = mu_b.reshape(B, d), var_b.reshape(B, d)
        staged = self._predict_stage(sets, tstar)
        res = None
        if staged is not None:
            ctx, kp, jt, meanvals = staged
            res = ctx.predict_batch(kp, mu_b, var_b, tstar, jitters=jt, latent=separate, outputs=True)
        if res is not None:
            lat_mean, _, out_mean, out_var, info = res
            self.last_info = _first_verdict(info)
            mean = np.transpose(out_mean + meanvals, (0, 2, 1))
            var = np.transpose(out_var, (0, 2, 1))
            return (mean, var, lat_mean) if separate else (mean, var)
        # one by one
        shape = (self.p + 1, self.q, self.N)
        means_, vars_, lats = [], [], []
        for b, x in enumerate(sets):
            self.set_parameters(x)
            m_, v_, parts = self._Prediction(tstar=tstar, mu=mu_b[b].reshape(shape), var=var_b[b].reshape(shape), separate=True)
            means_.append(m_)
            vars_.append(v_)
            lats.append(np.concatenate([np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)]))
        mean, var = np.array(means_), np.array(vars_)
        return (mean, var, np.array(lats)) if separate else (mean, var)

    def _predict_batch_from_sweeps(self, parameter_sets, tstar, states, max_iter, separate, sweeps, start):
        """``predict_batch(from_sweeps=True)``: see there."""
        if self._predict_form != 'variational':
            raise ValueError("predict_batch: from_sweeps=True predicts from the posterior the sweeps leave; it needs "
                             "predict='variational' (predict_form)")
        if states is not None:
            raise ValueError('predict_batch: from_sweeps=True takes no `states` -- a state carries no X; give `sweeps` and '
                             '`start` to run forced sweeps from a state of your own')
        if self._comm is not None:
            raise NotImplementedError('predict_batch(from_sweeps=True) is not available on a sharded inference object')
        sets, forced, trips, tstar = self._batch_request(
            'predict_batch', parameter_sets, max_iter, sweeps, start, tstar=tstar,
            no_trips='predict_batch: from_sweeps=True needs at least one committed sweep')
        staged = self._batch_stage(sets, start=start)
        res = None
        if staged is not None:
            ctx, kp, yr, jt, m0, v0 = staged
            res = ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, trips, tstar, forced=forced, latent=separate, outputs=True)
        if res is not None:
            self._batch_keep(res)
            lat_mean, out_mean, out_var = res[6], res[8], res[9]
            mean = np.transpose(out_mean + self._mean_values_batch(sets, tstar), (0, 2, 1))
            var = np.transpose(out_var, (0, 2, 1))
            return (mean, var, lat_mean) if separate else (mean, var)

        def predict(b, ctx, components, info, history, mu, var):
            _, _, means, jitters = components
            if info:
                gmean = gvar = np.full((self.q * (self.p + 1), tstar.size), np.nan)
            else:
                gmean, gvar, _ = ctx.predict(tstar)
            m_, v_, parts = self._combine_prediction(gmean, gvar, means, jitters, tstar, True, once=True)
            return (m_, v_, np.concatenate([np.asarray(parts[0], dtype=float), np.asarray(parts[1], dtype=float)])), info

        entry = (self._mu, self._var) if start is None else start
        means_, vars_, lats = zip(*self._one_by_one(sets, entry, forced, trips, predict, variational=True, chain_info=False))
        mean, var = np.array(means_), np.array(vars_)
        return (mean, var, np.array(lats)) if separate else (mean, var)

    def sample_posterior_batch(self, parameter_sets, tstar=None, n=1, noise=False, separate=False, rng=None, max_iter=None,
                               sweeps=None, start=None):
        """
        ``sample_posterior`` for several free-parameter vectors -- one joint curve (or `n`) per vector an ``mcmc`` run kept,
        smooth in `tstar`: each vector's loop runs and the vector is drawn from the posterior ``q(f_g) = N(mu_g, Sigma_g)``
        THAT loop leaves, all vectors SIDE BY SIDE (``gprn_elbocalc_batch_draws``: a draw pass at the end of each batch
        chunk, from the X, s and c every evaluation's last committed sweep left in the chunk's slabs).  Not in the reference.

        It needs ``predict='variational'`` (else ``ValueError``), as ``predict_batch(from_sweeps=True)`` does, and
        ``max_iter`` / ``sweeps`` / ``start`` mean what they mean there.  The standard normals ``(B, G, n, N*)`` are drawn up
        front from ``np.random.default_rng(rng)``; where the side-by-side form does not apply (N > ``batch_max_N``, a mask
        without ``batch_under_mask``, expressions that change shape between vectors) the vectors go one by one with the
        same numbers and the same meaning: the loop, then ``gprn_predict_draws`` in the posterior form on what it left.
        Every latent GP of every vector has its own nugget from the ladder 1.25e-12 x 100^k <= 1.25e-6
        (``self.last_nuggets``, (B, G)).  The mean functions are added per vector (on the device with ``device_means``), and
        with `noise` also N(0, jitter_i^2) per time, once, from each vector's own jitters, drawn after the normals from the
        same generator.  A vector whose factorisation meets a non-positive pivot -- in its sweeps or on the ladder's last
        rung -- gets NaN rows; ``last_info`` holds the first positive verdict.  The object keeps what ``nELBO_batch`` keeps.
        Sharded objects: ``NotImplementedError``.

        Returns draws (B, n, N*, p); with `separate` also the latent draws (B, G, n, N*): nodes first, then weight (j, i)
        at q + j p + i.
        """
        if self._predict_form != 'variational':
            raise ValueError("sample_posterior_batch draws from the posterior the sweeps leave; it needs "
                             "predict='variational' (predict_form)")
        n = int(n)
        if n < 1:
            raise ValueError('sample_posterior_batch: n >= 1 draws per vector expected')
        if self._comm is not None:
            raise NotImplementedError('sample_posterior_batch is not available on a sharded inference object')
        sets, forced, trips, tstar = self._batch_request(
            'sample_posterior_batch', parameter_sets, max_iter, sweeps, start, tstar=tstar,
            no_trips='sample_posterior_batch needs at least one committed sweep')
        B = len(sets)
        q, p, ns = self.q, self.p, tstar.size
        G = q * (p + 1)
        gen = np.random.default_rng(rng)
        z = gen.standard_normal((B, G, n, ns))
        staged = self._batch_stage(sets, start=start)
        res = None
        if staged is not None:
            ctx, kp, yr, jt, m0, v0 = staged
            res = ctx.elbocalc_batch_draws(kp, yr, jt, m0, v0, trips, tstar, z, forced=forced, latent=separate, outputs=True)
        if res is not None:
            self._batch_keep(res)
            lat, out, nug, dinfo = res[6], res[7], res[8], res[9]
            if not self.last_info and np.any(dinfo):
                self.last_info = _first_verdict(dinfo)
            jit_b = np.asarray(jt, dtype=float).reshape(B, p)
        else:
            # one by one, each vector from the same state and its own slice of the normals
            def draw(b, ctx, components, info, history, mu, var):
                lat_b, out_b, nug_b = np.full((G, n, ns), np.nan), np.full((p, n, ns), np.nan), np.full(G, np.nan)
                if not info:
                    l_, o_, nug_b, info = ctx.predict_draws(tstar, z[b])
                    if not info:
                        lat_b, out_b = l_, o_
                return (lat_b, out_b, nug_b, np.asarray(components[3], dtype=float)), info

            entry = (self._mu, self._var) if start is None else start
            lats, outs, nugs, jits = zip(*self._one_by_one(sets, entry, forced, trips, draw, variational=True, chain_info=False))
            lat, out, nug, jit_b = np.array(lats), np.array(outs), np.array(nugs), np.array(jits).reshape(B, p)
        self.last_nuggets = nug
        meanvals = self._mean_values_batch(sets, tstar)                         # (B, p, N*)
        draws = np.transpose(out, (0, 2, 3, 1)) + np.transpose(meanvals, (0, 2, 1))[:, None]
        if noise:
            draws = draws + gen.standard_normal(draws.shape) * np.abs(jit_b)[:, None, None, :]
        return (draws, lat) if separate else draws

    def _mean_programs(self, means):
        """[(ops, params)] per output -- the empty program for a mean that is None -- where ``device_means`` is on and
        every mean has a device program; else None: the caller evaluates on the host as it always has."""
        if not self.device_means or self._comm is not None:
            return None
        programs = []
        for m_ in means:
            pg = ([], np.zeros(0)) if m_ is None else \
                m_._device_program() if isinstance(m_, meanfunc.meanFunction) else None
            if pg is None:
                return None
            programs.append(pg)
        return programs

    def _mean_values_batch(self, sets, tstar):
        """The mean functions at `tstar` for B vectors, each at its own parameters: ``(B, p, n*)``.  Constant (or no) means
        are read from the vectors' own columns (nodes, weights, means, jitters: meanfield.py:193-202); anything else is
        evaluated per vector.  The object's parameters end at the last vector."""
        means = self._get_components()[2]
        laid = self._full_vectors(sets)
        if laid is not None and all(m_ is None or type(m_) is meanfunc.Constant for m_ in means):
            full, col, _ = laid
            out = np.zeros((len(sets), self.p, tstar.size))
            for i, m_ in enumerate(means):
                if m_ is not None:
                    out[:, i, :] = full[:, col:col + 1]
                    col += 1
            self.set_parameters(sets[-1])
            return out
        programs = self._mean_programs(means)
        if laid is not None and programs is not None:
            # every mean has a device program: the mean columns of the B full vectors in one slice, one call
            full, n_k, n_m = laid
            ctx = self._backend()
            for i, (ops, par) in enumerate(programs):
                ctx.set_mean(i, ops, par)
            out = ctx.eval_mean(full[:, n_k:n_k + n_m], tstar)
            self.set_parameters(sets[-1])
            return out
        out = []
        for x in sets:
            self.set_parameters(x)
            out.append(np.array(np.array_split(self._mean(self._get_components()[2], tstar), self.p)))
        return np.array(out)

    def _refuse_variational_batch(self, what):
        if self._predict_form == 'variational':
            raise NotImplementedError(
                f"{what} is not available with predict='variational' unless from_sweeps=True is given: the side-by-side "
                "evaluations of the reference form keep no committed sweep per vector.  from_sweeps=True runs each "
                "vector's loop and a prediction pass at the end of a batch chunk, where the slabs still hold each "
                "evaluation's X; else set predict_form = 'reference'")

    def posterior_predictive(self, parameter_sets, tstar=None, weights=None, draws=None, **kw):
        """
        The first two moments of the mixture of ``predict_batch``'s predictions over `parameter_sets` -- the posterior
        predictive of a chain: ``mean = sum_b w_b mean_b``, ``var = sum_b w_b (var_b + mean_b^2) - mean^2``.  `weights`
        (B,): default uniform, normalised to sum 1.  Further keywords go to ``predict_batch`` untouched (``states``,
        ``max_iter``; ``from_sweeps=True`` with ``sweeps`` / ``start``: the variational form, each vector predicted from the
        posterior its own loop leaves).
        ``draws=k`` (``predict='variational'``; uniform `weights` only, else ``ValueError``: resample the chain first)
        additionally returns k joint curves per vector from ``sample_posterior_batch`` -- ``max_iter``, ``sweeps`` and ``start``
        as given here, ``rng`` and ``noise`` its own; every vector's loop starts from the state the call found.
        Returns (mean (N*, p), variance (N*, p)) and, with `draws`, the curves (B k, N*, p), k per vector.
        """
        draw_kw = {key: kw.pop(key) for key in ('rng', 'noise') if key in kw}
        if draws is None and draw_kw:
            raise ValueError('posterior_predictive: `rng` and `noise` go with `draws`')
        if draws is not None:
            if int(draws) < 1:
                raise ValueError('posterior_predictive: draws >= 1 curves per vector expected')
            if weights is not None and np.ptp(np.asarray(weights, dtype=float)) > 0:
                raise ValueError('posterior_predictive: draws come one set per vector -- with non-uniform weights resample '
                                 'the chain first')
            if self._predict_form != 'variational':
                raise ValueError("posterior_predictive: draws need predict='variational' (predict_form)")
            kw.setdefault('from_sweeps', True)
        if not kw.get('from_sweeps'):
            self._refuse_variational_batch('posterior_predictive')
        kw.pop('separate', None)
        found = (self._mu, self._var)
        mean_b, var_b = self.predict_batch(parameter_sets, tstar=tstar, **kw)
        B = mean_b.shape[0]
        w = np.full(B, 1.0 / B) if weights is None else np.asarray(weights, dtype=float)
        if w.shape != (B,) or np.any(w < 0) or not np.sum(w) > 0:
            raise ValueError(f'posterior_predictive: weights must be {B} non-negative numbers with a positive sum')
        w = (w / np.sum(w))[:, None, None]
        mean = np.sum(w * mean_b, axis=0)
        var = np.sum(w * (var_b + mean_b * mean_b), axis=0) - mean * mean
        if draws is None:
            return mean, var
        self._mu, self._var = found
        curves = self.sample_posterior_batch(parameter_sets, tstar=tstar, n=int(draws), max_iter=kw.get('max_iter'),
                                             sweeps=kw.get('sweeps'), start=kw.get('start'), **draw_kw)
        return mean, var, curves.reshape((-1,) + curves.shape[2:])

    # ------------------------------------------------------------ gradients
    def grad_ELBO(self, mean_sweeps=8, mean_start=None, total=False, fused=False):
        """
        Gradient of the ELBO with respect to ALL parameters (the order of ``get_parameters(
        include_frozen=True)``: nodes, weights, means, jitters) at the current variational state.

        Not in the reference, whose optimiser is derivative-free (meanfield.py:1149-1150).
        One more committed sweep is run from the stored state with the explicit covariances kept; the
        gradient is the partial derivative of THAT sweep's ELBO (returned with it) at fixed variational
        means and covariances -- what the envelope theorem makes the total derivative at a converged state:

        * kernel hyper-parameters enter through the expected log prior only (meanfield.py:992-1067):
          ``dELBO/dtheta = 1/(2q) < K^-1 S K^-1 + a a^T - K^-1 , dK/dtheta >`` with ``a = K^-1 m`` and the
          (S, m) the reference pairs with that kernel -- quirks included: node j meets the cumulative
          ``Sigma_f0 + ... + Sigma_fj`` (Q1), weight (j, i) the raw-reshape row of ``mu_w`` (Q2).  The
          N^3 work (K^-1, K^-1 S K^-1) runs on the GPU (``gprn_grad_matrices``); ``dK/dtheta`` comes from
          ``covFunction._dk_dpars`` (closed forms for SquaredExponential, Periodic, QuasiPeriodic; Richardson-extrapolated
          central differences of ``kernel(r)`` otherwise, user kernels included).
        * jitters enter through the expected log likelihood (meanfield.py:895-990), in closed form.
        * mean-function parameters: at a fixed variational state, zero -- the reference's likelihood term reads
          the RAW data (quirk Q3), so the reported ELBO does not see them.  They act through the residual
          ``y - mean`` that the coordinate-ascent update reads (meanfield.py:623-624, 765-792), i.e. by moving the
          state the sweeps converge to; and because the update maximises a bound on the mean-subtracted data
          while the ELBO is evaluated on the raw data, that state is not stationary for the reported ELBO and the
          envelope theorem does not make the effect vanish.  With ``mean_sweeps > 0`` (default 8) these few
          entries are therefore central differences (relative step 1e-4) of the ELBO after ``mean_sweeps`` forced
          sweeps from the stored state with the mean parameter moved, everything else as it is: two short device
          runs per mean parameter, priors untouched (``mean_start``: run them from this ``(mu, var)`` instead of the
          stored state).  ``mean_sweeps=0`` gives the partial derivative (zeros).

        ``total=True``: the gradient of what the sweeps CONVERGE to, for every parameter.  With zero mean functions that
        is the fixed-state gradient above (the envelope theorem holds: checked to 1e-5 in the tests).  With non-zero mean
        functions it is not -- the fixed-state entries of the kernel parameters miss it by 2-85 % and one jitter even has
        the wrong sign at the test problem -- so then EVERY free parameter gets the finite-difference treatment of the
        mean-function parameters: central differences of the ELBO after ``mean_sweeps`` forced sweeps (two set-ups and
        runs per kernel parameter: this is for small problems and few parameters).

        ``fused=True``: the same gradient in the B-form, one device call for all kernel parameters
        (``gprn_grad_elbo``).  With ``B = I + S K S`` and ``X = chol(B)^-1`` as the sweep leaves it,
        ``K^-1 Sigma K^-1 - K^-1 = -S B^-1 S``, so the matrix that meets ``dK/dtheta`` is ``1/2 (a a^T - S B^-1 S)`` (plus
        the Q1 cross terms of the nodes j >= 1): the committed sweep runs WITHOUT the explicit covariances, on whichever
        path the problem takes, and nothing is divided by ``s`` -- which is why this form is also the gradient under a
        data mask (the default form raises ``NotImplementedError`` there).  Latent GPs with user-defined kernels get
        their matrix from ``gprn_grad_matrix`` and are contracted on the host.  The entries of the two forms agree to
        the accuracy of the explicit one (the B-form is the better conditioned: DESIGN.md 9 f-3).  Where the sweep meets
        a non-positive pivot (``last_info != 0``) this form returns ``(-inf, zeros)`` and keeps the stored state.

        ``elbo='bound'``: the gradient of the bound form, at fixed state, for EVERY parameter class -- kernel parameters
        ``< 1/2 (a a^T - S B^-1 S), dK/dtheta >`` with ``a = K^-1 m`` from the latent GP's own mean (no cross term, nothing
        divided by q), jitters in closed form with ``y - mean``, mean-function parameter theta of output i
        ``sum_n ((y - mean)_in - fit_in) / v_in  d mean_i(t_n) / d theta`` over the observed entries
        (``meanFunction._dm_dpars``).  The B-form is the only one there is (``fused`` left at its default selects it; the
        explicit form, which needs the reference's pairing, is not offered).  The bound is the function the updates
        maximise, so at a converged state it is stationary in the variational state and this fixed-state gradient is the
        total one (envelope theorem): ``total=True`` and ``mean_sweeps`` change nothing, and no differences of forced
        sweeps are ever run.

        Returns ``(ELBO, gradient)``.  Unsharded problems only.
        """
        bound = self._elbo == 'bound'
        fused = bool(fused) or bound
        if fused:
            if self._comm is not None:
                raise NotImplementedError('grad_ELBO(fused=True) is not available on a sharded inference object')
        else:
            self._refuse_masked('grad_ELBO')
        assert self._components_set, _NOT_SET
        if self._mu is None:
            self.ELBOcalc()
        nodes, weights, means, jitters = self._get_components()
        ctx = self._setup_device(nodes, weights, means, jitters)
        mu_in, var_in = np.array(self._mu, dtype=float), np.array(self._var, dtype=float)
        ctx.set_muvar(mu_in, var_in)
        if fused:
            elbo, _, info = ctx.sweep(1, commit=True)
            if info:
                # a non-positive pivot: no factors to take the gradient from.  As in the default form the ELBO is not
                # finite there and nELBO_and_grad hands a line search (inf, 0) to back off from; the state is kept
                self.last_info = info
                return -np.inf, np.zeros(len(self.get_parameters(include_frozen=True)))
            mu, var = ctx.get_muvar()
            grads = self._grad_from_state(nodes, weights, means, jitters, mu, var, None, fused=ctx, bound=bound)
        else:
            ctx.keep_sigma(True)
            try:
                elbo, _, info = ctx.sweep(1, commit=True)
                mu, var = ctx.get_muvar()
                grads = self._grad_from_state(nodes, weights, means, jitters, mu, var, ctx.grad_matrices,
                                              device=ctx.grad_kernel)
            finally:
                ctx.keep_sigma(False)
        self._mu, self._var = mu, var
        self.last_info = info
        if fused:
            self._mark_swept(nodes, weights, means, jitters)     # (gprn_grad_elbo keeps X, s and X^T X z)
        grads = np.array(grads)
        n_k = sum(k.pars.size for k in chain(nodes, weights))
        n_m = sum(0 if m_ is None else int(m_._parsize) for m_ in means)
        if bound:
            pass                                   # (the fixed-state gradient is the whole of it: see the docstring)
        elif total and mean_sweeps > 0 and np.any(self._mean(means) != 0.0):
            m0, v0 = (mu_in, var_in) if mean_start is None else mean_start
            grads[:] = self._mean_parameter_differences(0, grads.size, m0, v0, int(mean_sweeps), (mu, var), rel_step=1e-5)
        elif mean_sweeps > 0:
            if n_m:
                m0, v0 = (mu_in, var_in) if mean_start is None else mean_start
                grads[n_k:n_k + n_m] = self._mean_parameter_differences(n_k, n_m, m0, v0, int(mean_sweeps), (mu, var))
        return float(elbo[0]), grads

    def _mean_parameter_differences(self, first, count, mu, var, n_sweeps, restore, rel_step=1e-4):
        """d/dtheta of the ELBO after `n_sweeps` forced sweeps from the state (mu, var), for the `count`
        mean-function parameters that start at position `first` of the full parameter vector: central
        differences, the device's priors untouched (only ``y - mean`` changes); the device state ends as `restore`."""
        full = self.get_parameters(include_frozen=True).copy()
        out = np.zeros(count)
        try:
            for n in range(count):
                if self.frozen_mask[first + n]:
                    continue                                      # not a variable of anybody's optimisation
                v = full[first + n]
                h = rel_step * max(1.0, abs(v))
                e = []
                for sign in (1.0, -1.0):
                    x = full.copy()
                    x[first + n] = v + sign * h
                    self.set_parameters(x)
                    nodes, weights, means, jitters = self._get_components()
                    ctx = self._setup_device(nodes, weights, means, jitters)
                    ctx.set_muvar(mu, var)
                    e.append(ctx.sweep(n_sweeps, commit=False)[0][-1])
                out[n] = (e[0] - e[1]) / (2 * h) if np.all(np.isfinite(e)) else 0.0
        finally:
            self.set_parameters(full)
            nodes, weights, means, jitters = self._get_components()
            self._setup_device(nodes, weights, means, jitters).set_muvar(*restore)
        return out

    def _grad_from_state(self, nodes, weights, means, jitters, mu, var, matrices, device=None, fused=None, bound=False):
        """The O(N^2) and O(pqN) part of grad_ELBO: `matrices(gp)` returns ``(K^-1, K^-1 S K^-1)`` of latent GP
        `gp` (the GPU's ``gprn_grad_matrices``; a NumPy stand-in in the CPU tests).  `device(gp, m, n)`, when
        given, is tried first: the whole contraction on the GPU (``gprn_grad_kernel``: closed-form or
        central-difference dK/dtheta of the kernel's device program), None for kernels without one.
        `fused`: the device context after a committed sweep -- the B-form instead: every kernel with a device program in
        ONE call (``gprn_grad_elbo``), the others through ``gprn_grad_matrix`` (G itself) and the host contraction
        below; `matrices` and `device` are not used then.
        `bound`: the entries of the bound form (``elbo='bound'``): every latent GP with its own mean, nothing divided by q,
        ``y - mean`` in the jitter entries, the mean-function entries from ``meanFunction._dm_dpars``."""
        t = np.asarray(self.time, dtype=float)
        # (N x N on the host: formed only for a kernel that is contracted here -- 134 MB and 16 ms at N = 4096)
        r = None
        q, p, N = self.q, self.p, self.N
        m_scr = mu[1:].reshape(q, p, N)                      # quirk Q2 (meanfield.py:1021)
        qdiv = 1.0 if bound else float(q)                    # ELBO = (...) / q, meanfield.py:709 -- not in the bound form
        grads = []
        on_dev = None
        if fused is not None:
            counts = [k.pars.size if isinstance(k, covfunc.covFunction) and k._device_program() is not None else 0
                      for k in chain(nodes, weights)]
            on_dev = list(fused.grad_elbo(int(sum(counts))))
        for gp, kernel in enumerate(chain(nodes, weights)):
            if fused is not None:
                if counts[gp]:
                    grads += [float(on_dev.pop(0)) / qdiv for _ in range(counts[gp])]
                    continue
                G = fused.grad_matrix(gp) / qdiv
                if isinstance(kernel, _TWO_ARGUMENT):
                    dks = covfunc._richardson(kernel, lambda: np.asarray(kernel(t[:, None], t[None, :]), dtype=float))
                else:
                    r = t[:, None] - t[None, :] if r is None else r
                    dks = kernel._dk_dpars(r)
                grads += [float(np.sum(G * dk)) for dk in dks]
                continue
            if gp < q:
                m = mu[0, gp]
            else:
                jj, ii = divmod(gp - q, p)
                m = mu[1 + ii, jj] if bound else m_scr[jj, ii]
            if device is not None and kernel._device_program() is not None:
                on_device = device(gp, m, kernel.pars.size)
                if on_device is not None:
                    grads += [float(v) / qdiv for v in on_device]
                    continue
            Kinv, P = matrices(gp)
            a = Kinv @ m
            G = 0.5 * (P - Kinv + np.outer(a, a)) / qdiv
            if isinstance(kernel, _TWO_ARGUMENT):             # kernel(t_i, t_j): differences only
                dks = covfunc._richardson(kernel, lambda: np.asarray(kernel(t[:, None], t[None, :]), dtype=float))
            else:
                r = t[:, None] - t[None, :] if r is None else r
                dks = kernel._dk_dpars(r)
            grads += [float(np.sum(G * dk)) for dk in dks]
        # jitters: LogL = -1/2 sum [log(2 pi v) + ((Y - fit)^2 + A) / v],  v = jitter^2 + yerr^2
        variance = np.asarray(jitters, dtype=float)[:, None]**2 + self.yerr2
        fit = np.einsum('iqn,qn->in', mu[1:], mu[0])
        # (Y: the raw data, quirk Q3 -- y - mean in the bound form, which therefore sees the mean-function parameters)
        Y = self.y - self._mean(means).reshape(p, N) if bound else self.y
        if bound:
            w = (Y - fit) / variance
            if self.mask is not None:
                w = np.where(self.mask, w, 0.0)
            for i, m_ in enumerate(means):
                if m_ is None:
                    continue
                dm = m_._dm_dpars(t)
                grads += [0.0] * int(m_._parsize) if dm is None else [float(v) for v in np.asarray(dm, dtype=float) @ w[i]]
        else:
            grads += [0.0] * sum(0 if m_ is None else int(m_._parsize) for m_ in means)
        A = np.zeros((p, N))
        for i in range(p):
            for j in range(q):
                A[i] += var[0, j] * mu[1 + i, j]**2 + var[1 + i, j] * mu[0, j]**2 + var[0, j] * var[1 + i, j]
        dv = -0.5 * (1.0 / variance - ((Y - fit)**2 + A) / variance**2)
        if self.mask is not None:                            # observed entries only (whatever a masked y / yerr holds)
            dv = np.where(self.mask, dv, 0.0)
        grads += [float(np.sum(dv[i]) * 2 * jitters[i]) / qdiv for i in range(p)]
        return grads

    def nELBO_and_grad(self, parameters, max_iter=None, sweeps=None, start=None, fused=False):
        """``(-ELBO, -dELBO/dparameters)`` over the FREE parameters, for gradient-based optimisers.  Default:
        ``nELBO(parameters)`` (warm-started ELBOcalc, as the reference's objective), then ``grad_ELBO``.  With
        ``sweeps`` (and a start state ``(mu, var)``): the ELBO after exactly that many forced sweeps from ``start``
        plus the one ``grad_ELBO`` adds -- a deterministic, smooth function of the parameters.  ``fused``: as in
        ``grad_ELBO`` (one device call for the kernel parameters; allowed under a data mask).  With ``elbo='bound'`` the
        B-form is the only one and the gradient is exact for every parameter (``grad_ELBO``)."""
        fused = bool(fused) or self._elbo == 'bound'
        if fused:
            if self._comm is not None:
                raise NotImplementedError('nELBO_and_grad(fused=True) is not available on a sharded inference object')
        else:
            self._refuse_masked('nELBO_and_grad')
        if sweeps is None:
            self.nELBO(parameters, max_iter=max_iter)
            elbo, grad = self.grad_ELBO(fused=fused)
            return -elbo, -grad[~self.frozen_mask]
        assert self._components_set, _NOT_SET
        self.set_parameters(np.array(parameters, dtype=float))
        nodes, weights, means, jitters = self._get_components()
        if start is None:
            start = self._initMuVar(nodes, weights, jitters)
        ctx = self._setup_device(nodes, weights, means, jitters)
        ctx.set_muvar(np.asarray(start[0], dtype=float), np.asarray(start[1], dtype=float))
        _, _, info = ctx.sweep(int(sweeps), commit=True)
        self.last_info = info
        self._mu, self._var = ctx.get_muvar()
        elbo, grad = self.grad_ELBO(mean_sweeps=int(sweeps) + 1, mean_start=start, total=True, fused=fused)
        if not np.isfinite(elbo):
            return np.inf, np.zeros(int((~self.frozen_mask).sum()))
        return -elbo, -grad[~self.frozen_mask]

    def _jitter_grads_batch(self, jitters, mu, var, resid=None):
        """``_grad_from_state``'s jitter entries for B states at once: ``jitters (B, p)``, ``mu`` / ``var (B, p + 1, q, N)``
        -> ``(B, p)``, d ELBO / d jitter_i at fixed state (LogL = -1/2 sum [log(2 pi v) + ((Y - fit)^2 + A) / v],
        v = jitter^2 + yerr^2; divided by q as the ELBO is, meanfield.py:709).  `resid` ``(B, p, N)``: the bound form's
        entries -- Y is each vector's own ``y - mean``, and nothing is divided by q."""
        jitters = np.asarray(jitters, dtype=float)
        mu, var = np.asarray(mu, dtype=float), np.asarray(var, dtype=float)
        variance = jitters[:, :, None]**2 + self.yerr2[None]
        fit = np.einsum('biqn,bqn->bin', mu[:, 1:], mu[:, 0])
        mf2, vf = mu[:, :1]**2, var[:, :1]
        A = np.sum(vf * mu[:, 1:]**2 + var[:, 1:] * mf2 + vf * var[:, 1:], axis=2)
        Y = self.y[None] if resid is None else np.asarray(resid, dtype=float)
        dv = -0.5 * (1.0 / variance - ((Y - fit)**2 + A) / variance**2)
        if self.mask is not None:
            dv = np.where(self.mask[None], dv, 0.0)
        return np.sum(dv, axis=2) * 2 * jitters / (self.q if resid is None else 1.0)

    def _mean_grads_batch(self, sets, jitters, mu, resid):
        """The bound form's mean-function entries for B vectors: ``sum_n ((y - mean)_in - fit_in) / v_in d mean_i / d theta``
        over the observed entries, each vector at its own parameters.  ``(B, n_mean_parameters)``; the object's parameters
        end at the last vector."""
        jitters = np.asarray(jitters, dtype=float)
        mu = np.asarray(mu, dtype=float)
        t = np.asarray(self.time, dtype=float)
        fit = np.einsum('biqn,bqn->bin', mu[:, 1:], mu[:, 0])
        w = (np.asarray(resid, dtype=float) - fit) / (jitters[:, :, None]**2 + self.yerr2[None])
        if self.mask is not None:
            w = np.where(self.mask[None], w, 0.0)
        programs = self._mean_programs(self.means)
        laid = None if programs is None else self._full_vectors([np.asarray(x) for x in sets])
        if laid is not None:
            # ``device_means``: d mean / d theta of all B vectors in ONE gprn_eval_mean_grad call, contracted here
            full, n_k, n_m = laid
            ctx = self._backend()
            for i, (ops, par) in enumerate(programs):
                ctx.set_mean(i, ops, par)
            dm = ctx.eval_mean_grad(full[:, n_k:n_k + n_m])
            owner = np.repeat(np.arange(self.p), [par.size for _, par in programs])
            self.set_parameters(sets[-1])
            return np.einsum('bkn,bkn->bk', dm, w[:, owner])
        rows = []
        for b, x in enumerate(sets):
            self.set_parameters(x)
            row = []
            for i, m_ in enumerate(self.means):
                if m_ is None:
                    continue
                dm = m_._dm_dpars(t)
                row += [0.0] * int(m_._parsize) if dm is None else list(np.asarray(dm, dtype=float) @ w[b, i])
            rows.append(row)
        return np.array(rows, dtype=float).reshape(len(sets), -1)

    def nELBO_and_grad_batch(self, parameter_sets, max_iter=None, sweeps=None, start=None):
        """
        ``(values, grads)`` for several free-parameter vectors: ``values`` a list of ``-ELBO``, ``grads`` an array
        ``(B, n_free)`` of ``-dELBO/d(free parameters)`` -- the objective and gradient a multi-start gradient optimiser or a
        gradient-based ensemble sampler asks for, all vectors SIDE BY SIDE on the GPU (``gprn_elbocalc_batch_grad``).  Not
        in the reference, whose optimiser is derivative-free (meanfield.py:1149-1150).

        The gradient is the fixed-state one of ``grad_ELBO(mean_sweeps=0, fused=True)``, and value and gradient belong to the
        SAME sweep, the last one of that vector's loop (no further sweep is run for the gradient):

        * kernel hyper-parameters: the B-form on the device, ``1/(2q) < a a^T - S B^-1 S (+ the Q1 cross terms), dK/dtheta >``
          at the state and factors that sweep left (quirks Q1, Q2 as in ``grad_ELBO``);
        * jitters: closed form from each vector's returned state (``_grad_from_state``'s formula, vectorised);
        * mean-function parameters: zero.  At a fixed variational state the reported ELBO does not see them -- the
          reference's likelihood term reads the RAW data (quirk Q3) -- and because the update maximises a bound on the
          mean-subtracted data while the ELBO is evaluated on the raw data, the state the sweeps converge to is not
          stationary for it: the envelope theorem does not make their effect through the state vanish.  What
          ``grad_ELBO(mean_sweeps > 0)`` adds by differences is not computed here.

        ``sweeps=n`` (n >= 1): every vector runs exactly ``n`` forced sweeps -- no stop rule: a deterministic, smooth
        function of the parameters -- from ``start`` = ``(mu, var)``, else the stored state, else ``_initMuVar``.  Without
        ``sweeps``: the warm-started loop under the stop rule (``max_iter`` >= 1 trips at most), every vector from the state
        the object holds, as ``nELBO_batch``; the object then keeps the state of the last vector whose loop converged
        (``start`` without ``sweeps`` is a ``ValueError``).
        A vector whose factorisation meets a non-positive pivot returns ``(inf, zeros)``.

        ``elbo='bound'``: the entries of the bound form (``grad_ELBO``) -- own means, no cross terms, nothing divided by q,
        the jitter entries with each vector's own ``y - mean``, and the mean-function entries filled in from
        ``meanFunction._dm_dpars``: the whole gradient, exact at a converged state.

        Where the side-by-side form does not apply (user-defined kernels, N above ``batch_max_N``, a data mask without
        ``batch_under_mask``, kernel expressions that change shape between vectors) the vectors are evaluated one by one with the same meaning: the
        loop, then ``gprn_grad_elbo`` on what it left.  Unsharded objects only.
        """
        if self._comm is not None:
            raise NotImplementedError('nELBO_and_grad_batch is not available on a sharded inference object')
        sets, forced, trips, _ = self._batch_request('nELBO_and_grad_batch', parameter_sets, max_iter, sweeps, start, empty_ok=True,
                                                     no_trips='nELBO_and_grad_batch: a gradient needs at least one sweep')
        n_free, n_all = int((~self.frozen_mask).sum()), int(self.frozen_mask.size)
        for x in sets:
            if x.ndim != 1:                                    # (before anything of the object changes)
                raise ValueError('nELBO_and_grad_batch: one-dimensional parameter vectors expected')
            if x.size not in (n_free, n_all):
                self.set_parameters(x)                         # (raises the reference's ValueError, meanfield.py:223-259)
        free = ~self.frozen_mask
        if not sets:
            return [], np.zeros((0, n_free))
        entry = (self._mu, self._var) if start is None else start
        staged = self._batch_stage(sets, start=start)
        res = None
        if staged is not None:
            ctx, kp, yr, jt, m0, v0 = staged
            n_k = sum(k.pars.size for k in chain(self.nodes, self.weights))
            if kp.shape[1] == n_k:                             # (every program's parameters are its kernel's own)
                res = ctx.elbocalc_batch(kp, yr, jt, m0, v0, trips, want_state=True, want_grad=True, forced=forced)
        if res is not None:
            elbo, _, _, info, mu_f, var_f, g_k = self._batch_keep(res)
            n_m = n_all - n_k - self.p
            if self._elbo == 'bound':
                on_device = isinstance(yr, _hip.MeanParams)        # (device_means: y - mean and the mean entries came with the call)
                resid = np.reshape(yr.resid if on_device else yr, (len(sets), self.p, self.N))
                mean_rows = yr.mean_grad if on_device else self._mean_grads_batch(sets, jt, mu_f, resid)
                grads = np.concatenate((g_k, mean_rows.reshape(len(sets), n_m),
                                        self._jitter_grads_batch(jt, mu_f, var_f, resid=resid)), axis=1)
            else:
                grads = np.concatenate((g_k / self.q, np.zeros((len(sets), n_m)), self._jitter_grads_batch(jt, mu_f, var_f)), axis=1)
            bad = (info > 0) | ~np.isfinite(elbo)
            grads[bad] = 0.0
            values = [float('inf') if b else float(-e) for e, b in zip(elbo, bad)]
            return values, -grads[:, free]
        # one by one, each vector from the same state
        grads = np.zeros((len(sets), n_free))

        def value_and_grad(b, ctx, components, info, history, mu, var):
            e = history[-1]
            if info or not np.isfinite(e):
                return float('inf'), True
            g = np.array(self._grad_from_state(*components, mu, var, None, fused=ctx, bound=self._elbo == 'bound'))
            grads[b] = -g[free]
            return float(-e), False

        values = self._one_by_one(sets, entry, forced, trips, value_and_grad, variational=False, chain_info=True)
        return values, grads

    # ------------------------------------------------ held-out scores: cross-validation side by side
    def _data_mask(self):
        """The object's data mask as a (p, N) bool array (all True without one)."""
        return np.ones((self.p, self.N), dtype=bool) if self.mask is None else np.asarray(self.mask, dtype=bool)

    def _check_fit_masks(self, fit_masks, B, what):
        """(B, p, N) bool fit masks under the data mask that obey the mask's own rules, or a ``ValueError`` naming the
        evaluation -- before anything touches a device."""
        fit = np.asarray(fit_masks)
        if fit.shape != (B, self.p, self.N):
            raise ValueError(f'{what}: fit_masks must have shape (B, p, N) = {(B, self.p, self.N)}, got {fit.shape}')
        fit = fit.astype(bool)
        D = self._data_mask()
        for b in range(B):
            if np.any(fit[b] & ~D):
                raise ValueError(f'{what}: fit mask {b} fits an entry the data mask does not hold')
            empty = np.flatnonzero(~fit[b].any(axis=1))
            if empty.size:
                raise ValueError(f'{what}: fit mask {b} leaves output(s) {empty.tolist()} without a fitted entry')
            if self.q >= 2:
                gaps = np.flatnonzero(~fit[b].any(axis=0))
                if gaps.size:
                    raise ValueError(f'{what}: fit mask {b} leaves time index(es) {gaps[:10].tolist()} without a fitted '
                                     f'output (q >= 2 needs one at every time)')
        return fit

    def heldout_batch(self, parameter_sets, fit_masks, max_iter=None, sweeps=None, start=None):
        """
        Fit vector b of ``parameter_sets`` on the entries ``fit_masks[b]`` (p, N; True = fitted) and score the rest: the
        held-out log predictive density, all evaluations SIDE BY SIDE on the GPU (``gprn_elbocalc_batch_heldout``) --
        k folds x S vectors of a cross-validation in one call.  Not in the reference, whose only model score is the ELBO.

        Every fit mask lies under the object's data mask D and obeys its rules (an entry per output; with q >= 2 an output
        at every time); evaluation b holds out ``D & ~fit_masks[b]``.  ``sweeps=n``: exactly n forced sweeps, no stop rule,
        as in ``nELBO_and_grad_batch``; else the loop under the stop rule, ``max_iter`` trips at most.  Each evaluation
        starts from ``_initMuVar`` on y zero-filled under ITS fit mask -- what a fresh object with ``mask=fit_masks[b]``
        starts from, so that no held-out value leaks into the start -- or, with ``start=(mu, var)``, from that state.

        Returns a ``HeldOut`` record: ``lpd`` (B, p) and ``n_held`` (B, p), the log predictive density summed over the
        held-out entries of each output and their number; ``mean`` and ``var`` (B, p, N), the predictive mean (mean
        functions included) and variance (jitter once, yerr^2 included) at the held-out entries, zero elsewhere; ``elbo``,
        ``iterations``, ``converged``, ``info`` (B,) and ``state_mu``, ``state_var`` -- row b what ``ELBOcalc`` returns on an
        object with ``mask=fit_masks[b]``.  An evaluation whose factorisation failed has NaN in ``elbo``, ``lpd`` and rows.

        Where the side-by-side form does not apply this raises ``NotImplementedError`` with the reason -- a sharded
        object, user-defined kernels, ``sweep_order='sequential'``, N above ``batch_max_N``; there is no silent one-by-one
        fallback.  The object's stored state is left alone; its parameters end at the last vector.
        """
        what = 'heldout_batch'
        sets, forced, trips, _ = self._batch_request(what, parameter_sets, max_iter, sweeps, start, start_needs_sweeps=False,
                                                     no_trips=f'{what}: a held-out score needs at least one committed sweep')
        B = len(sets)
        if any(x.ndim != 1 for x in sets):
            raise ValueError(f'{what}: one-dimensional parameter vectors expected')
        fit = self._check_fit_masks(fit_masks, B, what)
        if start is not None and (len(start) != 2 or np.size(start[0]) != self.d or np.size(start[1]) != self.d):
            raise ValueError(f'{what}: start must be (mu, var) of {self.d} values each')
        if self._comm is not None:
            raise NotImplementedError(f'{what} is not available on a sharded inference object')
        if self._sweep_order != 'reference':
            raise NotImplementedError(f"{what}: per-evaluation fit masks are not supported under sweep_order='sequential'")
        if self.N > self.batch_max_N:
            raise NotImplementedError(f'{what}: N = {self.N} is above batch_max_N = {self.batch_max_N}, the largest problem '
                                      'the side-by-side form takes')
        self._need_programs(what, *self._get_components()[:2])
        placeholder = (np.zeros(self.d), np.ones(self.d))
        staged = self._batch_stage(sets, start=placeholder if start is None else start, own_masks=True)
        if staged is None:
            raise NotImplementedError(f'{what}: the vectors cannot be laid out side by side (lengths that differ, or kernel '
                                      'expressions that change shape between vectors)')
        ctx, kp, yr, jt, m0, v0 = staged
        if start is None:
            y_all = self.y
            try:
                for b, x in enumerate(sets):
                    self.set_parameters(x)
                    nodes, weights, _, jitters = self._get_components()
                    self.y = np.where(fit[b], y_all, 0.0)
                    mu, var = self._initMuVar(nodes, weights, jitters)
                    m0[b], v0[b] = np.ravel(mu), np.ravel(var)
            finally:
                self.y = y_all
        res = ctx.elbocalc_batch_heldout(kp, yr, jt, m0, v0, trips, fit, forced=forced)
        if res is None:
            raise NotImplementedError(f'{what}: the library has no side-by-side form for this problem')
        elbo, iters, conv, info, mu_f, var_f, hmean, hvar, lpd, n_held = res
        self.last_info = _first_verdict(info)
        held = self._data_mask()[None] & ~fit
        hmean = np.where(held, hmean + self._mean_values_batch(sets, np.asarray(self.time, dtype=float)), hmean)
        return HeldOut(lpd=lpd, n_held=n_held, mean=hmean, var=hvar, elbo=elbo, iterations=iters, converged=conv, info=info,
                       state_mu=mu_f, state_var=var_f)

    def cv_folds(self, k, scheme='entries', block=None, rng=None):
        """
        ``k`` fit masks (k, p, N) under the object's data mask for a k-fold cross-validation: fold f fits everything but
        the observed entries assigned to it.

        * ``scheme='entries'``: entry (i, n) goes to fold (r_n + i) mod k with a seeded r_n per time, so that (with p <= k)
          two outputs of one time never share a fold;
        * ``scheme='blocks'``: per output, contiguous runs of ``block`` times (default: about N / (2 k)) go to one fold, run
          r of output i to fold (r + i + r_0) mod k -- whole seasons are held out, the runs of the outputs offset.

        Every observed entry is held out in exactly one fold, except those whose removal would break the mask's rules -- the
        only fitted entry of an output, or with q >= 2 the only observed output of a time: they stay fitted in every fold
        and are counted in the result's ``n_never_held``.  ``rng``: a seed or a ``numpy.random.RandomState``.
        ``ValueError`` where no valid split exists: k < 2, or q >= 2 with p = 1.
        """
        k = int(k)
        if k < 2:
            raise ValueError('cv_folds: k >= 2 folds expected')
        if self.q >= 2 and self.p == 1:
            raise ValueError('cv_folds: with q >= 2 every time needs a fitted output, and with p = 1 nothing can be held out')
        if scheme not in ('entries', 'blocks'):
            raise ValueError(f"cv_folds: scheme must be 'entries' or 'blocks', got {scheme!r}")
        rs = rng if isinstance(rng, np.random.RandomState) else np.random.RandomState(rng)
        D = self._data_mask()
        i_idx, n_idx = np.arange(self.p)[:, None], np.arange(self.N)[None, :]
        if scheme == 'entries':
            fold = (rs.randint(0, k, size=self.N)[None, :] + i_idx) % k
        else:
            block = max(1, self.N // (2 * k)) if block is None else int(block)
            if block < 1:
                raise ValueError('cv_folds: block >= 1 times expected')
            fold = (n_idx // block + i_idx + rs.randint(0, k)) % k
        hold = np.array([D & (fold == f) for f in range(k)])
        for f in range(k):
            fitted = D & ~hold[f]
            if self.q >= 2:                                    # a time whose observed outputs all went to this fold keeps its first
                for n in np.flatnonzero(D.any(axis=0) & ~fitted.any(axis=0)):
                    hold[f, np.flatnonzero(D[:, n])[0], n] = False
            fitted = D & ~hold[f]
            for i in np.flatnonzero(~fitted.any(axis=1)):       # an output with nothing left keeps its first observed entry
                hold[f, i, np.flatnonzero(D[i])[0]] = False
        folds = (D[None] & ~hold).view(_Folds)
        folds.n_never_held = int((D & ~hold.any(axis=0)).sum())
        return folds

    def cross_validate(self, folds, parameter_sets=None, **kw):
        """
        k-fold cross-validation of S parameter vectors in ONE side-by-side call: the S x k evaluations, set-major, through
        ``heldout_batch`` (whose keywords ``max_iter``, ``sweeps``, ``start`` pass through).  ``folds``: (k, p, N) fit masks,
        as ``cv_folds`` returns them; ``parameter_sets``: default the object's current vector.

        Returns a ``CrossValidation`` record: ``lpd`` (S, k, p) and ``n_held`` (S, k, p); ``elpd`` (S,), the sum of ``lpd``
        over folds and outputs -- the score to compare models by; ``mean`` and ``var`` (S, p, N), each entry from the fold
        that held it out, NaN where no fold did; ``elbo``, ``iterations``, ``converged``, ``info`` (S, k).
        """
        folds = np.asarray(folds)
        if folds.ndim != 3 or folds.shape[1:] != (self.p, self.N) or folds.shape[0] < 1:
            raise ValueError(f'cross_validate: folds must have shape (k, p, N) = (k, {self.p}, {self.N}), got {folds.shape}')
        folds = folds.astype(bool)
        k = folds.shape[0]
        sets = [np.array(self.get_parameters(), dtype=float)] if parameter_sets is None else \
            [np.array(x, dtype=float) for x in parameter_sets]
        S = len(sets)
        if S < 1:
            raise ValueError('cross_validate: no parameter vector')
        res = self.heldout_batch([x for x in sets for _ in range(k)], np.tile(folds, (S, 1, 1)), **kw)
        held = self._data_mask()[None] & ~folds                  # (k, p, N)
        mean = np.full((S, self.p, self.N), np.nan)
        var = np.full((S, self.p, self.N), np.nan)
        rm, rv = res.mean.reshape(S, k, self.p, self.N), res.var.reshape(S, k, self.p, self.N)
        for f in range(k):
            mean[:, held[f]] = rm[:, f][:, held[f]]
            var[:, held[f]] = rv[:, f][:, held[f]]
        lpd = res.lpd.reshape(S, k, self.p)
        return CrossValidation(lpd=lpd, elpd=lpd.sum(axis=(1, 2)), n_held=res.n_held.reshape(S, k, self.p), mean=mean, var=var,
                               elbo=res.elbo.reshape(S, k), iterations=res.iterations.reshape(S, k),
                               converged=res.converged.reshape(S, k), info=res.info.reshape(S, k))

    def mcmc(self, priors, p0=None, vars=None, niter=500, **kwargs):
        """
        Sample the posterior of the free parameters with emcee, the ELBO (100
        sweeps at most, warm-started) standing in for the marginal likelihood
        (meanfield.py:1154-1286).  `priors`: dict name -> frozen scipy.stats
        distribution.  emcee is imported here, not at package import; without it
        this raises ImportError.  Returns the sampler.

        Same sequence as the reference: walkers from the priors (or an ellipsoid around `p0`), one
        evaluation of every initial walker (it also moves the warm-start state), a sampler over an HDF
        backend file ``gprn.h5`` that is reset on every call, convergence from the autocorrelation time
        every ten steps.  Beyond the reference: keyword arguments go on to ``emcee.EnsembleSampler`` (the
        reference accepts and drops them), so ``pool=sharding.EvalPool()`` spreads the walkers over the
        GPUs of a node; ``backend=`` replaces the HDF file, and without h5py emcee's in-memory backend is used.
        ``batch=True`` hands emcee a VECTORISED log-probability: the walkers of a half-step are evaluated side by side
        on the GPU (``nELBO_batch``), each from the SAME warm-start state -- the one the object holds when the half-step
        begins -- instead of from its predecessor's converged state (meanfield.py:1102-1104).  What that changes: an
        evaluation is 100 sweeps at most under the 1e-3 stop rule, which fires when progress is slow, not when the fixed
        point is near, so its value depends on where its loop started.  Measured on 40 prior draws of a small problem
        (``tests/test_parity_gpu.py::test_mcmc_with_the_walkers_side_by_side``): side by side against chained, median
        4e-4 relative, nine in ten within 4e-3, worst 0.17 -- and the reference's own chaining differs from itself by the
        same amounts when the same vectors are evaluated in the opposite order.  The batched log-probabilities are
        therefore as good an estimate of the objective as the reference's; the chain is not the reference's walker for
        walker (one accept / reject decision that falls inside that spread sends the ensembles apart for good: a moved
        walker changes every later proposal), the posterior it samples is.
        """
        assert self._components_set, _NOT_SET
        from emcee import EnsembleSampler, backends
        self._select_vars(vars)
        names = np.array(list(self.parameters_dict.keys()))[~self.frozen_mask]

        def draw():
            return np.array([priors[n].rvs() for n in names])

        def logprior(x):
            return float(sum(priors[n].logpdf(v) for v, n in zip(x, names)))

        def logposterior(x):
            lp = logprior(x)
            if np.isneginf(lp):
                return -np.inf, -np.inf
            elbo = -self.nELBO(x, max_iter=100)
            return lp + elbo, elbo

        def logposterior_batch(X):
            X = np.atleast_2d(X)
            # (the priors of all walkers at once, name by name in logprior's order: the same sums, 1 / nwalkers of the
            # scipy.stats calls -- at 40 walkers x 20 parameters those calls outweighed the side-by-side evaluations)
            lp = np.zeros(X.shape[0])
            for k, n in enumerate(names):
                lp = lp + np.asarray(priors[n].logpdf(X[:, k]), dtype=float)
            out = np.full((X.shape[0], 2), -np.inf)
            ok = np.flatnonzero(~np.isneginf(lp))
            if ok.size:
                elbo = -np.array(self.nELBO_batch([X[i] for i in ok], max_iter=100, pool=batch_pool))
                out[ok, 0] = lp[ok] + elbo
                out[ok, 1] = elbo
            return out

        batch = bool(kwargs.pop('batch', False))
        # (a vectorised log-probability never reaches emcee's pool: with both, each rank of the pool evaluates its share
        # of a half-step's walkers side by side -- nELBO_batch(pool=...))
        pool_rank = getattr(kwargs.get('pool'), 'rank', 0)
        batch_pool = kwargs.pop('pool', None) if batch else None

        ndim = len(names)
        nwalkers = 2 * ndim
        print(f'Setting up sampler (parameters: {ndim}, walkers: {nwalkers})')
        if p0 is None:
            p0 = np.array([draw() for _ in range(nwalkers)])
        else:
            from emcee.utils import sample_ellipsoid
            sigma = []
            for n in names:
                try:
                    sigma.append(priors[n].std())
                except TypeError:
                    sigma.append(priors[n].std)
            p0 = sample_ellipsoid(p0, np.diag(sigma) / 100, size=nwalkers)
            for i, x in enumerate(p0):
                if np.isneginf(logprior(x)):
                    p0[i] = draw()
        print('initial values for parameters are set')
        start = time_module.time()
        _ = logposterior_batch(p0) if batch else [logposterior(x) for x in p0]
        print()
        print(f'evaluation for initial values took {time_module.time() - start:.0f} sec')
        print('- adjust your expectations accordingly')

        # the reference's HDF5 file (meanfield.py:1262-1263) -- written by ONE process: with an SPMD pool
        # (sharding.EvalPool) every rank runs this same method, and N writers resetting one file end in an
        # h5py lock error or a corrupt file; the other ranks keep emcee's in-memory backend
        if 'backend' not in kwargs and pool_rank == 0:
            try:
                be = backends.HDFBackend('gprn.h5')
                be.reset(nwalkers, ndim)
                kwargs['backend'] = be
            except (ImportError, OSError):     # h5py missing or the file is locked: emcee's in-memory backend
                pass
        if batch:
            kwargs['vectorize'] = True
        sampler = EnsembleSampler(nwalkers, ndim, logposterior_batch if batch else logposterior, **kwargs)
        old_tau = np.inf
        for sample in sampler.sample(p0, iterations=niter, progress=True):
            if sampler.iteration % 10 == 0:
                print(sample.log_prob.max())
            if sampler.iteration % 10:
                continue
            tau = sampler.get_autocorr_time(tol=0)
            converged = np.all(tau * 100 < sampler.iteration)
            converged &= np.all(np.abs(old_tau - tau) / tau < 0.01)
            if converged:
                print('MCMC converged!')
                break
            old_tau = tau
        return sampler

    def _select_vars(self, vars):
        """ Freeze/thaw by the `vars` convention shared by optimize and mcmc:
        'name' frees only that parameter, '-name' all but it, a list frees those. """
        if vars is None:
            return
        if isinstance(vars, str):
            if '-' in vars:
                self.thaw_parameter(name='*')
                self.freeze_parameter(name=vars.replace('-', ''))
            else:
                self.freeze_parameter(name='*')
                self.thaw_parameter(name=vars)
        elif isinstance(vars, list):
            self.freeze_parameter(name='*')
            for name in vars:
                self.thaw_parameter(name=name)
        else:
            raise ValueError(f'`vars` should be str or list, got {type(vars)}')

