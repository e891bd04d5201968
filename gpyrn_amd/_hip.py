"""ctypes binding of libgprn_hip.so (C ABI: include/gprn_hip.h).

Thin by design: NumPy arrays in, NumPy arrays out, status codes turned into
exceptions.  There is no CPU fallback anywhere in this package -- if the
library or a GPU is missing, `Context()` raises `BackendUnavailable`.
"""
import ctypes
import os
from ctypes import POINTER, byref, c_char, c_char_p, c_double, c_int, c_int32, c_int64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GPRN_HIP_LIB') or os.path.join(_HERE, 'libgprn_hip.so')

GPRN_E_ARG, GPRN_E_HIP, GPRN_E_NODEV, GPRN_E_COMM, GPRN_E_NOMEM, GPRN_E_UNSUPPORTED = -1, -2, -3, -4, -5, -6
GPRN_BATCH_FORCED = 1          # gprn_elbocalc_batch_grad: no stop rule, max_iter committed sweeps per evaluation
COV_JOINT = 1
ORDER_REFERENCE, ORDER_SEQUENTIAL = 0, 1
ELBO_REFERENCE, ELBO_BOUND = 0, 1    # option "elbo_form": the reference's number (quirks Q1-Q3, Q5) or the model's bound
# option "predict_form": _gp.GP.prediction restated, or the predictive of the posterior the committed sweep left
PREDICT_REFERENCE, PREDICT_POSTERIOR = 0, 1
M_K, M_KLINV, M_SIGMA, M_BX, M_BL = 0, 1, 2, 3, 4
T_NAMES = ('fill', 'build_B', 'diag', 'panel', 'update', 'lauum', 'vec', 'update_ahead')
TILE = 128

_dp = POINTER(c_double)


class BackendUnavailable(RuntimeError):
    """libgprn_hip.so is not built, or there is no MI355X to run it on."""


class BackendError(RuntimeError):
    pass


class MeanParams:
    """What stands in for ``y_resid`` in ``Context.elbocalc_batch`` when y - mean is to be formed on the device
    (gprn_elbocalc_batch_means): the B rows of mean parameters (B, n_mean_params) -- the programs are the context's
    (``set_mean``) -- and the raw data (p N).  After the call: ``resid`` (B, p N), the y - mean the call formed, and, where
    asked for (``want_mean_grad``), ``mean_grad`` (B, n_mean_params), the bound form's mean entries."""

    def __init__(self, params, y_raw, want_mean_grad=False):
        self.params = np.ascontiguousarray(params, dtype=np.float64)
        self.y_raw = np.asarray(y_raw, dtype=float).ravel()
        self.want_mean_grad = bool(want_mean_grad)
        self.resid = self.mean_grad = None

    def host_resid(self, ctx):
        """y - mean through gprn_eval_mean, for the entry points that take a host array"""
        return self.y_raw[None] - ctx.eval_mean(self.params).reshape(self.params.shape[0], -1)


# every exported entry point: name -> (restype, argtypes).  tests/test_abi.py
# checks this table against include/gprn_hip.h and the built library.
SIGNATURES = {
    'gprn_device_count': (c_int, []),
    'gprn_create': (c_int, [POINTER(c_void_p), c_int]),
    'gprn_destroy': (None, [c_void_p]),
    'gprn_last_error': (c_char_p, [c_void_p]),
    'gprn_last_info_gp': (c_int, [c_void_p]),
    'gprn_set_data': (c_int, [c_void_p, c_int, c_int, c_int, _dp, _dp, _dp]),
    'gprn_set_mask': (c_int, [c_void_p, c_void_p]),
    'gprn_set_sweep_order': (c_int, [c_void_p, c_int]),
    'gprn_comm_unique_id': (c_int, [POINTER(c_char)]),
    'gprn_comm_init': (c_int, [c_void_p, c_int, c_int, POINTER(c_char)]),
    'gprn_set_owners': (c_int, [c_void_p, POINTER(c_int)]),
    'gprn_comm_barrier_max': (c_int, [c_void_p, _dp]),
    'gprn_set_kernel': (c_int, [c_void_p, c_int, POINTER(c_int32), c_int, _dp, c_int, c_int]),
    'gprn_upload_K': (c_int, [c_void_p, c_int, _dp]),
    'gprn_set_y_resid': (c_int, [c_void_p, _dp]),
    'gprn_set_jitters': (c_int, [c_void_p, _dp]),
    'gprn_factor_priors': (c_int, [c_void_p]),
    'gprn_set_muvar': (c_int, [c_void_p, _dp, _dp]),
    'gprn_get_muvar': (c_int, [c_void_p, _dp, _dp]),
    'gprn_set_mean': (c_int, [c_void_p, c_int, POINTER(c_int32), c_int, _dp, c_int]),
    'gprn_eval_mean': (c_int, [c_void_p, c_int, _dp, c_int, c_int, _dp, _dp]),
    'gprn_eval_mean_grad': (c_int, [c_void_p, c_int, _dp, c_int, c_int, _dp, _dp]),
    'gprn_sweep': (c_int, [c_void_p, c_int, c_int, _dp, _dp]),
    'gprn_predict': (c_int, [c_void_p, c_int, _dp, _dp, _dp]),
    'gprn_predict_upload': (c_int, [c_void_p, c_int, c_int, _dp, _dp, _dp]),
    'gprn_predict_cov': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp]),
    'gprn_predict_draws': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp, _dp]),
    'gprn_predict_upload_kss': (c_int, [c_void_p, c_int, c_int, _dp]),
    'gprn_get_scalars': (c_int, [c_void_p, _dp]),
    'gprn_keep_sigma': (c_int, [c_void_p, c_int]),
    'gprn_get_matrix': (c_int, [c_void_p, c_int, c_int, _dp]),
    'gprn_get_logdet_K': (c_int, [c_void_p, _dp]),
    'gprn_profile_enable': (c_int, [c_void_p, c_int]),
    'gprn_profile_read': (c_int, [c_void_p, _dp, POINTER(c_int64), c_int]),
    'gprn_test_gemm': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, _dp, _dp, _dp]),
    'gprn_comm_allreduce_sum': (c_int, [c_void_p, _dp, c_int]),
    'gprn_test_factor_invert': (c_int, [c_void_p, c_int, c_int, _dp, _dp, _dp]),
    'gprn_test_lauum': (c_int, [c_void_p, c_int, _dp, _dp]),
    'gprn_test_gemm_rate': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, _dp]),
    'gprn_test_fill_rate': (c_int, [c_void_p, c_int, _dp]),
    'gprn_test_mfma_peak': (c_int, [c_void_p, c_int, c_int, _dp]),
    'gprn_test_tile_launch': (c_int, [c_void_p, c_int, c_int, _dp, c_int, POINTER(c_int64), c_int, c_int, c_int, _dp, c_int,
                              c_int]),
    'gprn_test_tile_step': (c_int, [c_void_p, c_int, _dp, c_int, c_int, c_int, c_int, POINTER(c_int64)]),
    'gprn_set_option': (c_int, [c_void_p, c_char_p, c_int, POINTER(c_int)]),
    'gprn_elbocalc_batch': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp, _dp, c_int, _dp, POINTER(c_int), POINTER(c_int),
                            POINTER(c_int), _dp, _dp]),
    'gprn_elbocalc_batch_grad': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp, _dp, c_int, c_int, _dp, POINTER(c_int),
                                 POINTER(c_int), POINTER(c_int), _dp, _dp, _dp]),
    'gprn_elbocalc_batch_means': (c_int, [c_void_p, c_int, _dp, c_int, _dp, c_int, _dp, _dp, _dp, c_int, c_int, _dp, POINTER(c_int),
                                  POINTER(c_int), POINTER(c_int), _dp, _dp, _dp, _dp, _dp]),
    'gprn_elbocalc_batch_predict': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp, _dp, c_int, c_int, c_int, _dp, _dp,
                                            POINTER(c_int), POINTER(c_int), POINTER(c_int), _dp, _dp, _dp, _dp, _dp, _dp]),
    'gprn_elbocalc_batch_draws': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp, _dp, c_int, c_int, c_int, _dp, c_int, _dp, _dp,
                                          POINTER(c_int), POINTER(c_int), POINTER(c_int), _dp, _dp, _dp, _dp, _dp, POINTER(c_int)]),
    'gprn_elbocalc_batch_heldout': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp, _dp, c_int, c_int, c_void_p, _dp,
                                            POINTER(c_int), POINTER(c_int), POINTER(c_int), _dp, _dp, _dp, _dp, _dp,
                                            POINTER(c_int)]),
    'gprn_predict_batch': (c_int, [c_void_p, c_int, _dp, c_int, _dp, _dp, _dp, c_int, _dp, _dp, _dp, _dp, _dp, POINTER(c_int)]),
    'gprn_test_predict_fill': (c_int, [c_void_p, c_int, c_int, _dp, c_int, _dp, c_int, c_int, c_int, _dp, _dp, _dp, _dp]),
    'gprn_test_fill_rect': (c_int, [c_void_p, POINTER(c_int32), c_int, _dp, c_int, c_double, c_int, c_int, c_int, _dp, _dp, _dp,
                            _dp]),
    'gprn_elbocalc': (c_int, [c_void_p, c_int, _dp, _dp, _dp, _dp, c_int, _dp, c_int, POINTER(c_int), POINTER(c_int),
                      POINTER(c_int), _dp, _dp]),
    'gprn_expected_loglike': (c_int, [c_void_p, _dp]),
    'gprn_prior_terms': (c_int, [c_void_p, c_int, _dp, _dp, _dp]),
    'gprn_grad_matrices': (c_int, [c_void_p, c_int, _dp, _dp]),
    'gprn_grad_kernel': (c_int, [c_void_p, c_int, _dp, _dp]),
    'gprn_grad_elbo': (c_int, [c_void_p, _dp, c_int]),
    'gprn_grad_matrix': (c_int, [c_void_p, c_int, _dp]),
    'gprn_eval_kernel': (c_int, [c_void_p, POINTER(c_int32), c_int, _dp, c_int, c_double, _dp]),
    'gprn_eval_kernel_grad': (c_int, [c_void_p, POINTER(c_int32), c_int, _dp, c_int, _dp]),
    'gprn_sample_prior': (c_int, [c_void_p, POINTER(c_int32), c_int, _dp, c_int, c_double, c_int, _dp, _dp]),
}

_lib = None


def load_library():
    """dlopen the in-tree library and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendUnavailable(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; '
            f'g.build()"` (or make -C gpyrn_amd/csrc)')
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as exc:
        raise BackendUnavailable(f'cannot load {LIB_PATH}: {exc}') from exc
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_count():
    return int(load_library().gprn_device_count())


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f'expected shape {tuple(shape)}, got {a.shape}')
    return a


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _ip(a):
    return a.ctypes.data_as(POINTER(c_int))


def _opt(a):
    return None if a is None else _ptr(a)


# what the side-by-side wrappers (Context.elbocalc_batch*, predict_batch) share.  Plain functions of anything that has
# p, q and N: the wrappers are also called unbound, on an object that holds the sizes and no handle.
def _batch_inputs(ctx, kernel_params, mu, var, y_resid=None, jitters=None):
    """kernel_params (B, n_kpar), mu / var (B, d) and, where given, y_resid (B, p, N) and jitters (B, p), checked and made
    contiguous: ``(kp, yr, jt, m0, v0)``.  A ``MeanParams`` becomes y - mean through gprn_eval_mean: the entry points that
    come here take a host array."""
    kp = _f64(kernel_params)
    if kp.ndim != 2 or kp.shape[0] < 1:
        raise ValueError(f'kernel_params must be (B, n_kpar), got {kp.shape}')
    B = kp.shape[0]
    d = (ctx.p + 1) * ctx.q * ctx.N
    if isinstance(y_resid, MeanParams):
        y_resid = y_resid.host_resid(ctx)
    yr, jt = (None if a is None else _f64(a) for a in (y_resid, jitters))
    m0, v0 = _f64(mu), _f64(var)
    if yr is not None and yr.size != B * ctx.p * ctx.N:
        raise ValueError(f'y_resid must be (B, p, N) = ({B}, {ctx.p}, {ctx.N}), got {yr.shape}')
    if jt is not None and jt.size != B * ctx.p:
        raise ValueError(f'jitters must be (B, p) = ({B}, {ctx.p}), got {jt.shape}')
    if m0.size != B * d or v0.size != B * d:
        raise ValueError(f'mu and var must hold (B, d) = ({B}, {d}) values each, got {m0.shape} and {v0.shape}')
    return kp, yr, jt, m0, v0


def _batch_outputs(ctx, B, want_state=True):
    """The six outputs every gprn_elbocalc_batch* entry fills: ``(elbo, iterations, converged, info, mu_out, var_out)``."""
    d = (ctx.p + 1) * ctx.q * ctx.N
    elbo = np.empty(B)
    it, cv, info = (np.zeros(B, dtype=np.int32) for _ in range(3))
    mo = np.empty((B, d)) if want_state else None
    vo = np.empty((B, d)) if want_state else None
    return elbo, it, cv, info, mo, vo


def _batch_result(ctx, rc, what, outs, *tail):
    """What a gprn_elbocalc_batch* wrapper returns: None where the library has no side-by-side form, else ``outs`` (as
    ``_batch_outputs`` made them) as (elbo, iterations, converged, info[, states (B, p+1, q, N) twice]), then ``tail``."""
    if rc == GPRN_E_UNSUPPORTED:
        return None
    ctx._check(rc, what)
    elbo, it, cv, info, mo, vo = outs
    head = (elbo, it.astype(int), cv.astype(bool), info.astype(int))
    if mo is not None:
        shape = (elbo.size, ctx.p + 1, ctx.q, ctx.N)
        head += (mo.reshape(shape), vo.reshape(shape))
    return head + tail


def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    rc = load_library().gprn_comm_unique_id(buf)
    if rc:
        raise BackendError(f'gprn_comm_unique_id failed ({rc}): is librccl present?')
    return buf.raw


class Context:
    """One GPU.  Mirrors the C handle; methods map 1:1 onto the C entry points."""

    def __init__(self, device=0):
        self._h = None
        self._lib = load_library()
        h = c_void_p()
        rc = self._lib.gprn_create(byref(h), int(device))
        if rc == GPRN_E_NODEV:
            raise BackendUnavailable('no HIP device visible: gpyrn_amd has no CPU path '
                                     '(the NumPy oracle lives in oracle/, for tests only)')
        if rc:
            raise BackendError(f'gprn_create({device}) failed with {rc}')
        self._h = h
        self.device = int(device)
        self.N = self.p = self.q = self.G = 0
        self.world, self.rank = 1, 0

    def close(self):
        if self._h is not None:
            self._lib.gprn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- status ------------------------------------------------------------
    def _check(self, rc, what):
        """Negative codes raise; a positive code is a LAPACK-style info and is returned."""
        if rc < 0:
            msg = self._lib.gprn_last_error(self._h)
            raise BackendError(f'{what}: {msg.decode() if msg else rc} (code {rc})')
        return rc

    @property
    def last_info_gp(self):
        return int(self._lib.gprn_last_info_gp(self._h))

    # -- problem -----------------------------------------------------------
    def set_data(self, time, y, yerr, q):
        time = _f64(time)
        y = _f64(y)
        yerr = _f64(yerr, y.shape)
        p, N = y.shape
        if time.shape != (N,):
            raise ValueError('time and y disagree')
        self._check(self._lib.gprn_set_data(self._h, N, p, int(q), _ptr(time), _ptr(y), _ptr(yerr)),
                    'set_data')
        self.N, self.p, self.q, self.G = N, p, int(q), int(q) * (p + 1)

    def set_mask(self, mask):
        """(p, N) truthy = observed, or None to clear (gprn_set_mask)."""
        if mask is None:
            self._check(self._lib.gprn_set_mask(self._h, None), 'set_mask')
            return
        m = np.ascontiguousarray(np.asarray(mask, dtype=bool), dtype=np.uint8)
        if m.shape != (self.p, self.N):
            raise ValueError(f'expected shape {(self.p, self.N)}, got {m.shape}')
        self._check(self._lib.gprn_set_mask(self._h, m.ctypes.data_as(c_void_p)), 'set_mask')

    def set_sweep_order(self, order):
        """ORDER_REFERENCE (0: the reference's Jacobi ordering) or ORDER_SEQUENTIAL (1) for every following sweep
        (gprn_set_sweep_order)."""
        self._check(self._lib.gprn_set_sweep_order(self._h, int(order)), 'set_sweep_order')

    def comm_init(self, world, rank, unique_id):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128) if unique_id else None
        self._check(self._lib.gprn_comm_init(self._h, int(world), int(rank), buf), 'comm_init')
        self.world, self.rank = int(world), int(rank)

    def set_owners(self, owner):
        arr = (c_int * self.G)(*[int(o) for o in owner])
        self._check(self._lib.gprn_set_owners(self._h, arr), 'set_owners')
        self._owner = [int(o) for o in owner]

    def owner_of(self, gp):
        """Rank that factors latent GP `gp` (0 on an unsharded context)."""
        owner = getattr(self, '_owner', None)
        return owner[gp] if owner else 0

    def barrier_max(self, value=0.0):
        v = c_double(float(value))
        self._check(self._lib.gprn_comm_barrier_max(self._h, byref(v)), 'barrier_max')
        return v.value

    def allreduce_sum(self, values):
        """Sum of a float64 vector over the ranks of this context's communicator."""
        buf = np.array(values, dtype=np.float64).ravel()
        self._check(self._lib.gprn_comm_allreduce_sum(self._h, _ptr(buf), buf.size), 'allreduce_sum')
        return buf

    def set_kernel(self, gp, ops, params, add_nugget):
        flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 3))
        par = _f64(np.atleast_1d(params))
        self._check(self._lib.gprn_set_kernel(
            self._h, int(gp), flat.ctypes.data_as(POINTER(c_int32)), flat.shape[0],
            _ptr(par), par.size, int(bool(add_nugget))), 'set_kernel')

    def set_mean(self, output, ops, params):
        """The mean program of `output` (gprn_set_mean; meanfunc's ``_device_program``); ops None or empty: no mean."""
        flat = np.ascontiguousarray(np.asarray(ops if ops is not None else [], dtype=np.int32).reshape(-1, 3))
        par = _f64(np.atleast_1d(params)) if flat.shape[0] else np.zeros(0)
        self._check(self._lib.gprn_set_mean(self._h, int(output), flat.ctypes.data_as(POINTER(c_int32)), flat.shape[0],
                                            _ptr(par), par.size), 'set_mean')

    def _eval_mean(self, fn, what, mean_params, t, rows):
        mp = np.atleast_2d(_f64(mean_params))
        ts = None if t is None else _f64(np.atleast_1d(t))
        nt = self.N if ts is None else ts.size
        out = np.empty((mp.shape[0], rows(mp.shape[1]), nt))
        self._check(fn(self._h, mp.shape[0], _ptr(mp), mp.shape[1], nt, None if ts is None else _ptr(ts), _ptr(out)), what)
        return out

    def eval_mean(self, mean_params, t=None):
        """The outputs' means under B parameter rows (B, n_mean_params) at the times t (None: the data's), (B, p, nt):
        gprn_eval_mean."""
        return self._eval_mean(self._lib.gprn_eval_mean, 'eval_mean', mean_params, t, lambda n: self.p)

    def eval_mean_grad(self, mean_params, t=None):
        """d mean / d every mean parameter, (B, n_mean_params, nt): gprn_eval_mean_grad."""
        return self._eval_mean(self._lib.gprn_eval_mean_grad, 'eval_mean_grad', mean_params, t, lambda n: n)

    def upload_K(self, gp, K):
        K = _f64(K, (self.N, self.N))
        self._check(self._lib.gprn_upload_K(self._h, int(gp), _ptr(K)), 'upload_K')

    def set_y_resid(self, y):
        y = _f64(y, (self.p, self.N))
        self._check(self._lib.gprn_set_y_resid(self._h, _ptr(y)), 'set_y_resid')

    def set_jitters(self, jitters):
        j = _f64(np.atleast_1d(jitters), (self.p,))
        self._check(self._lib.gprn_set_jitters(self._h, _ptr(j)), 'set_jitters')

    def factor_priors(self):
        return self._check(self._lib.gprn_factor_priors(self._h), 'factor_priors')

    def set_muvar(self, mu, var):
        d = self.N * self.q * (self.p + 1)
        mu = _f64(np.ravel(mu), (d,))
        var = _f64(np.ravel(var), (d,))
        self._check(self._lib.gprn_set_muvar(self._h, _ptr(mu), _ptr(var)), 'set_muvar')

    def get_muvar(self):
        shape = (self.p + 1, self.q, self.N)
        mu, var = np.empty(shape), np.empty(shape)
        self._check(self._lib.gprn_get_muvar(self._h, _ptr(mu), _ptr(var)), 'get_muvar')
        return mu, var

    def sweep(self, n=1, commit=True):
        """n x ELBOaux.  Returns (elbo[n], parts[n,3] = LogL, LogP, Ent, info)."""
        elbo = np.empty(n)
        parts = np.empty((n, 3))
        info = self._check(self._lib.gprn_sweep(self._h, int(n), int(bool(commit)),
                                                _ptr(elbo), _ptr(parts)), 'sweep')
        return elbo, parts, info

    def predict(self, tstar):
        """Conditional mean / variance of every latent GP at `tstar`: two (G, n*) arrays (complete on
        every rank of a sharded context) and the LAPACK-style info."""
        ts = _f64(np.ravel(tstar))
        mean = np.zeros((self.G, ts.size))
        var = np.zeros((self.G, ts.size))
        info = self._check(self._lib.gprn_predict(self._h, ts.size, _ptr(ts), _ptr(mean), _ptr(var)),
                           'predict')
        return mean, var, info

    def predict_upload(self, gp, K_tiny, Kstar, kss):
        """Host-evaluated K + 1.25e-12 I (N, N), K* (n*, N) and k** (n*) of latent GP `gp` for the next predict()."""
        K_tiny = _f64(K_tiny, (self.N, self.N))
        Kstar = _f64(np.atleast_2d(Kstar))
        if Kstar.shape[1] != self.N:
            raise ValueError('Kstar must have N columns')
        kss = _f64(np.ravel(kss), (Kstar.shape[0],))
        self._check(self._lib.gprn_predict_upload(self._h, int(gp), Kstar.shape[0], _ptr(K_tiny), _ptr(Kstar),
                                                  _ptr(kss)), 'predict_upload')

    def predict_upload_kss(self, gp, Kss):
        """Host-evaluated K** (n*, n*) of latent GP `gp` for the next predict_cov() / predict_draws()."""
        Kss = _f64(np.atleast_2d(Kss))
        if Kss.shape[0] != Kss.shape[1]:
            raise ValueError('Kss must be square')
        self._check(self._lib.gprn_predict_upload_kss(self._h, int(gp), Kss.shape[0], _ptr(Kss)), 'predict_upload_kss')

    def predict_cov(self, tstar, joint=False, latent=True, outputs=True):
        """Latent means (G, n*), latent covariances (G, n*, n*) or None, and the per-output covariance -- (p, n*, n*), or
        (p n*, p n*) with `joint` -- or None (gprn_predict_cov; the jitters last set)."""
        ts = _f64(np.ravel(tstar))
        ns = ts.size
        mean = np.zeros((self.G, ns))
        lat = np.empty((self.G, ns, ns)) if latent else None
        out = (np.empty((self.p * ns, self.p * ns)) if joint else np.empty((self.p, ns, ns))) if outputs else None
        self._check(self._lib.gprn_predict_cov(self._h, ns, _ptr(ts), COV_JOINT if joint else 0, _ptr(mean),
                                               _ptr(lat) if latent else None, _ptr(out) if outputs else None),
                    'predict_cov')
        return mean, lat, out

    def predict_draws(self, tstar, z, outputs=True):
        """Joint posterior draws from standard normals z (G, n, n*): (latent draws (G, n, n*), sum_j w o f per output
        (p, n, n*) or None, the nugget of every latent GP (G), info)."""
        ts = _f64(np.ravel(tstar))
        ns = ts.size
        z = _f64(z)
        if z.ndim != 3 or z.shape[0] != self.G or z.shape[2] != ns:
            raise ValueError(f'z must be (G, n, n*) = ({self.G}, n, {ns})')
        nd = z.shape[1]
        lat = np.empty((self.G, nd, ns))
        out = np.empty((self.p, nd, ns)) if outputs else None
        nug = np.zeros(self.G)
        info = self._check(self._lib.gprn_predict_draws(self._h, ns, _ptr(ts), nd, _ptr(z), _ptr(lat),
                                                        _ptr(out) if outputs else None, _ptr(nug)), 'predict_draws')
        return lat, out, nug, info

    def get_scalars(self):
        """Per-GP scalars of the last sweep: dict of log det B (G), tr B^-1 (G), m^T K^-1 m (G), Q1 traces (q, q)."""
        out = np.empty(3 * self.G + self.q * self.q)
        self._check(self._lib.gprn_get_scalars(self._h, _ptr(out)), 'get_scalars')
        G = self.G
        return {'logdetB': out[:G].copy(), 'trBinv': out[G:2 * G].copy(), 'muKmu': out[2 * G:3 * G].copy(),
                'q1': out[3 * G:].reshape(self.q, self.q).copy()}

    def eval_kernel(self, ops, params, nugget):
        """K = expr(t_i, t_j) + nugget I at the data times, filled on the device."""
        flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 3))
        par = _f64(np.atleast_1d(params))
        K = np.empty((self.N, self.N))
        self._check(self._lib.gprn_eval_kernel(self._h, flat.ctypes.data_as(POINTER(c_int32)), flat.shape[0],
                                               _ptr(par), par.size, float(nugget), _ptr(K)), 'eval_kernel')
        return K

    def eval_kernel_grad(self, ops, params):
        """dK/dparams[l] of expr(t_i, t_j) at the data times, (n_params, N, N): the exact parameter derivatives of the
        kernel program, evaluated on the device; each matrix symmetric to the bit, the nugget not differentiated."""
        flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 3))
        par = _f64(np.atleast_1d(params))
        dK = np.empty((par.size, self.N, self.N))
        self._check(self._lib.gprn_eval_kernel_grad(self._h, flat.ctypes.data_as(POINTER(c_int32)), flat.shape[0],
                                                    _ptr(par), par.size, _ptr(dK)), 'eval_kernel_grad')
        return dK

    def sample_prior(self, ops, params, nugget, z):
        """L z for every row z of standard normals, K + nugget I = L L^T; returns (samples, info)."""
        flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 3))
        par = _f64(np.atleast_1d(params))
        z = _f64(np.atleast_2d(z))
        if z.shape[1] != self.N:
            raise ValueError('z must have N columns')
        out = np.empty_like(z)
        info = self._check(self._lib.gprn_sample_prior(
            self._h, flat.ctypes.data_as(POINTER(c_int32)), flat.shape[0], _ptr(par), par.size, float(nugget),
            z.shape[0], _ptr(z), _ptr(out)), 'sample_prior')
        return out, info

    def expected_loglike(self):
        """inference._expectedLogLike of the state and jitters last set (gprn_expected_loglike)."""
        v = c_double(0.0)
        self._check(self._lib.gprn_expected_loglike(self._h, byref(v)), 'expected_loglike')
        return v.value

    def prior_terms(self, gp, S, m):
        """(log det K_gp, m^T K_gp^-1 m, tr(K_gp^-1 S)) from the resident factor of K_gp (gprn_prior_terms)."""
        S = _f64(S, (self.N, self.N))
        m = _f64(np.ravel(m), (self.N,))
        out = np.zeros(3)
        self._check(self._lib.gprn_prior_terms(self._h, int(gp), _ptr(S), _ptr(m), _ptr(out)), 'prior_terms')
        return out

    def grad_matrices(self, gp):
        """(K^-1, K^-1 S K^-1) of latent GP `gp` after a sweep with keep_sigma: the N^3 part of the ELBO gradient."""
        Kinv, P = np.empty((self.N, self.N)), np.empty((self.N, self.N))
        self._check(self._lib.gprn_grad_matrices(self._h, int(gp), _ptr(Kinv), _ptr(P)), 'grad_matrices')
        return Kinv, P

    def grad_kernel(self, gp, m, n_params):
        """Kernel-parameter gradient of latent GP `gp` contracted on the device (closed forms for SE / Periodic /
        QuasiPeriodic, central differences of the kernel program otherwise); None for a latent GP whose matrix
        was uploaded (user-defined kernels) -- use grad_matrices then."""
        m = _f64(np.ravel(m), (self.N,))
        out = np.zeros(max(4, int(n_params)))
        rc = self._lib.gprn_grad_kernel(self._h, int(gp), _ptr(m), _ptr(out))
        if rc == GPRN_E_UNSUPPORTED:           # every other error (sharded context, no Sigma kept, ...) raises
            return None
        self._check(rc, 'grad_kernel')
        return out[:n_params]

    def grad_elbo(self, n_params):
        """d/dtheta of the expected log prior of the last committed sweep for every kernel parameter of every latent GP
        with a device program, one call (gprn_grad_elbo: the B-form, no keep_sigma); `n_params`: their number.  NOT
        divided by q."""
        out = np.zeros(max(1, int(n_params)))
        self._check(self._lib.gprn_grad_elbo(self._h, _ptr(out), int(n_params)), 'grad_elbo')
        return out[:int(n_params)]

    def grad_matrix(self, gp):
        """G = 1/2 (a a^T + M) of latent GP `gp` after a committed sweep, (N, N) symmetric: what meets dK/dtheta
        (gprn_grad_matrix; for kernels the caller differentiates)."""
        out = np.empty((self.N, self.N))
        self._check(self._lib.gprn_grad_matrix(self._h, int(gp), _ptr(out)), 'grad_matrix')
        return out

    def keep_sigma(self, on=True):
        self._check(self._lib.gprn_keep_sigma(self._h, int(bool(on))), 'keep_sigma')

    def get_matrix(self, which, gp):
        out = np.empty((self.N, self.N))
        self._check(self._lib.gprn_get_matrix(self._h, int(which), int(gp), _ptr(out)), 'get_matrix')
        return out

    def get_logdet_K(self):
        out = np.empty(self.G)
        self._check(self._lib.gprn_get_logdet_K(self._h, _ptr(out)), 'get_logdet_K')
        return out

    def elbocalc(self, max_iter, setup=False, y_resid=None, jitters=None, mu=None, var=None):
        """ELBOcalc from its set-up block on (meanfield.py:618-649) in one call of the library: optionally the set-up
        with the kernels last sent, y - mean, the jitters and the starting state (None: as set before), then the loop.
        Returns (elboArray, iterNumber, converged, info, mu, var) with the state the loop ended in."""
        cap = int(min(max_iter, 1 << 20)) + 1
        hist = np.empty(cap)
        d = (self.p + 1) * self.q * self.N
        mu_out, var_out = np.empty(d), np.empty(d)
        n, it, conv = c_int(0), c_int(0), c_int(0)
        keep = [None if a is None else _f64(np.ravel(a)) for a in (y_resid, jitters, mu, var)]
        ptrs = [None if a is None else _ptr(a) for a in keep]
        if (keep[0] is not None and keep[0].size != self.p * self.N) or (keep[1] is not None and keep[1].size != self.p) or \
                (keep[2] is not None and (keep[2].size != d or keep[3] is None or keep[3].size != d)):
            raise ValueError('elbocalc: y_resid (p, N), jitters (p,), mu and var (d,) expected')
        info = self._check(self._lib.gprn_elbocalc(self._h, 1 if setup else 0, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                                   int(max_iter), _ptr(hist), cap, byref(n), byref(it), byref(conv),
                                                   _ptr(mu_out), _ptr(var_out)), 'elbocalc')
        shape = (self.p + 1, self.q, self.N)
        return (hist[:min(n.value, cap)].copy(), it.value, bool(conv.value), info,
                mu_out.reshape(shape), var_out.reshape(shape))

    def elbocalc_batch(self, kernel_params, y_resid, jitters, mu, var, max_iter, want_state=False, want_grad=False,
                       forced=False):
        """B independent ELBOcalc loops side by side (gprn_elbocalc_batch): kernel_params (B, n_kpar), y_resid (B, p, N),
        jitters (B, p), mu / var (B, d).  Returns (elbo[B], iterations[B], converged[B], info[B]) and, with want_state,
        the final states (B, p+1, q, N) twice -- or None where the library has no batched form for this problem.
        want_grad (gprn_elbocalc_batch_grad): the tuple ends with grads (B, n_kpar), row b what grad_elbo returns after
        evaluation b's loop alone (NOT divided by q; zeros where info > 0).  forced (GPRN_BATCH_FORCED): no stop rule,
        exactly max_iter committed sweeps per evaluation."""
        kp = _f64(np.atleast_2d(kernel_params))
        B = kp.shape[0]
        d = (self.p + 1) * self.q * self.N
        means = y_resid if isinstance(y_resid, MeanParams) else None
        yr = None if means is not None else _f64(np.reshape(y_resid, (B, self.p * self.N)))
        jt = _f64(np.reshape(jitters, (B, self.p)))
        m0, v0 = _f64(np.reshape(mu, (B, d))), _f64(np.reshape(var, (B, d)))
        outs = elbo, it, cv, info, mo, vo = _batch_outputs(self, B, want_state)
        grads = np.zeros((B, kp.shape[1])) if want_grad else None
        if means is not None:
            means.resid = np.empty((B, self.p * self.N))
            means.mean_grad = np.zeros((B, means.params.shape[1])) if means.want_mean_grad and want_grad else None
            rc = self._lib.gprn_elbocalc_batch_means(self._h, B, _ptr(kp), kp.shape[1], _ptr(means.params), means.params.shape[1],
                                                     _ptr(jt), _ptr(m0), _ptr(v0), int(max_iter),
                                                     GPRN_BATCH_FORCED if forced else 0, _ptr(elbo), _ip(it), _ip(cv),
                                                     _ip(info), _opt(mo), _opt(vo), _opt(grads), _ptr(means.resid),
                                                     _opt(means.mean_grad))
        elif want_grad or forced:
            rc = self._lib.gprn_elbocalc_batch_grad(self._h, B, _ptr(kp), kp.shape[1], _ptr(yr), _ptr(jt), _ptr(m0), _ptr(v0),
                                                    int(max_iter), GPRN_BATCH_FORCED if forced else 0, _ptr(elbo), _ip(it),
                                                    _ip(cv), _ip(info), _opt(mo), _opt(vo), _opt(grads))
        else:
            rc = self._lib.gprn_elbocalc_batch(self._h, B, _ptr(kp), kp.shape[1], _ptr(yr), _ptr(jt), _ptr(m0), _ptr(v0),
                                               int(max_iter), _ptr(elbo), _ip(it), _ip(cv), _ip(info), _opt(mo), _opt(vo))
        return _batch_result(self, rc, 'elbocalc_batch', outs, *((grads,) if want_grad else ()))

    def elbocalc_batch_predict(self, kernel_params, y_resid, jitters, mu, var, max_iter, tstar, forced=False, latent=True,
                               outputs=True):
        """B independent ELBOcalc loops side by side, each followed by the prediction of the posterior it leaves
        (gprn_elbocalc_batch_predict): the arrays of ``elbocalc_batch``, tstar (n*).  Returns (elbo, iterations, converged,
        info, mu_out, var_out, lat_mean, lat_var, out_mean, out_var): the first six what ``elbocalc_batch(want_state=True)``
        returns, to the bit; the latent rows (B, G, n*) -- row b what ``predict()`` returns in the posterior form right after
        ``elbocalc`` ran vector b's loop alone from (mu_b, var_b) -- or None without `latent`; the per-output combination
        with the jitter once and without the mean functions, (B, p, n*), or None without `outputs`.  Rows of an evaluation
        with info > 0 are NaN.  forced (GPRN_BATCH_FORCED): no stop rule, exactly max_iter committed sweeps each.  None
        where the library has no side-by-side form for this problem."""
        if not (latent or outputs):
            raise ValueError('elbocalc_batch_predict: ask for the latent pair, the output pair or both')
        kp, yr, jt, m0, v0 = _batch_inputs(self, kernel_params, mu, var, y_resid, jitters)
        B = kp.shape[0]
        ts = _f64(np.ravel(tstar))
        if ts.size < 1:
            raise ValueError('tstar is empty')
        if int(max_iter) < 1:
            raise ValueError('elbocalc_batch_predict: a prediction needs a committed sweep (max_iter >= 1)')
        ns = ts.size
        outs = elbo, it, cv, info, mo, vo = _batch_outputs(self, B)
        lm = np.empty((B, self.G, ns)) if latent else None
        lv = np.empty((B, self.G, ns)) if latent else None
        om = np.empty((B, self.p, ns)) if outputs else None
        ov = np.empty((B, self.p, ns)) if outputs else None
        rc = self._lib.gprn_elbocalc_batch_predict(self._h, B, _ptr(kp), kp.shape[1], _ptr(yr), _ptr(jt), _ptr(m0), _ptr(v0),
                                                   int(max_iter), GPRN_BATCH_FORCED if forced else 0, ns, _ptr(ts), _ptr(elbo),
                                                   _ip(it), _ip(cv), _ip(info), _ptr(mo), _ptr(vo), _opt(lm), _opt(lv),
                                                   _opt(om), _opt(ov))
        return _batch_result(self, rc, 'elbocalc_batch_predict', outs, lm, lv, om, ov)

    def elbocalc_batch_heldout(self, kernel_params, y_resid, jitters, mu, var, max_iter, fit_masks, forced=False, rows=True):
        """B independent ELBOcalc loops side by side, evaluation b fitted under its OWN mask fit_masks[b] (p, N; True = fitted),
        each followed by the score of what it held out (gprn_elbocalc_batch_heldout): the arrays of ``elbocalc_batch``.
        Returns (elbo, iterations, converged, info, mu_out, var_out, held_mean, held_var, lpd, n_held): the first six what
        ``elbocalc`` returns on a context masked with fit_masks[b]; the predictive mean (without the mean functions) and
        variance of every held-out entry, (B, p, N), zero elsewhere -- or None without `rows`; the log predictive density
        summed over the held-out entries of each output, (B, p), and their number.  Rows of an evaluation with info > 0 are
        NaN.  forced (GPRN_BATCH_FORCED): no stop rule, exactly max_iter committed sweeps each.  None where the library has
        no side-by-side form for this problem."""
        kp, yr, jt, m0, v0 = _batch_inputs(self, kernel_params, mu, var, y_resid, jitters)
        B = kp.shape[0]
        fm = np.asarray(fit_masks)
        if fm.shape != (B, self.p, self.N):
            raise ValueError(f'fit_masks must be (B, p, N) = ({B}, {self.p}, {self.N}), got {fm.shape}')
        fm = np.ascontiguousarray(fm != 0, dtype=np.uint8)
        if int(max_iter) < 1:
            raise ValueError('elbocalc_batch_heldout: a held-out score needs a committed sweep (max_iter >= 1)')
        outs = elbo, it, cv, info, mo, vo = _batch_outputs(self, B)
        hm = np.empty((B, self.p, self.N)) if rows else None
        hv = np.empty((B, self.p, self.N)) if rows else None
        lpd = np.empty((B, self.p))
        nh = np.zeros((B, self.p), dtype=np.int32)
        rc = self._lib.gprn_elbocalc_batch_heldout(self._h, B, _ptr(kp), kp.shape[1], _ptr(yr), _ptr(jt), _ptr(m0), _ptr(v0),
                                                   int(max_iter), GPRN_BATCH_FORCED if forced else 0, fm.ctypes.data,
                                                   _ptr(elbo), _ip(it), _ip(cv), _ip(info), _ptr(mo), _ptr(vo), _opt(hm),
                                                   _opt(hv), _ptr(lpd), _ip(nh))
        return _batch_result(self, rc, 'elbocalc_batch_heldout', outs, hm, hv, lpd, nh.astype(int))

    def elbocalc_batch_draws(self, kernel_params, y_resid, jitters, mu, var, max_iter, tstar, z, forced=False, latent=True,
                             outputs=True):
        """B independent ELBOcalc loops side by side, each followed by joint draws from the posterior it leaves
        (gprn_elbocalc_batch_draws): the arrays of ``elbocalc_batch``, tstar (n*), the standard normals z (B, G, n, n*).
        Returns (elbo, iterations, converged, info, mu_out, var_out, lat_draws, out_draws, nuggets, draw_info): the first six
        what ``elbocalc_batch(want_state=True)`` returns, to the bit; the latent draws (B, G, n, n*) -- row b what
        ``predict_draws()`` returns in the posterior form right after ``elbocalc`` ran vector b's loop alone from
        (mu_b, var_b), with z_b -- or None without `latent`; sum_j w o f per output, (B, p, n, n*), without mean functions
        and noise, or None without `outputs`; the nugget of every (vector, latent GP), (B, G); draw_info (B,), > 0 where a
        vector's last rung failed.  Rows of an evaluation with info > 0 or draw_info > 0 are NaN.  forced
        (GPRN_BATCH_FORCED): no stop rule, exactly max_iter committed sweeps each.  None where the library has no
        side-by-side form for this problem."""
        if not (latent or outputs):
            raise ValueError('elbocalc_batch_draws: ask for the latent draws, the output draws or both')
        kp, yr, jt, m0, v0 = _batch_inputs(self, kernel_params, mu, var, y_resid, jitters)
        B = kp.shape[0]
        ts = _f64(np.ravel(tstar))
        if ts.size < 1:
            raise ValueError('tstar is empty')
        ns = ts.size
        z = _f64(z)
        if z.ndim != 4 or z.shape[0] != B or z.shape[1] != self.G or z.shape[2] < 1 or z.shape[3] != ns:
            raise ValueError(f'z must be (B, G, n, n*) = ({B}, {self.G}, n, {ns}), got {z.shape}')
        if int(max_iter) < 1:
            raise ValueError('elbocalc_batch_draws: a draw needs a committed sweep (max_iter >= 1)')
        nd = z.shape[2]
        outs = elbo, it, cv, info, mo, vo = _batch_outputs(self, B)
        dinfo = np.zeros(B, dtype=np.int32)
        lat = np.empty((B, self.G, nd, ns)) if latent else None
        out = np.empty((B, self.p, nd, ns)) if outputs else None
        nug = np.zeros((B, self.G))
        rc = self._lib.gprn_elbocalc_batch_draws(self._h, B, _ptr(kp), kp.shape[1], _ptr(yr), _ptr(jt), _ptr(m0), _ptr(v0),
                                                 int(max_iter), GPRN_BATCH_FORCED if forced else 0, ns, _ptr(ts), nd, _ptr(z),
                                                 _ptr(elbo), _ip(it), _ip(cv), _ip(info), _ptr(mo), _ptr(vo), _opt(lat),
                                                 _opt(out), _ptr(nug), _ip(dinfo))
        return _batch_result(self, rc, 'elbocalc_batch_draws', outs, lat, out, nug, dinfo.astype(int))

    def predict_batch(self, kernel_params, mu, var, tstar, jitters=None, latent=True, outputs=True):
        """gprn_predict for B parameter vectors side by side (gprn_predict_batch): kernel_params (B, n_kpar), mu / var (B, d)
        -- each evaluation's own state -- jitters (B, p) (needed with `outputs`), tstar (n*).  Returns (lat_mean, lat_var,
        out_mean, out_var, info): the latent rows (B, G, n*) -- row b what predict() returns for vector b and state b alone --
        or None without `latent`; the per-output combination of _Prediction without the mean functions, (B, p, n*), or None
        without `outputs`; info (B,), LAPACK-style per evaluation.  None where the library has no side-by-side form for
        this problem (a communicator, a host-evaluated kernel, a kernel that is not even in t_i - t_j)."""
        if not (latent or outputs):
            raise ValueError('predict_batch: ask for the latent pair, the output pair or both')
        if outputs and jitters is None:
            raise ValueError('predict_batch: the output pair needs the jitters')
        kp, _, jt, m0, v0 = _batch_inputs(self, kernel_params, mu, var, jitters=jitters if outputs else None)
        B = kp.shape[0]
        ts = _f64(np.ravel(tstar))
        if ts.size < 1:
            raise ValueError('tstar is empty')
        ns = ts.size
        lm = np.empty((B, self.G, ns)) if latent else None
        lv = np.empty((B, self.G, ns)) if latent else None
        om = np.empty((B, self.p, ns)) if outputs else None
        ov = np.empty((B, self.p, ns)) if outputs else None
        info = np.zeros(B, dtype=np.int32)
        rc = self._lib.gprn_predict_batch(self._h, B, _ptr(kp), kp.shape[1], _ptr(m0), _ptr(v0), _opt(jt), ns, _ptr(ts),
                                          _opt(lm), _opt(lv), _opt(om), _opt(ov), _ip(info))
        if rc == GPRN_E_UNSUPPORTED:
            return None
        self._check(rc, 'predict_batch')
        return lm, lv, om, ov, info.astype(int)

    def test_predict_fill(self, kernel_params, var, eval_index, gp, tstar, batched):
        """K + 1.25e-12 I + diag(v) (N, N), K* (n*, N) and k** (n*) of slot (eval_index, gp) as gprn_predict_batch fills them
        (`batched`) or as gprn_predict does for that vector alone (gprn_test_predict_fill)."""
        kp = _f64(np.atleast_2d(kernel_params))
        B = kp.shape[0]
        v0 = _f64(np.reshape(var, (B, (self.p + 1) * self.q * self.N)))
        ts = _f64(np.ravel(tstar))
        K, Ks, kss = np.empty((self.N, self.N)), np.empty((ts.size, self.N)), np.empty(ts.size)
        self._check(self._lib.gprn_test_predict_fill(self._h, int(bool(batched)), B, _ptr(kp), kp.shape[1], _ptr(v0),
                                                     int(eval_index), int(gp), ts.size, _ptr(ts), _ptr(K), _ptr(Ks), _ptr(kss)),
                    'test_predict_fill')
        return K, Ks, kss

    def test_fill_rect(self, ops, params, nugget, tstar, form=0, batched=0, s=None):
        """K* and k** of a kernel expression between tstar (rows) and the data times (columns) by one of prediction's four
        rectangular fills (gprn_test_fill_rect): form 0 the reference form, 1 the posterior form K* diag(s); batched 0 the
        single launch, 1 / 2 the batched launch with the caller's program in slot 0 / 1 of two.  Returns the WHOLE padded
        buffers, K* (ns_pad, ld) and k** (ns_pad): NaN wherever the kernel wrote nothing."""
        flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 3))
        par = _f64(np.atleast_1d(params))
        ts = _f64(np.ravel(tstar))
        sv = None if s is None else _f64(np.ravel(s), (self.N,))
        pad = lambda n: -(-n // TILE) * TILE
        Ks, kss = np.empty((pad(ts.size), pad(self.N))), np.empty(pad(ts.size))
        self._check(self._lib.gprn_test_fill_rect(self._h, flat.ctypes.data_as(POINTER(c_int32)), flat.shape[0], _ptr(par),
                                                  par.size, float(nugget), int(form), int(batched), ts.size, _ptr(ts),
                                                  None if sv is None else _ptr(sv), _ptr(Ks), _ptr(kss)), 'test_fill_rect')
        return Ks, kss

    def option(self, name, value=-1):
        """Read (value < 0) or set a per-context switch of the library; returns the previous value.  Among them
        ``'predict_form'`` (PREDICT_REFERENCE / PREDICT_POSTERIOR: what predict, predict_cov and predict_draws compute) and
        the read-only ``'state_ready'`` (1 while a committed sweep's factors are still in the workspaces)."""
        old = c_int(0)
        self._check(self._lib.gprn_set_option(self._h, name.encode(), int(value), byref(old)), 'set_option')
        return old.value

    # -- timing --------------------------------------------------------------
    def profile_enable(self, families=T_NAMES):
        mask = 0
        for f in families or ():
            mask |= 1 << T_NAMES.index(f)
        self._check(self._lib.gprn_profile_enable(self._h, mask), 'profile_enable')

    def profile_read(self, reset=True):
        ms = np.zeros(len(T_NAMES))
        n = np.zeros(len(T_NAMES), dtype=np.int64)
        self._check(self._lib.gprn_profile_read(self._h, _ptr(ms), n.ctypes.data_as(POINTER(c_int64)),
                                                int(bool(reset))), 'profile_read')
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(T_NAMES)}

    # -- diagnostics -----------------------------------------------------------
    def test_gemm(self, A, B, C, a_mode, b_mode, c_mode):
        A, B = _f64(A), _f64(B)
        C = _f64(C).copy()
        M, K = A.shape
        K2, N = B.shape
        assert K == K2 and C.shape == (M, N)
        self._check(self._lib.gprn_test_gemm(self._h, M, N, K, a_mode, b_mode, c_mode,
                                             _ptr(A), _ptr(B), _ptr(C)), 'test_gemm')
        return C

    def test_factor_invert(self, A):
        A = _f64(A)
        if A.ndim == 2:
            A = A[None]
        batch, n, _ = A.shape
        L, X = np.empty_like(A), np.empty_like(A)
        info = self._check(self._lib.gprn_test_factor_invert(self._h, n, batch, _ptr(A), _ptr(L), _ptr(X)),
                           'test_factor_invert')
        return L, X, info

    def gemm_rate(self, M, N, K, how, reps=3):
        """TFLOP/s of C -= A.B^T (M x N x K) through the tile contraction: one launch of 64 x 64 (how 0) / 128 x 128 (how 1)
        workgroups."""
        v = c_double(0.0)
        self._check(self._lib.gprn_test_gemm_rate(self._h, int(M), int(N), int(K), int(how), int(reps), byref(v)), 'test_gemm_rate')
        return 2.0 * M * N * K / (v.value * 1e-3) / 1e12

    def fill_rate(self, reps=20):
        """ms per pass over all local covariance fills (the kernels last sent), timed inside one pair of events."""
        v = c_double(0.0)
        self._check(self._lib.gprn_test_fill_rate(self._h, int(reps), byref(v)), 'test_fill_rate')
        return v.value

    def mfma_peak(self, wg_per_cu=1, iters=2000):
        """Measured fp64 MFMA issue ceiling (TFLOP/s) of this device."""
        v = c_double(0.0)
        self._check(self._lib.gprn_test_mfma_peak(self._h, int(wg_per_cu), int(iters), byref(v)),
                    'test_mfma_peak')
        return v.value

    def test_lauum(self, X):
        X = _f64(X)
        out = np.empty_like(X)
        self._check(self._lib.gprn_test_lauum(self._h, X.shape[0], _ptr(X), _ptr(out)), 'test_lauum')
        return out

    def test_tile_launch(self, bufs, tasks, shape, tag, ldc=0, ft_s=None, ft_n=0, acc=False):
        """One launch of the tile kernel (gprn_test_tile_launch).  bufs: (nbatch, 4, ld, ld); tasks: rows of (c_off, a_off,
        b_off, klen, c_buf, a_buf, b_buf, modes).  Returns every buffer as the launch left it."""
        out = _f64(bufs).copy()
        nbatch, nbuf, ld, ld2 = out.shape
        if nbuf != 4 or ld != ld2:
            raise ValueError(f'expected (nbatch, 4, ld, ld), got {out.shape}')
        t = np.ascontiguousarray(tasks, dtype=np.int64).reshape(-1, 8)
        s = None if ft_s is None else _f64(ft_s, (nbatch, ld))
        self._check(self._lib.gprn_test_tile_launch(self._h, ld, nbatch, _ptr(out), len(t),
                                                    t.ctypes.data_as(POINTER(c_int64)), int(shape), int(tag), int(ldc),
                                                    None if s is None else _ptr(s), int(ft_n), int(bool(acc))),
                    'test_tile_launch')
        return out

    def test_tile_step(self, bufs, which, table=True, tasks=(), n_l=0):
        """One launch of k_chain_l / k_chain_u / k_tile_panel at step 0 of 256 x 256 matrices (gprn_test_tile_step).  bufs:
        (nbatch, 2, 256, 256), B and X; tasks: the panel's list, its first n_l the L part."""
        out = _f64(bufs).copy()
        if out.shape[1:] != (2, 2 * TILE, 2 * TILE):
            raise ValueError(f'expected (nbatch, 2, 256, 256), got {out.shape}')
        t = np.ascontiguousarray(tasks, dtype=np.int64).reshape(-1, 8)
        self._check(self._lib.gprn_test_tile_step(self._h, out.shape[0], _ptr(out), int(which), int(bool(table)), int(n_l),
                                                  len(t) - int(n_l), t.ctypes.data_as(POINTER(c_int64))), 'test_tile_step')
        return out
