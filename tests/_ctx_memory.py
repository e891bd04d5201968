"""What a context takes and gives back, counted: the scenarios of tests/test_ctx_memory_gpu.py and profiles/ctx_alloc_counts.py,
written once.  A Ledger reads the library's two process-wide counters (options "live_allocs" / "allocs_made") through a probe
context that does nothing else, and notes them after every step relative to its start; every scenario runs on a context of its
own, destroys it and returns the ledger's rows [step, allocations made so far, allocations live]."""
import numpy as np

from gpyrn_amd import _hip, covfunc

SHAPES = {'one_tile': (45, 2, 2), 'two_tiles': (200, 2, 2), 'q1_masked_time': (45, 2, 1)}
B = 3                         # evaluations of the side-by-side steps


class Problem:
    """Synthetic data, SE kernels for every latent GP and a starting state: all the entry points take."""

    def __init__(self, N, p, q, seed=0):
        rng = np.random.default_rng(seed + 7 * N + p + q)
        self.N, self.p, self.q, self.G = N, p, q, q * (p + 1)
        self.time = np.sort(rng.uniform(0.0, 60.0, N))
        self.y = np.sin(self.time / 5.0)[None, :] * rng.uniform(0.5, 2.0, (p, 1)) + 0.1 * rng.standard_normal((p, N))
        self.yerr = np.full((p, N), 0.1)
        self.ops = [(covfunc.OP_PUSH, covfunc.KID['SE'], 0)]
        self.params = np.array([[1.0 + 0.1 * g, 6.0 + g] for g in range(self.G)])      # (amplitude, length scale) per latent GP
        self.jit = np.full(p, 0.2)
        d = (p + 1) * q * N
        self.mu0, self.var0 = 0.1 * rng.standard_normal(d), np.full(d, 0.5)
        self.tstar = np.linspace(-1.0, 61.0, (-(-N // 128)) * 128 + 3)                  # ns = ld + 3
        self.tshort = self.tstar[::19][:7]
        self.z = rng.standard_normal((self.G, 2, self.tshort.size))

    def mask(self, which=0):
        """Every output observed somewhere; with q = 1 one time with NO output observed (the node phase's entries)."""
        m = np.ones((self.p, self.N), dtype=bool)
        m[0, 3 + which:self.N:7] = False
        m[self.p - 1, 5 + which:self.N:11] = False
        m[0, ~m.any(axis=0)] = True                   # (q >= 2 needs an observed output at every time)
        if self.q == 1:
            m[:, 9 + which] = False
        return m

    def batch(self, n=B):
        """The arrays of gprn_elbocalc_batch* for n evaluations: (kernel_params, y_resid, jitters, mu, var)."""
        kp = np.array([np.ravel(self.params) * (1.0 + 0.01 * b) for b in range(n)])
        return kp, np.array([self.y] * n), np.array([self.jit] * n), np.array([self.mu0] * n), np.array([self.var0] * n)

    def folds(self, n=2, mask=None):
        """Fold b holds out every fifth entry of output b (of what `mask` observes): every time keeps a fitted output."""
        f = np.ones((n, self.p, self.N), dtype=bool) if mask is None else np.array([mask] * n)
        for b in range(n):
            f[b, b % self.p, b + 1::5] = False
        return f


class Ledger:
    def __init__(self):
        self.probe = _hip.Context(0)
        self.made0, self.live0 = self.read()
        self.rows = []

    def read(self):
        return self.probe.option('allocs_made'), self.probe.option('live_allocs')

    def note(self, step):
        made, live = self.read()
        self.rows.append([step, made - self.made0, live - self.live0])
        return self.rows[-1]

    def close(self):
        self.probe.close()
        return self.rows


def set_up(ctx, pr, mask=None, data=True):
    if data:
        ctx.set_data(pr.time, pr.y, pr.yerr, pr.q)
        for g in range(pr.G):
            ctx.set_kernel(g, pr.ops, pr.params[g], True)
    if mask is not None:
        ctx.set_mask(mask)
    ctx.set_y_resid(pr.y)
    ctx.set_jitters(pr.jit)
    ctx.factor_priors()
    ctx.set_muvar(pr.mu0, pr.var0)


def sweeps(ctx, n=3):
    elbo, _, info = ctx.sweep(n)
    assert np.all(np.isfinite(elbo)), (elbo, info)          # (the numbers are other tests' business; a NaN would cut the scenario short)


def life_cycle(shape):
    """Set-up, sweeps, ELBOcalc, the predictions, a kernel gradient, the four side-by-side calls, destroy."""
    pr = Problem(*SHAPES[shape])
    masked = shape == 'q1_masked_time'
    led = Ledger()
    ctx = _hip.Context(0)
    led.note('create')
    if masked:
        ctx.option('batch_mask', 1)
    set_up(ctx, pr, pr.mask() if masked else None)
    led.note('set_up')
    sweeps(ctx)
    led.note('sweep x3')
    ctx.elbocalc(20, setup=True, y_resid=pr.y, jitters=pr.jit, mu=pr.mu0, var=pr.var0)
    led.note('elbocalc')
    ctx.predict(pr.tstar)
    led.note('predict ns = ld + 3')
    ctx.predict_cov(pr.tshort)
    led.note('predict_cov')
    ctx.predict_draws(pr.tshort, pr.z)
    led.note('predict_draws')
    if not masked:                                    # (gprn_keep_sigma refuses a data mask)
        ctx.set_muvar(pr.mu0, pr.var0)
        ctx.keep_sigma(True)
        ctx.factor_priors()
        sweeps(ctx, 1)
        assert ctx.grad_kernel(0, ctx.get_muvar()[0][0, 0], 2) is not None
        ctx.keep_sigma(False)
        led.note('grad_kernel')
    kp, yr, jt, m0, v0 = pr.batch()
    for step, call in (('elbocalc_batch', lambda: ctx.elbocalc_batch(kp, yr, jt, m0, v0, 20)),
                       ('elbocalc_batch_grad', lambda: ctx.elbocalc_batch(kp, yr, jt, m0, v0, 20, want_grad=True)),
                       ('elbocalc_batch_predict', lambda: ctx.elbocalc_batch_predict(kp, yr, jt, m0, v0, 20, pr.tshort)),
                       ('elbocalc_batch_heldout', lambda: ctx.elbocalc_batch_heldout(kp[:2], yr[:2], jt[:2], m0[:2], v0[:2], 20,
                                                                                     pr.folds(2, pr.mask() if masked else None)))):
        out = call()
        assert out is not None, step                  # (None: the library has no side-by-side form for this problem)
        led.note(step)
    ctx.close()
    led.note('destroy')
    return led.close()


def reuse_data():
    """One context, three problems in turn: two tiles, one tile, two tiles again."""
    led = Ledger()
    ctx = _hip.Context(0)
    for i, shape in enumerate(('two_tiles', 'one_tile', 'two_tiles')):
        set_up(ctx, Problem(*SHAPES[shape]))
        led.note('set_up %s #%d' % (shape, i))
        sweeps(ctx)
        led.note('sweep x3 #%d' % i)
    ctx.close()
    led.note('destroy')
    return led.close()


def reuse_mask(shape):
    """A mask, none, another mask."""
    pr = Problem(*SHAPES[shape])
    led = Ledger()
    ctx = _hip.Context(0)
    set_up(ctx, pr)
    sweeps(ctx)
    led.note('unmasked')
    for step, mask in (('mask', pr.mask()), ('mask cleared', None), ('second mask', pr.mask(1))):
        ctx.set_mask(mask)
        set_up(ctx, pr, data=False)
        sweeps(ctx)
        led.note(step)
    ctx.close()
    led.note('destroy')
    return led.close()


def elbo_form_frees_batch(shape):
    """Changing option "elbo_form" with batch buffers present frees them."""
    pr = Problem(*SHAPES[shape])
    led = Ledger()
    ctx = _hip.Context(0)
    set_up(ctx, pr)
    led.note('set_up')
    out = ctx.elbocalc_batch(*pr.batch(), 20)
    assert out is not None
    led.note('elbocalc_batch')
    ctx.option('elbo_form', _hip.ELBO_BOUND)
    led.note('elbo_form changed')
    ctx.close()
    led.note('destroy')
    return led.close()


def sequential_under_mask(shape):
    """The sequential sweep order with option "order_mask" on a masked context."""
    pr = Problem(*SHAPES[shape])
    led = Ledger()
    ctx = _hip.Context(0)
    ctx.option('order_mask', 1)
    ctx.set_sweep_order(_hip.ORDER_SEQUENTIAL)
    set_up(ctx, pr, pr.mask())
    sweeps(ctx)
    led.note('sweep x3')
    ctx.close()
    led.note('destroy')
    return led.close()


def steady(shape):
    """A warm call, then the same call again: what the SECOND gprn_sweep, gprn_elbocalc and gprn_elbocalc_batch allocate."""
    pr = Problem(*SHAPES[shape])
    led = Ledger()
    ctx = _hip.Context(0)
    set_up(ctx, pr)
    kp, yr, jt, m0, v0 = pr.batch()
    calls = (('sweep', lambda: sweeps(ctx)),
             ('elbocalc', lambda: ctx.elbocalc(20, setup=True, y_resid=pr.y, jitters=pr.jit, mu=pr.mu0, var=pr.var0)),
             ('elbocalc_batch', lambda: ctx.elbocalc_batch(kp, yr, jt, m0, v0, 20)))
    for name, call in calls:
        call()
        led.note(name + ' warm')
        call()
        led.note(name + ' second')
    ctx.close()
    led.note('destroy')
    return led.close()


def second_call_allocs(rows):
    """{call: allocations its second run made} of steady()'s rows."""
    made = {step: m for step, m, _ in rows}
    return {k[:-len(' second')]: made[k] - made[k[:-len(' second')] + ' warm'] for k in made if k.endswith(' second')}


def all_scenarios():
    """{name: scenario}, each a function without arguments that returns its rows."""
    import functools
    out = {'life_cycle/' + shape: functools.partial(life_cycle, shape) for shape in SHAPES}
    out['reuse_data'] = reuse_data
    for shape in SHAPES:
        out['reuse_mask/' + shape] = functools.partial(reuse_mask, shape)
    for shape in ('one_tile', 'two_tiles'):
        out['elbo_form_frees_batch/' + shape] = functools.partial(elbo_form_frees_batch, shape)
        out['sequential_under_mask/' + shape] = functools.partial(sequential_under_mask, shape)
        out['steady/' + shape] = functools.partial(steady, shape)
    return out
