"""Prediction's rectangular fills K* and k** (csrc/fill.hip: k_fill_rect<KID>, its posterior form k_fill_rect<KID, true>,
k_fill_rect_batch, k_fill_rect_batch_post) launch by launch through gprn_test_fill_rect, against
tests/golden/rect_highprec (oracle/gen_rect_highprec.py, mpmath at 40 digits): every built-in kernel, the derivative
kernels and the composites over the regimes of the square fixture, rows from t* and columns from t, held to the bound of
tests/_fill_fixture.py -- the one NumPy's own evaluation meets (tests/test_rect_highprec.py).

The buffers come back WHOLE and hold NaN bytes before the launch: the zeros of the padding are the kernel's."""
import numpy as np
import pytest

from gpyrn_amd import _hip
from oracle import kernel_formulas as kf
from tests import _fill_fixture as ff

pytestmark = pytest.mark.gpu
N, NS, LD, NS_PAD = 200, 137, 256, 256
REGIMES = ('R1', 'R2', 'R3', 'R4', 'R5', 'R6')
FORMS = (ff.REF, ff.POST)
RATIOS = {}                          # (kernel, form) -> worst error / allowed seen


def _s_pow2(n):
    """s of the posterior form as exact powers of two, zero on a tenth of the rows (none of them a coincident column of the
    fixture): K* diag(s) is then exact in the reference, and the bound applies to it as it stands"""
    k = np.arange(n)
    return np.where(k % 10 == 6, 0.0, np.array([0.25, 0.5, 1.0, 2.0])[k % 4])


def _ctx(t):
    ctx = _hip.Context(0)
    ctx.set_data(t, np.zeros((1, t.size)), np.ones((1, t.size)), 1)
    return ctx


@pytest.fixture(scope='module')
def rect():
    """(meta, arrays, one context per time set)"""
    meta, d = ff.load_rect()
    ctxs = {reg: _ctx(d['t_' + reg]) for reg in ('R1', 'R2', 'R3', 'R5', 'R6')}
    yield meta, d, ctxs
    assert all(ctx.option('fallbacks') == 0 for ctx in ctxs.values())
    for ctx in ctxs.values():
        ctx.close()


def _fill(meta, d, ctxs, c, form, batched=0, s=None, ops=None, pars=None):
    ts = d['ts_' + c['tset']]
    if form == ff.POST and s is None:
        s = _s_pow2(N)
    return ctxs[c['tset']].test_fill_rect(c['ops'] if ops is None else ops, c['pars'] if pars is None else pars,
                                          ff.rect_nugget(meta, c, form), ts, form=form, batched=batched,
                                          s=s if form == ff.POST else None)


def _show(fails):
    return '\n'.join(fails[:25]) + ('\n... %d in all' % len(fails) if len(fails) > 25 else '')


def _record():
    """the `rect_fill_accuracy` lines of `pytest -s` (profiles/rect_fill_accuracy.txt): per kernel the worst
    |K - K_ref| / allowed seen so far over the sampled elements of K* and all of k**, reference form | posterior form"""
    print()
    for k in sorted({k for k, _ in RATIOS}):
        print('rect_fill_accuracy %-28s %.3f  %.3f' % (k, RATIOS.get((k, ff.REF), 0.0), RATIOS.get((k, ff.POST), 0.0)))


# ------------------------------------------------------------------ every case, both forms, the single launch
@pytest.mark.parametrize('regime', REGIMES)
def test_single_launch_meets_the_bound_in_both_forms(rect, regime):
    """|K - K_ref| <= (4 + 2 kappa) 2^-53 |K_ref| + the denormal floor at every sampled element of K* and in all of k**,
    NaN where the reference is NaN; R6: where the exact value is a double, that double.  The posterior form runs with s a
    pattern of powers of two and zeros: K*_ref s_n is exact, the same bound holds, and a column of s = 0 is exactly 0.0
    whatever the size of the kernel's values (where they are finite: 0 NaN is NaN)."""
    meta, d, ctxs = rect
    cases = [c for c in meta['cases'] if c['regime'] == regime]
    assert cases
    s = _s_pow2(N)
    fails = []
    for c in cases:
        for form in FORMS:
            Ks, kss = _fill(meta, d, ctxs, c, form)
            vk, vs = ff.rect_views(c, d, form, NS)
            if form == ff.POST:
                vk = ff.scale_columns(vk, s)
            ratios = []
            for what, K, (cc, dd) in (('K*', Ks, vk), ('k**', kss[:, None], vs)):
                v = ff.violations(K, cc, dd, ratios=ratios)
                if v:
                    fails.append('%s form %d %s: %d elements off, e.g. [%d,%d] = %r, reference %r, allowed %.3g'
                                 % (c['name'], form, what, len(v), *v[0]))
                if regime == 'R6':
                    i, j, hi, lo, _ = ff.case_arrays(cc, dd)
                    k = K[i, j]
                    bad = (lo == 0) & ~((k == hi) | (np.isnan(k) & np.isnan(hi)))
                    if bad.any():
                        fails.append('%s form %d %s: [%d,%d] = %r, the exact value is the double %r'
                                     % (c['name'], form, what, i[bad][0], j[bad][0], k[bad][0], hi[bad][0]))
            key = (c['kernel'], form)
            RATIOS[key] = max(RATIOS.get(key, 0.0), *ratios)
            if form == ff.POST and np.all(np.isfinite(vk[1]['hi'])) and np.all(np.isfinite(vs[1]['hi'])):
                z = Ks[:NS, :N][:, s == 0]
                if not np.all(z == 0.0):
                    fails.append('%s: a column of s = 0 is not zero' % c['name'])
    _record()
    assert not fails, _show(fails)


def _two_prod(a, b):
    """a b = p + e exactly (Veltkamp's split, Dekker's product)"""
    def split(x):
        c = 134217729.0 * x
        h = c - (c - x)
        return h, x - h
    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def test_generic_s_costs_one_more_rounding(rect):
    """The posterior form with s of full mantissas: K*[i][n] s_n rounds once more -- C0 + 1 in the bound, against the
    exact product of the reference and s_n."""
    meta, d, ctxs = rect
    s = np.random.default_rng(5).uniform(0.5, 2.0, N)
    fails = []
    for c in meta['cases']:
        Ks, _ = _fill(meta, d, ctxs, c, ff.POST, s=s)
        cc, dd = ff.rect_views(c, d, ff.POST, NS)[0]
        with np.errstate(all='ignore'):
            p, e = _two_prod(dd['hi'], s[dd['j'].astype(int)])
            dd = dict(dd, hi=p, lo=np.where(np.isfinite(p), e + dd['lo'].astype(float) * s[dd['j'].astype(int)], 0.0))
        v = ff.violations(Ks, cc, dd, c0=ff.C0 + 1)
        if v:
            fails.append('%s: %d elements off, e.g. [%d,%d] = %r, reference %r, allowed %.3g' % (c['name'], len(v), *v[0]))
    assert not fails, _show(fails)


# ------------------------------------------------------------------ padding
def test_padding_is_zero_and_k_star_star_has_ns_entries(rect):
    """Rows [ns, ns_pad) and columns [N, ld) of the returned buffer are exactly 0.0 in both forms (cov_conditional contracts
    over all ld columns), k** is written at its ns entries and nowhere else."""
    meta, d, ctxs = rect
    fails = []
    for c in meta['cases']:
        for form in FORMS:
            Ks, kss = _fill(meta, d, ctxs, c, form)
            assert Ks.shape == (NS_PAD, LD) and kss.shape == (NS_PAD,)
            pad = np.concatenate([Ks[NS:].ravel(), Ks[:NS, N:].ravel()])
            want = np.isfinite(ff.rect_views(c, d, form, NS)[1][1]['hi'])
            if not np.all(pad == 0.0):
                fails.append('%s form %d: %d entries of the padding are not 0.0' % (c['name'], form, int((pad != 0.0).sum())))
            if not (np.isnan(kss[NS:]).all() and np.array_equal(np.isfinite(kss[:NS]), want)):
                fails.append('%s form %d: k** has %d finite entries' % (c['name'], form, int(np.isfinite(kss).sum())))
            if c['regime'] in ('R1', 'R2') and not np.isfinite(Ks[:NS, :N]).all():
                fails.append('%s form %d: K* is not finite everywhere' % (c['name'], form))
    assert not fails, _show(fails)


# ------------------------------------------------------------------ shapes at the edges
EDGE_KERNELS = ('SquaredExponential_R1_0',       # host reciprocals
                'Matern52_R1_0',                 # a plain specialisation
                'deep7_R1_0')                    # k_fill_rect<-1>; ROWS = 1 with grid.y = ns_pad in the posterior form
EDGE_NS = (1, 7, 8, 9, 128, 129, 257)
LDBL = np.longdouble


def _longdouble_k(ops, pars, r):
    """(k, sum_u |u dk/du|) of a program in r alone (no WhiteNoise in it) at the long-double array r, u over r and the
    parameters.  k in NumPy long double; the sum by central differences of relative step 1e-6 in doubles, whose own
    error -- some 1e-10 |k| per variable -- moves the bound by less than a part in 1e9."""
    k = kf.program(kf.np_arith(np, LDBL), ops, [LDBL(v) for v in pars], np.asarray(r, dtype=LDBL), LDBL(0), False)
    A = kf.np_arith(np, np.float64)
    xs = [np.asarray(r, dtype=np.float64)] + [np.float64(v) for v in pars]
    f = lambda x: kf.program(A, ops, x[1:], x[0], 0.0, False)           # noqa: E731
    h = 1e-6
    tot = np.zeros(k.shape)
    for u in range(len(xs)):
        up, dn = list(xs), list(xs)
        up[u], dn[u] = xs[u] * (1 + h), xs[u] * (1 - h)
        tot += np.abs(f(up) - f(dn)) / (2 * h)
    return k, tot


def _view(k, tot, delta, nug):
    """(case, d) as `violations` takes them for the whole matrix k + nug delta (the nugget: a constant of the sum)"""
    k = k + LDBL(nug) * delta
    hi = k.astype(float)
    i, j = np.indices(hi.shape)
    with np.errstate(all='ignore'):
        kappa = np.where(k != 0, tot / np.abs(k), 0).astype(float)
    d = {'i': i.ravel(), 'j': j.ravel(), 'hi': hi.ravel(), 'lo': (k - hi).astype(float).ravel(), 'kappa': kappa.ravel()}
    return {'off': 0, 'n': hi.size}, d


@pytest.mark.parametrize('n', [1, 77, 128, 200, 256, 300])
def test_shapes_at_the_edges(rect, n):
    """ld = 128, 256 (the posterior form's k** column in a workgroup of its own) and 384 (a partial last column block) against
    ns = 1 ... 257 (one row, the 8-row groups' edges, the 128-row padding's edges, three row tiles): bound, zeros of the
    padding, k**, for three kernels -- against a long-double evaluation of kernel_formulas at test time (once per kernel,
    over the longest t*: the shorter ones are its heads, and every one of them ends on the last data time)."""
    meta, d, _ = rect
    cases = {c['name']: c for c in meta['cases']}
    rng = np.random.default_rng(100 + n)
    t = np.sort(rng.uniform(0.0, 60.0, n))
    ld = -(-n // 128) * 128
    s = _s_pow2(n)
    s[n - 1], s[n // 3] = 2.0, 0.5
    ts = rng.uniform(-6.0, 66.0, max(EDGE_NS))
    ts[3], ts[5] = t[n // 3], ts[2]
    ts[[ns - 1 for ns in EDGE_NS]] = t[n - 1]                # the last row meets the last column
    delta = ts[:, None] == t[None, :]
    assert delta.sum() == len(EDGE_NS) + 1
    r = np.asarray(ts, dtype=LDBL)[:, None] - np.asarray(t, dtype=LDBL)[None, :]
    ctx = _ctx(t)
    fails = []
    try:
        for name in EDGE_KERNELS:
            c = cases[name]
            ops = [tuple(o) for o in c['ops']]
            assert c['nugget'] and not any(o[0] == 0 and o[1] in (kf.KID['WHITENOISE'],) + kf.TWO_ARGUMENT for o in ops)
            k, tot = _longdouble_k(ops, c['pars'], r)
            k0, tot0 = _longdouble_k(ops, c['pars'], np.zeros((1, 1)))
            for ns in EDGE_NS:
                ns_pad = -(-ns // 128) * 128
                for form in FORMS:
                    nug = ff.rect_nugget(meta, c, form)
                    Ks, kss = ctx.test_fill_rect(c['ops'], c['pars'], nug, ts[:ns], form=form, s=s if form == ff.POST else None)
                    assert Ks.shape == (ns_pad, ld) and kss.shape == (ns_pad,)
                    where = '%s form %d N %d ns %d' % (name, form, n, ns)
                    view = _view(k[:ns], tot[:ns], delta[:ns] if form == ff.POST else np.zeros_like(delta[:ns]), nug)
                    if form == ff.POST:
                        view = ff.scale_columns(view, s)
                    v = ff.violations(Ks, *view)
                    if v:
                        fails.append('%s K*: %d elements off, e.g. [%d,%d] = %r, reference %r, allowed %.3g' % (where, len(v), *v[0]))
                    # (a kernel in r alone: k** is one number)
                    v = ff.violations(kss[:, None], *_view(k0, tot0, np.ones((1, 1), dtype=bool), nug))
                    if v or not np.all(kss[:ns] == kss[0]) or not np.isnan(kss[ns:]).all():
                        fails.append('%s k**: %r ...' % (where, kss[:3]))
                    pad = np.concatenate([Ks[ns:].ravel(), Ks[:ns, n:].ravel()])
                    if not np.all(pad == 0.0):
                        fails.append('%s: %d entries of the padding are not 0.0' % (where, int((pad != 0.0).sum())))
                    if form == ff.POST and not np.all(Ks[:ns, :n][:, s == 0] == 0.0):
                        fails.append('%s: a column of s = 0 is not zero' % where)
        assert ctx.option('fallbacks') == 0
    finally:
        ctx.close()
    assert not fails, _show(fails)


# ------------------------------------------------------------------ specialised against generic
# kernels whose own instantiation may differ from the postfix program in the last bits (a contraction the compiler is free
# to choose per call site) and are held to the bound on both sides instead: none -- fill_eval.h rounds as written
CONTRACTION_DIFFERS = ()


def test_specialised_instantiation_equals_the_generic_program(rect):
    """k_fill_rect<KID> and k_fill_rect<KID, true> (one instantiation per kernel id; SE / Periodic / QP with host
    reciprocals) against the generic program of k * Constant(1.0), k_fill_rect<-1> and the one-row k_fill_rect<-1, true>: the
    same bits in the whole buffer, k** included."""
    meta, d, ctxs = rect
    fails = []
    kids = set()
    for c in meta['cases']:
        if len(c['ops']) != 1 or c['kernel'] in CONTRACTION_DIFFERS:
            continue
        kids.add(c['ops'][0][1])
        ops, pars = c['ops'] + [[0, 0, len(c['pars'])], [2, 0, 0]], list(c['pars']) + [1.0]
        for form in FORMS:
            own, gen = _fill(meta, d, ctxs, c, form), _fill(meta, d, ctxs, c, form, ops=ops, pars=pars)
            for what, a, b in zip(('K*', 'k**'), own, gen):
                if not np.array_equal(a, b, equal_nan=True):
                    fails.append('%s form %d %s: %d entries differ' % (c['name'], form, what,
                                                                       int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())))
    assert kids == set(range(24)), sorted(kids)               # every kernel id has run its own instantiation
    assert not fails, _show(fails)


# ------------------------------------------------------------------ batched against single
@pytest.mark.parametrize('regime', ['R1', 'R2'])
def test_batched_launch_has_the_bits_of_the_single_launch(rect, regime):
    """k_fill_rect_batch and k_fill_rect_batch_post over two programs -- the case's and one with every parameter scaled by
    1.25 (and another s) -- return the case's matrix and k** with the bits of the single launch, whichever of the two slots the
    case's program takes: nothing of the neighbour leaks."""
    meta, d, ctxs = rect
    fails = []
    for c in meta['cases']:
        if c['regime'] != regime:
            continue
        for form in FORMS:
            single = _fill(meta, d, ctxs, c, form)
            assert np.isfinite(single[0]).all() and np.isfinite(single[1][:NS]).all()
            for slot in (1, 2):
                got = _fill(meta, d, ctxs, c, form, batched=slot)
                for what, a, b in zip(('K*', 'k**'), got, single):
                    if not np.array_equal(a, b, equal_nan=True):
                        fails.append('%s form %d slot %d %s: %d entries differ' % (c['name'], form, slot - 1, what, int((a != b).sum())))
    assert not fails, _show(fails)


# ------------------------------------------------------------------ cross-check with the square fill
def test_rectangular_fill_at_the_data_times_against_the_square_fixture():
    """t* = t, the times of the SQUARE fixture (tests/golden/fill_highprec): off the diagonal the reference form's K* meets the
    bound eval_kernel(..., nugget = 0) is held to; under s = 1 the posterior form's row at a data time is the row of
    eval_kernel(..., GPRN_SETUP_NUGGET) within the bound, the diagonal with its nugget and WhiteNoise.  Bound-wise, not
    bit-wise: the symmetric fill has its own reciprocals.  (Pairs of EQUAL stamps off the diagonal, which the square
    fixture's R2 and R6 carry, are left out: there the posterior form has its delta terms and the square fill has not --
    data times are taken to be distinct.)"""
    cases, d = ff.load()
    rmeta, _ = ff.load_rect()
    nugget = {c['name']: c['nugget'] for c in rmeta['cases']}
    ctxs = {}
    fails = []
    try:
        for c in cases:
            t = d['t_' + c['tset']]
            ctx = ctxs.get(c['tset'])
            if ctx is None:
                ctx = ctxs[c['tset']] = _ctx(t)
            i, j, hi, lo, kappa = ff.case_arrays(c, d)
            nug = rmeta['setup_nugget'] if nugget[c['name']] else 0.0
            for form in FORMS:
                Ks, _ = ctx.test_fill_rect(c['ops'], c['pars'], nug if form == ff.POST else 0.0, t, form=form,
                                           s=np.ones(t.size) if form == ff.POST else None)
                keep = (i != j) & (t[i] != t[j]) if form == ff.REF else (i == j) | (t[i] != t[j])
                # (the nugget on the diagonal: hi + nug as a double-double, Knuth's two-sum)
                add = np.where(i == j, nug, 0.0) if form == ff.POST else np.zeros(i.size)
                with np.errstate(invalid='ignore'):
                    sm = hi + add
                    bb = sm - hi
                    err = (hi - (sm - bb)) + (add - bb)
                    view = {'i': i[keep], 'j': j[keep], 'hi': sm[keep], 'lo': np.where(np.isfinite(sm), err + lo, 0.0)[keep],
                            'kappa': kappa[keep]}
                v = ff.violations(Ks, {'off': 0, 'n': int(keep.sum())}, view)
                if v:
                    fails.append('%s form %d: %d elements off, e.g. [%d,%d] = %r, reference %r, allowed %.3g'
                                 % (c['name'], form, len(v), *v[0]))
    finally:
        for ctx in ctxs.values():
            ctx.close()
    assert not fails, _show(fails)
