"""The celerite kernels on the host (gpyrn_amd.covfunc: SHO, Rotation, CeleriteTerm): ids, parameter plumbing, device
programs, and NumPy's own evaluation of the values and of the closed-form parameter derivatives against
tests/golden/celerite_highprec (tests/_gen_celerite_fixtures.py, mpmath at 40 digits) at the bounds the device is held to:

    |K - K_ref| <= (4 + 2 kappa) 2^-53 |K_ref| + the denormal floor       (tests/_fill_fixture.violations, c0 unraised)
    max |d - d_ref| <= 2e-11 max |d_ref| per parameter and case           (tests/_dk_cases.DK_TOL)

and the identities that tie the three to each other and to the kernels the library already had."""
import os
import re

import numpy as np
import pytest

from gpyrn_amd import covfunc as c
from gpyrn_amd import inference, meanfunc
from tests import _celerite_fixture as cx
from tests import _celerite_formulas as cf
from tests import _dk_cases as dc
from tests import _fill_fixture as ff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fixture():
    return cx.load()


# ------------------------------------------------------------------ ids, plumbing, programs
def test_ids_match_the_header():
    text = open(os.path.join(ROOT, 'include', 'gprn_hip.h')).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r'GPRN_K_([A-Z0-9]+)\s*=\s*(\d+)', text)}
    assert ids.pop('COUNT') == 27 == len(ids)
    assert ids == c.KID == cf.KID
    assert (c.KID['SHO'], c.KID['ROTATION'], c.KID['CELERITE']) == (24, 25, 26)
    assert {'SHO', 'Rotation', 'CeleriteTerm'} <= set(c.__all__)
    assert cx.DK_TOL == dc.DK_TOL


def test_parameter_plumbing():
    sho, rot, cel = c.SHO(1.3, 11.0, 3.0), c.Rotation(1.1, 9.0, 1.2, 0.3, 0.4), c.CeleriteTerm(1.2, 0.3, 0.1, 0.7)
    assert (sho._param_names, rot._param_names, cel._param_names) == (
        ('theta', 'P0', 'Q'), ('theta', 'P', 'Q0', 'dQ', 'f'), ('a', 'b', 'c', 'd'))
    # set_parameters consumes its own and hands the tail on
    tail = sho.set_parameters(np.arange(1.0, 14.0))
    tail = rot.set_parameters(tail)
    tail = cel.set_parameters(tail)
    assert sho.pars.tolist() == [1, 2, 3] and rot.pars.tolist() == [4, 5, 6, 7, 8] and cel.pars.tolist() == [9, 10, 11, 12]
    assert np.asarray(tail).tolist() == [13]
    assert repr(sho) == 'SHO(theta=1.0, P0=2.0, Q=3.0)'
    t = np.linspace(0.0, 30.0, 16)
    g = inference(1, t, np.zeros(16), np.ones(16))
    g.set_components([c.SHO(1.3, 11.0, 3.0)], [c.Rotation(1.1, 9.0, 1.2, 0.3, 0.4)], [meanfunc.Constant(0.0)], [0.1])
    names = list(g.parameters_dict)
    assert names == ['node1.theta', 'node1.P0', 'node1.Q', 'weight1.theta', 'weight1.P', 'weight1.Q0', 'weight1.dQ',
                     'weight1.f', 'mean1.c', 'jitter1'], names
    g.freeze_parameter(name='weight1*')
    g.freeze_parameter(name='node1.Q')
    assert g.frozen_mask.tolist() == [False, False, True] + [True] * 5 + [False, False]
    g.thaw_parameter(name='weight1.f')
    assert g.get_parameters().tolist() == [1.3, 11.0, 0.4, 0.0, 0.1]
    g.set_parameters([1.5, 12.0, 0.5, 0.2, 0.3])
    assert g.nodes[0].pars.tolist() == [1.5, 12.0, 3.0] and g.weights[0].pars.tolist() == [1.1, 9.0, 1.2, 0.3, 0.5]


def test_device_programs():
    P, A, M = c.OP_PUSH, c.OP_ADD, c.OP_MUL
    sho, rot, cel = c.SHO(1.3, 11.0, 3.0), c.Rotation(1.1, 9.0, 1.2, 0.3, 0.4), c.CeleriteTerm(1.2, 0.3, 0.1, 0.7)
    for k, kid in ((sho, 24), (rot, 25), (cel, 26)):
        ops, pars = k._device_program()
        assert ops == [(P, kid, 0)] and np.array_equal(pars, k.pars)
    ops, pars = (sho * c.SquaredExponential(1.0, 30.0) + c.WhiteNoise(0.4))._device_program()
    assert ops == [(P, 24, 0), (P, c.KID['SE'], 3), (M, 0, 0), (P, c.KID['WHITENOISE'], 5), (A, 0, 0)]
    assert pars.tolist() == [1.3, 11.0, 3.0, 1.0, 30.0, 0.4]
    ops, pars = (rot + cel)._device_program()
    assert ops == [(P, 25, 0), (P, 26, 5), (A, 0, 0)] and pars.tolist() == [1.1, 9.0, 1.2, 0.3, 0.4, 1.2, 0.3, 0.1, 0.7]
    t = np.linspace(0.0, 30.0, 16)
    g = inference(1, t, np.zeros(16), np.ones(16))
    for k in (sho, rot, cel, sho * c.SquaredExponential(1.0, 30.0) + c.WhiteNoise(0.4), rot + cel):
        spec = g._kernel_spec(k)
        assert spec[0] == 'device' and spec[3] is True          # (one-argument: takes the set-up's nugget)

    class Mine(c.SHO):                                           # a user subclass may override __call__: no device id
        pass
    assert Mine(1.0, 2.0, 3.0)._device_program() is None


# ------------------------------------------------------------------ values and derivatives against the fixture
def test_numpy_values_meet_the_bound(fixture):
    meta, d, _ = fixture
    fails, ratios = [], {}
    for case in meta['cases']:
        r = []
        v = ff.violations(ff.numpy_matrix(case, d['t_' + case['tset']]), case, d, ratios=r)
        ratios[case['kernel']] = max(ratios.get(case['kernel'], 0.0), r[0])
        if v:
            fails.append('%s: %d elements off, e.g. K[%d,%d] = %r, reference %r, allowed %.3g' % (case['name'], len(v), *v[0]))
    print('\n' + '\n'.join('celerite_numpy_value %-14s worst error / allowed %.3f' % kv for kv in sorted(ratios.items())))
    assert not fails, '\n'.join(fails)


def test_numpy_rectangular_values_meet_the_bound(fixture):
    """K* and k** of the rectangular sample, both forms: the coincidence rule as covfunc has no word for it, the nugget and
    WhiteNoise as delta(t, t') added here."""
    meta, _, rd = fixture
    fails = []
    for case in meta['cases']:
        rc = cx.rect_case(case)
        t, ts = rd['t_' + case['tset']], rd['ts_' + case['tset']]
        k = cx.kernel_of(case)
        white = 0.4 ** 2 if 'WhiteNoise' in case['expr'] else 0.0
        with np.errstate(all='ignore'):
            off = np.asarray((k.k1 if white else k)(ts[:, None] - t[None, :]), dtype=float)
            zero = float(np.asarray((k.k1 if white else k)(np.zeros(1)))[0])
        for form in (ff.REF, ff.POST):
            nug = ff.rect_nugget(meta, rc, form)
            Ks = off + (nug + white) * (ts[:, None] == t[None, :]) if form == ff.POST else off
            kss = np.full((ts.size, 1), zero + white + nug)
            vk, vs = ff.rect_views(rc, rd, form, meta['ns'])
            for what, K, (cc, dd) in (('K*', Ks, vk), ('k**', kss, vs)):
                v = ff.violations(K, cc, dd)
                if v:
                    fails.append('%s form %d %s: %d off, e.g. [%d,%d] = %r, reference %r, allowed %.3g'
                                 % (case['name'], form, what, len(v), *v[0]))
    assert not fails, '\n'.join(fails)


def test_numpy_derivatives_meet_the_bound(fixture):
    """covFunction._dk_dpars of the three classes (closed forms) and through Sum / Multiplication.  WhiteNoise has no closed
    form on the host (the base class differentiates it numerically, to 1e-10): its parameter, the last of the two composites
    that carry it, is NOT compared here -- tests/test_celerite_dk_host.py and tests/test_celerite_gpu.py hold it."""
    meta, d, _ = fixture
    fails, seen = [], 0
    for case in meta['cases']:
        if case['dk_off'] is None:
            continue
        dK = cx.numpy_dk(case, d['t_' + case['tset']])
        w = cx.dk_worst(dK, case, d, skip=(dK.shape[0] - 1,) if 'WhiteNoise' in case['expr'] else ())
        seen += 1
        print('celerite_numpy_dk %-28s %.2e' % (case['name'], w))
        if not w <= cx.DK_TOL:
            fails.append('%s: off by %.2e of max |ref|' % (case['name'], w))
    assert seen == len(meta['cases']) - 12 - 3              # (NaN parameters; the three cases dropped from this bound)
    assert not fails, '\n'.join(fails)


def test_nan_parameters_give_nan(fixture):
    meta, d, _ = fixture
    nans = [case for case in meta['cases'] if '_nan_' in case['name']]
    assert len(nans) == 12
    for case in nans:
        t = d['t_' + case['tset']]
        assert np.isnan(ff.numpy_matrix(case, t)).all(), case['name']
        l = int(np.flatnonzero(np.isnan(case['pars']))[0])
        dK = cx.numpy_dk(case, t)
        # (the amplitude b of CeleriteTerm does not enter dk/da = e^-c tau cos: NaN wherever the value's own formula reads it)
        assert np.isnan(dK[l]).all() or case['kernel'] == 'CeleriteTerm', case['name']
        assert np.isnan(dK).any(axis=0).all(), case['name']


def test_the_fixture_holds_what_it_says(fixture):
    """Layout and coverage: every case of the issue's list, at most 500 elements each, the file sizes, the far tail's range."""
    meta, d, rd = fixture
    names = [case['name'] for case in meta['cases']]
    from tests import _gen_celerite_fixtures as gen
    assert names == [case['name'] for case in gen.case_list()]
    assert all(case['n'] <= 500 and case['rect']['n'] <= 500 for case in meta['cases'])
    size = sum(os.path.getsize(os.path.join(ff.GOLDEN, 'celerite_highprec.' + e)) for e in ('npz', 'json'))
    assert size < 2 ** 20
    for reg in ('R1', 'R2', 'R3'):
        assert 120 <= d['t_' + reg].size <= 200 and rd['t_' + reg].size == 129 and rd['ts_' + reg].size == 130
    by = {case['name']: case for case in meta['cases']}
    for name, lo, hi in (('SHO_tail_0', 1e3, 1e5), ('SHO_tail_1', 1e3, 1e5)):
        theta, P0, Q = by[name]['pars']
        a = np.pi * 60.0 / (P0 * Q)
        assert lo <= a <= hi * 1.01
        i, j, ref, _, _ = ff.case_arrays(by[name], d)
        assert ref.min() > 1e-3 * theta ** 2, name
    for name in ('SHO_underflow_0', 'SHO_underflow_1', 'CeleriteTerm_underflow_0'):
        i, j, ref, _, _ = ff.case_arrays(by[name], d)
        assert (ref[i != j] == 0).all() and (ref[i == j] > 0).all(), name


# ------------------------------------------------------------------ the end-to-end model of tests/test_celerite_gpu.py
@pytest.mark.parametrize('N', [45, 150])
def test_the_two_forms_of_a_sweep_agree_on_the_end_to_end_model(N):
    """oracle.cpu_ref.sweep_B against sweep_ref over three sweeps of tests/_celerite_model.py: 1e-9 on the ELBO and norm-wise on
    the state, so that the B-form's own gap does not eat the 1e-8 the device is held to; and ELBOcalc's stop rule ends away
    from its threshold, so that the trip count is comparable."""
    from oracle import cpu_ref
    from tests import _celerite_model as cm
    pr = cm.problem(N)
    a = pr['args']
    mu, var, mu2, var2 = pr['mu0'], pr['var0'], pr['mu0'], pr['var0']
    for _ in range(3):
        e1, mu, var, _ = cpu_ref.sweep_ref(*a, mu, var)
        e2, mu2, var2, _ = cpu_ref.sweep_B(*a, mu2, var2)
        assert abs(e1 - e2) <= 1e-9 * abs(e1)
        assert np.abs(mu - mu2).max() <= 1e-9 * np.abs(mu).max() and np.abs(var - var2).max() <= 1e-9 * np.abs(var).max()
    if N == 45:                                     # (the loop at N = 150 is the GPU test's own reference: seconds of NumPy)
        hist = cpu_ref.elbo_calc(*a, pr['mu0'], pr['var0'])[4]
        for k in (len(hist) - 1, len(hist) - 2):
            last = hist[k - 2:k + 1]
            assert abs(abs(np.std(last) / np.mean(last)) - 1e-3) > 1e-6 * 1e-3


# ------------------------------------------------------------------ identities
def _kappa(k, r):
    """sum_u |u dk/du| / |k| over r and the kernel's parameters by central differences of relative step 1e-6 in fp64 --
    their own error, 1e-10 kappa, moves the bound by a part in 1e9."""
    h = 1e-6
    leaves = []

    def walk(x):
        if isinstance(x, c._operator):
            walk(x.k1)
            walk(x.k2)
        else:
            leaves.append(x)
    walk(k)
    with np.errstate(all='ignore'):
        tot = np.abs(k(r * (1 + h)) - k(r * (1 - h))) / (2 * h)
        for leaf in leaves:
            keep = leaf.pars.copy()
            for l, v in enumerate(keep):
                leaf.pars = keep.copy(); leaf.pars[l] = v * (1 + h)
                up = k(r)
                leaf.pars = keep.copy(); leaf.pars[l] = v * (1 - h)
                tot = tot + np.abs(up - k(r)) / (2 * h)
            leaf.pars = keep
        val = k(r)
        return val, np.where(val != 0, tot / np.abs(val), 0.0)


def _allowed(k, r):
    val, kappa = _kappa(k, r)
    return val, (ff.C0 + ff.C1 * kappa) * ff.EPS * np.abs(val) + ff.A_DENORM


def _same(ka, kb, r):
    (a, ba), (b, bb) = _allowed(ka, r), _allowed(kb, r)
    bad = ~(np.abs(a - b) <= ba + bb)
    assert not bad.any(), '%s against %s: %d elements, worst %.3g of the two bounds' % (
        ka, kb, int(bad.sum()), float((np.abs(a - b) / (ba + bb))[bad].max()))


@pytest.fixture(scope='module')
def r_grid(fixture):
    t = fixture[1]['t_R1']
    return t[:, None] - t[None, :]


def test_sho_at_the_critical_point_is_matern32(r_grid):
    _same(c.SHO(1.3, 11.0, 0.5), c.Matern32(1.3, np.sqrt(3.0) * 11.0 / (2 * np.pi)), r_grid)


def test_rotation_is_two_oscillators(r_grid):
    """celerite2's mapping: Q1 = 1/2 + Q0 + dQ and Q2 = 1/2 + Q0, undamped periods P g / (2 Q) of the period P and its
    half, amplitudes theta^2 / (1 + f) and f theta^2 / (1 + f)"""
    for theta, P, Q0, dQ, f in ((1.1, 9.0, 1.2, 0.3, 0.4), (0.8, 25.0, 0.05, 2.0, 3.0)):
        Q1, Q2 = 0.5 + Q0 + dQ, 0.5 + Q0
        g1, g2 = 2 * np.sqrt((Q0 + dQ) * (Q0 + dQ + 1)), 2 * np.sqrt(Q0 * (Q0 + 1))
        two = (c.SHO(theta / np.sqrt(1 + f), P * g1 / (2 * Q1), Q1)
               + c.SHO(theta * np.sqrt(f / (1 + f)), 0.5 * P * g2 / (2 * Q2), Q2))
        _same(c.Rotation(theta, P, Q0, dQ, f), two, r_grid)


def test_real_celerite_term_is_exponential(r_grid):
    _same(c.CeleriteTerm(1.2, 0.0, 0.1, 0.0), c.Exponential(np.sqrt(1.2), 1 / 0.1), r_grid)


def test_underdamped_sho_is_a_celerite_term(r_grid):
    for theta, P0, Q in ((1.3, 11.0, 3.0), (1.3, 11.0, float(1 / np.sqrt(2))), (0.7, 4.0, 40.0)):
        w0, g = 2 * np.pi / P0, np.sqrt((2 * Q - 1) * (2 * Q + 1))
        _same(c.SHO(theta, P0, Q), c.CeleriteTerm(theta ** 2, theta ** 2 / g, w0 / (2 * Q), g * w0 / (2 * Q)), r_grid)
