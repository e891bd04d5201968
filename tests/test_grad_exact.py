"""The exact parameter derivatives' surface without a GPU: the header's declaration and option, the ABI table, and the
``exact_derivatives`` switch of ``inference`` reaching the context with every set-up (behind a stand-in context)."""
import os
import re

import numpy as np

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'gprn_hip.h')).read()


def test_the_header_declares_the_entry_point_and_the_option():
    text = _header()
    assert re.search(r'int\s+gprn_eval_kernel_grad\s*\(\s*gprn_ctx\s*\*\s*ctx,\s*const int32_t\s*\*\s*ops,\s*int n_ops,'
                     r'\s*const double\s*\*\s*params,\s*int n_params,\s*double\s*\*\s*dK_out\s*\)\s*;', text)
    assert 'not in the reference; derivative hooks covfunc.py:172-185' in text
    # with gprn_grad_kernel's rules, with gprn_grad_elbo's, and in gprn_set_option's list
    assert len(re.findall(r'"grad_exact"', text)) >= 3
    options = text[text.index('int gprn_set_option') - 4000:text.index('int gprn_set_option')]
    assert '"grad_exact"' in options


def test_the_abi_table_carries_the_entry_point():
    res, args = _hip.SIGNATURES['gprn_eval_kernel_grad']
    assert len(args) == 6 and hasattr(_hip.Context, 'eval_kernel_grad')


class _RecordingContext:
    """Stands in for _hip.Context through a set-up: remembers every option it is given."""
    rank = 0

    def __init__(self):
        self.options = []

    def option(self, name, value=-1):
        self.options.append((name, value))
        return 0

    def owner_of(self, gp):
        return 0

    def set_kernel(self, gp, ops, params, add_nugget):
        pass

    def upload_K(self, gp, K):
        pass

    def factor_priors(self):
        return 0

    def set_y_resid(self, y):
        pass

    def set_jitters(self, j):
        pass


def _object(**kw):
    rng = np.random.default_rng(3)
    N, p, q = 20, 2, 1
    t = np.sort(rng.uniform(0, 50, N))
    args = []
    for _ in range(p):
        args += [np.sin(t / 6) + 0.1 * rng.standard_normal(N), np.full(N, 0.2)]
    g = gpyrn.inference(q, t, *args, **kw)
    g.set_components([covfunc.Matern52(1.0, 10.0)], [covfunc.SquaredExponential(0.8, 20.0) + covfunc.WhiteNoise(0.1)] * p,
                     [meanfunc.Constant(0.0)] * p, [0.3] * p)
    return g


def _set_up(g):
    g._ctx = fake = _RecordingContext()
    g._prior_key = None
    g._setup_device(*g._get_components())
    return [v for n, v in fake.options if n == 'grad_exact']


def test_the_default_is_off():
    g = _object()
    assert g.exact_derivatives is False
    assert _set_up(g) == [0]


def test_the_switch_reaches_the_context_with_every_set_up():
    g = _object(exact_derivatives=True)
    assert g.exact_derivatives is True
    assert _set_up(g) == [1]
    g._setup_device(*g._get_components())              # unchanged kernels: no new factors, the option all the same
    assert [v for n, v in g._ctx.options if n == 'grad_exact'] == [1, 1]
    g.exact_derivatives = False                        # an attribute: the next set-up takes it back
    g._setup_device(*g._get_components())
    assert [v for n, v in g._ctx.options if n == 'grad_exact'] == [1, 1, 0]


def test_from_series_takes_the_keyword():
    t = np.linspace(0, 10, 12)
    series = [(t, np.sin(t), np.full(t.size, 0.1)), (t[::2] + 0.01, np.cos(t[::2]), np.full(t[::2].size, 0.1))]
    assert gpyrn.inference.from_series(1, series, exact_derivatives=True).exact_derivatives is True
    assert gpyrn.inference.from_series(1, series).exact_derivatives is False


def test_the_numpy_helper_of_the_gpu_tests_is_a_derivative():
    """tests/_dk_numpy.py (the plain fp64 evaluation that sets a kernel's bound in tests/test_grad_exact_gpu.py) against the
    long-double reference, element-wise: every kernel of r and the composites, three regimes."""
    from tests import _dk_cases as dc, _dk_numpy
    from oracle import kernel_formulas as kf
    t = dc.times(40)
    for L, P in dc.REGIMES:
        for name, k in dc.kernels(L, P):
            ops, pars = dc.program_of(k)
            if kf.uses_t(ops):
                continue
            assert dc.worst(_dk_numpy.dk_dpars(ops, pars, t), dc.reference(ops, pars, t)) <= 1e-9, (name, L, P)


def test_the_documents_name_the_option():
    for name in ('DESIGN.md', 'INTEGRATION.md', 'README.md'):
        assert 'grad_exact' in open(os.path.join(ROOT, name)).read(), name
