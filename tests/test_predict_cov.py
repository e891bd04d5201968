"""Full predictive covariances and joint posterior draws (inference.predict_cov / sample_posterior, gprn_predict_cov /
gprn_predict_draws): what holds without a GPU -- the algebra of the per-output covariance, the C ABI's declarations and
that the new methods have no host fallback."""
import os
import re

import numpy as np
import pytest

from gpyrn_amd import _hip
from tests import _predict_cov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('gprn_predict_cov', 'gprn_predict_draws', 'gprn_predict_upload_kss')


@pytest.mark.parametrize('q', [1, 2, 3])
@pytest.mark.parametrize('p', [1, 2, 3])
def test_output_covariance_diagonal_is_the_prediction_variance(p, q):
    """The diagonal of the per-output covariance is _Prediction's variance (meanfield.py:1364-1373), jitter^2 once per
    node included, on random latent means and covariances."""
    rng = np.random.default_rng(100 * p + q)
    ns = 23
    means, covs = [], []
    for _ in range(q * (p + 1)):
        A = rng.standard_normal((ns, ns))
        means.append(rng.standard_normal(ns))
        covs.append(A @ A.T / ns)
    jit = rng.uniform(0.1, 2.0, p)
    cov = ref.output_cov(means, covs, jit, p, q, joint=False)
    joint = ref.output_cov(means, covs, jit, p, q, joint=True)
    diag = np.array([np.diag(c) for c in cov]).T
    var = ref.prediction_variance(np.array(means[:q]), np.array([np.diag(c) for c in covs[:q]]),
                                  np.array(means[q:]), np.array([np.diag(c) for c in covs[q:]]), jit, p, q)
    np.testing.assert_allclose(diag, var, rtol=1e-14, atol=0)
    np.testing.assert_allclose(np.diag(joint).reshape(p, ns).T, var, rtol=1e-14, atol=0)
    for i in range(p):                   # the diagonal blocks of the joint matrix are the per-output matrices
        np.testing.assert_array_equal(joint[i * ns:(i + 1) * ns, i * ns:(i + 1) * ns], cov[i])


def test_new_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, 'include', 'gprn_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _hip.SIGNATURES, name
    assert re.search(r'#define GPRN_COV_JOINT 1\b', text) and _hip.COV_JOINT == 1


def test_library_exports_the_new_entry_points():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load_library()
    for name in NEW:
        assert hasattr(lib, name), name


def test_no_gpu_is_an_error_not_a_fallback():
    if _hip.device_count() > 0:
        pytest.skip('a GPU is present')
    import gpyrn_amd as gpyrn
    t, y, e = np.random.RandomState(0).rand(3, 12)
    g = gpyrn.inference(1, t, y, e)
    g.set_components(gpyrn.SquaredExponential(1, 1), gpyrn.SquaredExponential(1, 1), gpyrn.Constant(0), 0.1)
    assert hasattr(g, 'predict_cov') and hasattr(g, 'sample_posterior')
    with pytest.raises(_hip.BackendUnavailable):
        g.predict_cov()
    with pytest.raises(_hip.BackendUnavailable):
        g.sample_posterior(n=2)
