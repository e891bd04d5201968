"""The switch that lets the side-by-side forms run under a data mask (inference(..., batch_under_mask=), option
"batch_mask" of the library): what needs no device."""
import os
import re

import numpy as np

import gpyrn_amd as gpyrn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data():
    rng = np.random.RandomState(3)
    t = np.linspace(0.0, 9.0, 10)
    return t, rng.randn(2, 10), 0.1 + 0.1 * rng.rand(2, 10)


def _components(g):
    g.set_components(gpyrn.SquaredExponential(1, 1), [gpyrn.SquaredExponential(1, 1)] * 2,
                     [gpyrn.Constant(0), gpyrn.Constant(0)], [0.1, 0.1])
    return g


def test_the_keyword_decides_whether_a_masked_object_is_batchable():
    t, y, e = _data()
    m = np.ones((2, 10), dtype=bool)
    m[0, 2] = False
    args = [y[0], e[0], y[1], e[1]]
    off = _components(gpyrn.inference(1, t, *args, mask=m))
    assert off.batch_under_mask is False and not off._batchable()
    on = _components(gpyrn.inference(1, t, *args, mask=m, batch_under_mask=True))
    assert on.batch_under_mask is True and on._batchable()
    # an attribute, as batch_max_N: it may be set later
    off.batch_under_mask = True
    assert off._batchable()
    off.batch_under_mask = False
    assert not off._batchable()
    # the other obstacles stay obstacles
    on.batch_max_N = 5
    assert not on._batchable()
    del on.batch_max_N
    assert on._batchable()

    class FakeComm:
        world, rank, local_rank = 2, 0, 0
    on._comm = FakeComm()
    assert not on._batchable()
    on._comm = None
    assert on._batchable()
    # without a mask the keyword changes nothing
    assert _components(gpyrn.inference(1, t, *args))._batchable()
    assert _components(gpyrn.inference(1, t, *args, batch_under_mask=True))._batchable()


def test_from_series_passes_the_keyword_through():
    rng = np.random.RandomState(5)
    t1, t2 = np.sort(rng.rand(8)) * 10, np.sort(rng.rand(7)) * 10
    series = [(t1, rng.randn(8), np.full(8, 0.1)), (t2, rng.randn(7), np.full(7, 0.1))]
    off = _components(gpyrn.inference.from_series(1, series))
    on = _components(gpyrn.inference.from_series(1, series, batch_under_mask=True))
    assert off.mask is not None and not off.mask.all()
    assert not off._batchable() and on._batchable()


def test_the_header_names_the_option():
    text = open(os.path.join(ROOT, 'include', 'gprn_hip.h')).read()
    assert '"batch_mask"' in text
    # in gprn_set_option's list and in the refusal paragraphs of gprn_elbocalc_batch* and gprn_set_mask
    assert len(re.findall(r'"batch_mask"', text)) >= 4
