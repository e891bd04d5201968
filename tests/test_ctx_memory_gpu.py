"""A context gives back what it took (gprn_ctx::Mem: one owner per lifetime).  The library counts its device and pinned
allocations (options "live_allocs" / "allocs_made", process-wide); every scenario of tests/_ctx_memory.py reads them through a
probe context made first, runs on a second context, destroys it, and only differences are compared -- other fixtures may hold
contexts of their own.  One tile (N = 45), two tiles (N = 200), and q = 1 with a fully masked time.  The steady-state calls are
held to the counts of the commit BEFORE the owners (profiles/ctx_alloc_counts.json, table "parent": that commit with nothing
but the two counters patched into its allocation calls), not to numbers taken from this tree."""
import functools
import json
import os

import pytest

from tests import _ctx_memory as M

pytestmark = pytest.mark.gpu
PARENT = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                     'ctx_alloc_counts.json')))['parent']


@functools.lru_cache(maxsize=None)
def _life_cycle(shape):
    rows = M.life_cycle(shape)
    print(shape, rows)
    return rows


def _live(rows):
    return {step: live for step, _, live in rows}


@pytest.mark.parametrize('shape', list(M.SHAPES))
def test_life_cycle_gives_everything_back(shape):
    rows = _life_cycle(shape)
    live = _live(rows)
    assert live['create'] == 0                       # (a context without a problem holds no memory)
    assert live['set_up'] > 0 and live['elbocalc_batch_heldout'] > live['set_up']
    assert live['destroy'] == 0, rows


def test_set_data_again_holds_what_the_first_time_held():
    """N = 200, N = 45, N = 200 again on one context: the same shape holds the same number of allocations both times.  (What
    lives as long as the context -- the factorisation's task lists and signals, made by the two-tile sweeps -- stays through the
    one-tile problem, so that one is not compared with a fresh context.)"""
    rows = M.reuse_data()
    print(rows)
    live = _live(rows)
    assert live['set_up two_tiles #0'] == live['set_up two_tiles #2']
    assert live['sweep x3 #0'] == live['sweep x3 #2']
    assert 0 < live['set_up one_tile #1'] <= live['sweep x3 #1']
    assert live['destroy'] == 0, rows


@pytest.mark.parametrize('shape', list(M.SHAPES))
def test_mask_set_cleared_set(shape):
    rows = M.reuse_mask(shape)
    print(rows)
    live = _live(rows)
    assert live['mask'] > live['unmasked'] and live['second mask'] > live['unmasked']
    assert live['mask cleared'] == live['unmasked']
    assert live['destroy'] == 0, rows


@pytest.mark.parametrize('shape', ['one_tile', 'two_tiles'])
def test_elbo_form_change_frees_the_batch(shape):
    rows = M.elbo_form_frees_batch(shape)
    print(rows)
    live = _live(rows)
    assert live['elbocalc_batch'] > live['set_up']
    assert live['elbo_form changed'] == live['set_up']        # (down by exactly what the batch took)
    assert live['destroy'] == 0, rows


@pytest.mark.parametrize('shape', ['one_tile', 'two_tiles'])
def test_sequential_order_under_a_mask(shape):
    rows = M.sequential_under_mask(shape)
    print(rows)
    assert rows[-2][2] > 0 and rows[-1][2] == 0, rows


@pytest.mark.parametrize('shape', ['one_tile', 'two_tiles'])       # the small path, the launch path
def test_second_call_allocates_no_more_than_before_the_owners(shape):
    rows = M.steady(shape)
    print(rows)
    now, before = M.second_call_allocs(rows), M.second_call_allocs(PARENT['steady/' + shape])
    assert set(now) == set(before) == {'sweep', 'elbocalc', 'elbocalc_batch'}
    for call in now:
        assert now[call] <= before[call], (call, now[call], before[call])
    live = _live(rows)
    for call in now:                                 # ... and keeps nothing more than the warm call left
        assert live[call + ' second'] == live[call + ' warm']
    assert live['destroy'] == 0, rows
