"""Child process of tests/test_fill_gpu.py: every case of tests/golden/fill_highprec filled on the device by
gprn_eval_kernel, in a process of its own so that the environment it inherits (GPRN_FILL_SYM=0: the full-matrix
fill instead of the symmetric one, read once per process) takes effect.  Usage: python -m tests._fill_worker OUT.npz"""
import sys

import numpy as np

from gpyrn_amd import _hip
from tests import _fill_fixture as ff


def fill_all():
    cases, d = ff.load()
    out, ctxs = {}, {}
    for c in cases:
        ctx = ctxs.get(c['tset'])
        if ctx is None:
            t = d['t_' + c['tset']]
            ctx = ctxs[c['tset']] = _hip.Context(0)
            ctx.set_data(t, np.zeros((1, t.size)), np.ones((1, t.size)), 1)
        out[c['name']] = ctx.eval_kernel(c['ops'], c['pars'], 0.0)
    for ctx in ctxs.values():
        ctx.close()
    return out


if __name__ == '__main__':
    np.savez(sys.argv[1], **fill_all())
