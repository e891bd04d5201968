"""One rank of a two-rank sharded object asked for full predictive covariances (started by test_predict_cov_gpu.py).

usage: python -m tests._cov_shard_worker <tag> <out.npz> <rendezvous tag>, RANK / WORLD_SIZE / LOCAL_RANK in the environment.
"""
import sys

import numpy as np

import gpyrn_amd as gpyrn
from gpyrn_amd import _hip, covfunc, meanfunc, sharding
from tests import _cases


def main(tag, out, uid_tag):
    meta, d = _cases.load(tag)
    nodes, weights, means, jit = _cases.components(meta, covfunc, meanfunc)
    comm = sharding.Comm(tag=uid_tag)
    g = gpyrn.inference(meta['q'], np.array(d['time']), *_cases.data_args(d), comm=comm)
    g.set_components(nodes, weights, means, jit)
    g._mu, g._var = d['mu_final'], d['var_final']
    msgs = []
    for call in (lambda: g.predict_cov(), lambda: g.sample_posterior(n=2, rng=0)):
        try:
            call()
            msgs.append('no error')
        except _hip.BackendError as exc:
            msgs.append(str(exc))
    np.savez(out, rank=comm.rank, world=comm.world, messages=np.array(msgs))
    comm.cleanup()


if __name__ == '__main__':
    main(*sys.argv[1:4])
