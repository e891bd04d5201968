"""The Python layer of the side-by-side API, pinned call for call: profiles/host_layer_trace.py drives the public batch methods
over a recording stand-in for the device context, and what it records -- the order and the arguments of every context call,
the return values, the state the object keeps -- must be what profiles/host_layer_trace.json holds.  That file was written
by the same script and is byte-identical on the commit that folded the layer's copies and on its parent."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location('host_layer_trace', os.path.join(ROOT, 'profiles', 'host_layer_trace.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_host_layer_hands_the_context_what_it_always_did():
    script = _script()
    record = json.loads(json.dumps(script.condense(script.run())))
    with open(os.path.join(ROOT, 'profiles', 'host_layer_trace.json')) as f:
        stored = json.load(f)
    differing = [(path, group) for path, groups in stored['digests'].items() for group in groups
                 if record['digests'].get(path, {}).get(group) != groups[group]]
    assert not differing, differing[:10]
    assert record == stored
    # every branch was taken: the side-by-side entries, the one-by-one forms, refusals and failed vectors
    for name in ('elbocalc_batch', 'elbocalc_batch_predict', 'elbocalc_batch_draws', 'elbocalc_batch_heldout', 'predict_batch',
                 'sweep', 'elbocalc', 'predict', 'predict_draws', 'grad_elbo', 'eval_mean', 'eval_mean_grad', 'set_mean'):
        assert name in stored['calls_seen'], name
    assert stored['cases'] > 600 and stored['raised'] > 0 and stored['left_last_info'] > 0
