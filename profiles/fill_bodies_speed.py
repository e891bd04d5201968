"""Speed of this build against the parent commit's build after the covariance fills were folded onto one body per shape
(csrc/fill.hip), by the standing rule (profiles/batch_tail_speed.py, whose legs and verdict these are): every leg in FRESH
processes that alternate parent / this tree / parent, every repetition kept, and per leg this tree's median must be no slower
than the parent's own SLOWEST repetition on the same box.

Stages (--stages, default all; each adds its part to --out, the verdicts are recomputed over everything in the file):

* bench    bench.py --gpus 1 --steps 20 --warmup 3 (the headline), bench.py --latency --latency-cpu-s 1 --latency-mcmc 0, and
           the fill pass bench.py times with --full (gprn_test_fill_rate: the set-up's fills launch behind launch in one event
           bracket, `fill.kernel_GBps` of its record) as a leg of its own;
* predict  profiles/predict_batch_timing.py of each tree (its own package and library): predict_batch from states, side by side;
* varpred  profiles/varpred_batch_timing.py --leg this TREE: predict_batch(from_sweeps=True) and nELBO_batch alone;
* draw     profiles/draw_batch_timing.py --leg this TREE: sample_posterior_batch side by side, one by one, nELBO_batch.

usage: python profiles/fill_bodies_speed.py --parent-tree DIR [--out FILE] [--stages bench,predict,varpred,draw] [--rounds R]
Exit status: 1 when a process failed or any leg is outside the bound, else 0."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_tail_speed import HERE, bench_leg, run, script_leg, verdicts  # noqa: E402


def predict_leg(tree):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'p.json')
        run([sys.executable, os.path.join(tree, 'profiles', 'predict_batch_timing.py'), '--out', out, '--reps', '9'], cwd=tree)
        res = {}
        for s in json.load(open(out))['shapes']:
            for k in ('side_by_side_both_pairs', 'side_by_side_outputs_only'):
                res['N%d_%s_ms_per_call' % (s['N'], k)] = s[k]['ms_per_call']
            assert s['fallbacks'] == 0 and s['all_finite']
        return res


def fill_pass_leg(tree):
    for ln in run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '5', '--warmup', '2', '--full', '--no-cpu'], cwd=tree).splitlines():
        if ln.startswith('{') and (json.loads(ln).get('fill') or {}).get('kernel_GBps'):
            return {'fill pass of the set-up, config 3 [GB/s]': json.loads(ln)['fill']['kernel_GBps']}
    raise RuntimeError('bench.py --full printed no fill pass')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', required=True)
    ap.add_argument('--out', default='fill_bodies_vs_parent.json')
    ap.add_argument('--stages', default='bench,predict,varpred,draw')
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_tree)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {'stages': {}}
    res.pop('error', None)
    stages = {'bench': (bench_leg(['--gpus', '1', '--steps', '20', '--warmup', '3']), a.rounds),
              'bench_latency': (bench_leg(['--latency', '--latency-cpu-s', '1', '--latency-mcmc', '0']), a.rounds),
              'bench_fill': (fill_pass_leg, a.rounds),
              'predict': (predict_leg, a.rounds),
              'varpred': (lambda t: script_leg('varpred_batch_timing.py', t), a.rounds),
              'draw': (lambda t: script_leg('draw_batch_timing.py', t), a.rounds)}
    want = a.stages.split(',')
    if 'bench' in want:
        want[want.index('bench') + 1:want.index('bench') + 1] = ['bench_latency', 'bench_fill']
    failed = None
    try:
        for name in want:
            leg, rounds = stages[name]
            st = res['stages'][name] = {'runs': {'parent_a': [], 'this': [], 'parent_b': []}, 'rounds_done': 0}
            for r in range(rounds):
                for o in ('parent_a', 'this', 'parent_b'):
                    st['runs'][o].append(leg(HERE if o == 'this' else parent))
                st['rounds_done'] = r + 1
                print(name, 'round', r + 1, json.dumps({o: st['runs'][o][-1] for o in st['runs']}), flush=True)
                with open(a.out, 'w') as f:
                    json.dump(res, f, indent=1)
    except BaseException as e:
        failed = '%s: %s' % (type(e).__name__, e)
        res['error'] = failed
    res['verdict'] = verdicts(res)
    res['all_legs_no_slower_than_the_parents_slowest'] = all(v['this_median_no_slower_than_parent_slowest'] for v in res['verdict'])
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    for v in res['verdict']:
        print('%-13s %-70s parent %s this %s median %.6g (x%.3f of the parent median) %s' % (
            v['stage'], v['leg'], ' '.join('%.6g' % x for x in v['parent_runs']), ' '.join('%.6g' % x for x in v['this_runs']),
            v['this_median'], v['this_median_over_parent_median'],
            'ok' if v['this_median_no_slower_than_parent_slowest'] else 'SLOWER than the parent\'s slowest'), flush=True)
    sys.exit(1 if failed or not res['all_legs_no_slower_than_the_parents_slowest'] else 0)


if __name__ == '__main__':
    main()
