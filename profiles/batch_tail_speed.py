"""Speed of this build against the parent commit's build after the tail behind the batch loops became one (csrc/batch_tail.hip):
every leg in FRESH processes that alternate parent / this tree / parent, every repetition of both builds kept, and per leg the
rule of profiles/api_scratch_vs_parent.json's speed.verdict -- this tree's median must be no slower than the parent's own
SLOWEST repetition on the same box.  No margin is fixed in advance: these legs are launch-bound and the parent's own range is
the yardstick.

Stages (--stages, default all; each adds its part to --out, and the verdicts are recomputed over everything in the file):

* grad     profiles/grad_batch_timing.py of each tree (its own package and library), three processes (--grad-rounds: times
           that many), each the median of nine calls: the side-by-side call with gradients and nELBO_batch alone at its three shapes;
* varpred  profiles/varpred_batch_timing.py --leg this TREE: predict_batch(from_sweeps=True) side by side and nELBO_batch alone
           at its three shapes.  (The script's own --parent-tree mode dates from the change that ADDED the pass: it measures
           the pass on this tree only.  Both trees have it now, so the same leg runs on both.)
* draw     profiles/draw_batch_timing.py --leg this TREE likewise: sample_posterior_batch side by side, one by one, nELBO_batch;
* bench    bench.py --gpus 1 --steps 20 --warmup 3 and bench.py --latency --latency-cpu-s 1 --latency-mcmc 0, three times each.

varpred and draw run --rounds rounds (default 9) of parent_a, this, parent_b; --budget-s: no round of a stage is started that
would not fit into S seconds at the pace so far (rounds_done says how many the medians are over).  The first process that
fails is the last: the JSON holds what was taken and the error.

usage: python profiles/batch_tail_speed.py --parent-tree DIR [--out FILE] [--stages grad,varpred,draw,bench] [--rounds R]
                                           [--budget-s S] [--merge FILE ...]
(--merge: no stage runs; the stages of the named files are combined into --out)
Exit status: 1 when a process failed or any leg is outside the bound, else 0."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, cwd=None, timeout=600):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if r.returncode:
        raise RuntimeError('%s ended with status %d: %s' % (' '.join(cmd[1:4]), r.returncode, r.stderr[-500:]))
    return r.stdout


def grad_leg(tree):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'g.json')
        run([sys.executable, os.path.join(tree, 'profiles', 'grad_batch_timing.py'), '--out', out, '--reps', '9'], cwd=tree)
        res = {}
        for s in json.load(open(out))['shapes']:
            for k in ('side_by_side_with_gradients', 'nELBO_batch_alone'):
                res['N%d_%s_ms_per_call' % (s['N'], k)] = s[k]['ms_per_call']
            assert s['fallbacks'] == 0 and s['all_finite']
        return res


def script_leg(script, tree):
    out = json.loads(run([sys.executable, os.path.join(HERE, 'profiles', script), '--leg', 'this', tree]).strip().splitlines()[-1])
    assert out.pop('fallbacks') == 0
    return out


def bench_leg(args):
    def leg(tree):
        res = {}
        for ln in run([sys.executable, 'bench.py'] + args, cwd=tree).splitlines():
            if not ln.startswith('{'):
                continue
            j = json.loads(ln)
            name = (j.get('config') or {}).get('workload') or j.get('metric') or 'headline'
            res['%s [%s]' % (name, j.get('unit'))] = j['value']
            if j.get('side_by_side'):
                res['%s, side by side [%s]' % (name, j['side_by_side'].get('unit', j.get('unit')))] = j['side_by_side']['value']
        assert res
        return res
    return leg


def verdicts(res):
    out = []
    for stage, st in res['stages'].items():
        runs = st['runs']
        parent = runs.get('parent_a', []) + runs.get('parent_b', [])
        for k in sorted(runs['this'][0]) if runs.get('this') and parent else []:
            higher = '/s]' in k or 'per_s' in k                     # (rates: higher is faster; everything else is a time)
            pv, tv = [r[k] for r in parent if k in r], [r[k] for r in runs['this'] if k in r]
            slowest = min(pv) if higher else max(pv)
            med = float(np.median(tv))
            out.append({'stage': stage, 'leg': k, 'higher_is_faster': higher, 'parent_runs': pv, 'this_runs': tv,
                        'parent_fastest': max(pv) if higher else min(pv), 'parent_slowest': slowest, 'this_median': med,
                        'parent_median': float(np.median(pv)), 'this_median_over_parent_median': med / float(np.median(pv)),
                        'this_median_no_slower_than_parent_slowest': bool(med >= slowest if higher else med <= slowest)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', required=True)
    ap.add_argument('--out', default='batch_tail_vs_parent.json')
    ap.add_argument('--stages', default='grad,varpred,draw,bench')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--budget-s', type=float, default=0.0)
    ap.add_argument('--grad-rounds', type=int, default=1, help='rounds of (parent, this, parent) processes of the grad stage')
    ap.add_argument('--merge', nargs='+', default=None, help='files that hold single stages, to combine into --out')
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_tree)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {'stages': {}}
    res.pop('error', None)
    for path in a.merge or []:
        res['stages'].update(json.load(open(path))['stages'])
    stages = {'grad': (grad_leg, a.grad_rounds), 'varpred': (lambda t: script_leg('varpred_batch_timing.py', t), a.rounds),
              'draw': (lambda t: script_leg('draw_batch_timing.py', t), a.rounds),
              'bench': (bench_leg(['--gpus', '1', '--steps', '20', '--warmup', '3']), 3),
              'bench_latency': (bench_leg(['--latency', '--latency-cpu-s', '1', '--latency-mcmc', '0']), 3)}
    want = [] if a.merge else a.stages.split(',')
    if 'bench' in want:
        want.append('bench_latency')
    failed = None
    try:
        for name in want:
            leg, rounds = stages[name]
            # (grad: three processes in all; bench: parent and this alternate three times; the others: parent, this, parent per round)
            order = ('parent_a', 'this') if name.startswith('bench') else ('parent_a', 'this', 'parent_b')
            st = res['stages'][name] = {'runs': {o: [] for o in order}, 'rounds_done': 0}
            began = time.time()
            for r in range(rounds):
                if a.budget_s and r and time.time() - began > a.budget_s * r / (r + 1.0):
                    break
                for o in order:
                    st['runs'][o].append(leg(HERE if o == 'this' else parent))
                st['rounds_done'] = r + 1
                print(name, 'round', r + 1, json.dumps({o: st['runs'][o][-1] for o in order}), flush=True)
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
        print('%-8s %-70s parent %s this median %.6g (x%.3f of the parent median) %s' % (
            v['stage'], v['leg'], ' '.join('%.6g' % x for x in v['parent_runs']), v['this_median'], v['this_median_over_parent_median'],
            'ok' if v['this_median_no_slower_than_parent_slowest'] else 'SLOWER than the parent\'s slowest'), flush=True)
    sys.exit(1 if failed or not res['all_legs_no_slower_than_the_parents_slowest'] else 0)


if __name__ == '__main__':
    main()
