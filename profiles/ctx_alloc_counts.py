"""Allocations of a context, step by step: runs the scenarios of tests/_ctx_memory.py (life cycle at three shapes, re-use across
gprn_set_data / gprn_set_mask / option "elbo_form", the sequential order under a mask, steady-state second calls) and prints the
library's counters "allocs_made" / "live_allocs" after every step, relative to the scenario's start.

    python profiles/ctx_alloc_counts.py [--lib PATH] [--label NAME] [--out FILE.json]

--lib: another build of libgprn_hip.so with the same two options -- the parent commit with the two counters patched into its
allocation calls, which is how the "parent" table of profiles/ctx_alloc_counts.json was made.  --out: merge the table into that
JSON file under --label (default "tree").  tests/test_ctx_memory_gpu.py holds the steady-state calls to the parent's table."""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib')
    ap.add_argument('--label', default='tree')
    ap.add_argument('--out')
    args = ap.parse_args()
    from gpyrn_amd import _hip
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    from tests import _ctx_memory as M
    table = {}
    for name, scenario in M.all_scenarios().items():
        print(name, flush=True)
        try:
            table[name] = scenario()
        except (_hip.BackendError, AssertionError) as exc:      # (an error code of the library's or a refusal: the others still run)
            print('    FAILED: %r' % (exc,))
            gc.collect()                                         # (its contexts go now, not inside the next scenario)
            continue
        for step, made, live in table[name]:
            print('    %-32s made %5d   live %4d' % (step, made, live))
    leaks = {name: rows[-1][2] for name, rows in table.items() if rows[-1][2] != 0}
    print('live after destroy != 0:', leaks or 'nowhere')
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc[args.label] = table
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
