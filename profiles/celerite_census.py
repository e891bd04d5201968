"""Kernel census of two trees side by side (profiles/celerite_isa_resources.txt): the parent against the tree with the celerite
kernel ids.  Directories as profiles/variant_dispatch_census.py takes them -- for every source S of gpyrn_amd/csrc S.res, the
output of

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I/opt/rocm/include --cuda-device-only \
          -Rpass-analysis=kernel-resource-usage -c S.hip -o /dev/null

and S.s, the same with -S -o S.s.  Usage: python profiles/celerite_census.py PARENT_DIR THIS_DIR

Per source: the kernels whose figures moved (old -> new), the kernels that are new with their figures, whether any kernel
uses scratch that did not on the parent, whether a VGPR count crossed an occupancy step, and whether the assembly of the
file is the parent's line for line."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from variant_dispatch_census import assembly, census, demangle, units  # noqa: E402

SOURCES = ('smalln', 'vecops', 'order', 'gemm_tile', 'grad', 'api_more', 'factor', 'mask', 'midn', 'fill', 'api', 'api_sweep',
           'api_test', 'batch_tail', 'mean')
KEYS = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]')


def figures(lines):
    d = dict(l.split(': ', 1) for l in lines if ': ' in l)
    return {k: d.get(k, '?') for k in KEYS}


def short(f):
    return 'SGPR %s VGPR %s AGPR %s scratch %s occupancy %s LDS %s' % tuple(f[k] for k in KEYS)


def main(parent, this):
    total = [0, 0]
    new_scratch, steps = [], []
    for s in SOURCES:
        a, b = census('%s/%s.res' % (parent, s)), census('%s/%s.res' % (this, s))
        da, db = demangle(list(a)), demangle(list(b))
        total[0] += len(a)
        total[1] += len(b)
        old = {da[k]: figures(a[k]) for k in a}
        new = {db[k]: figures(b[k]) for k in b}
        moved = [n for n in old if n in new and old[n] != new[n]]
        gone = [n for n in old if n not in new]
        added = [n for n in new if n not in old]
        ta, tb = assembly('%s/%s.s' % (parent, s)), assembly('%s/%s.s' % (this, s))
        same = 'identical' if ta == tb else ('identical but for the order of emission' if units(ta) == units(tb) else 'differs')
        print('%-15s %3d kernels -> %3d: %d moved, %d new, %d gone; assembly (%d lines) %s'
              % (s + '.hip', len(a), len(b), len(moved), len(added), len(gone), len(tb), same))
        for n in moved:
            print('    moved: %s\n        %s\n     -> %s' % (n.split('(')[0], short(old[n]), short(new[n])))
            if old[n][KEYS[4]] != new[n][KEYS[4]]:
                steps.append(n.split('(')[0])
        for n in gone:
            print('    gone:  %s' % n.split('(')[0])
        for n in added:
            print('    new:   %s\n        %s' % (n.split('(')[0], short(new[n])))
        for n in new:
            if new[n][KEYS[3]] != '0' and (n not in old or old[n][KEYS[3]] == '0'):
                new_scratch.append(n.split('(')[0])
    print('total: %d kernels -> %d' % tuple(total))
    print('kernels with scratch that had none on the parent (or are new): %s' % (', '.join(new_scratch) or 'none'))
    print('existing kernels whose occupancy changed: %s' % (', '.join(steps) or 'none'))


if __name__ == '__main__':
    main(*sys.argv[1:3])
