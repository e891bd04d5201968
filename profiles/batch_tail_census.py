"""Kernel census and device assembly of two trees in which kernels changed files (profiles/batch_tail_isa_resources.txt):
k_draw_pad_z and k_draw_combine_b moved from csrc/midn.hip to csrc/batch_tail.hip.  The inputs are those of
profiles/variant_dispatch_census.py (per source S of gpyrn_amd/csrc: S.res and S.s in each directory), and so are its readers.

Census: every kernel of every source of either tree by demangled name, whichever file it is in; the compiler's figures must be
identical.  Assembly: a source both trees have with the same kernels is compared line for line; the sources a kernel left or
entered are pooled and compared function by function (variant_dispatch_census.units: each function with its kernel
descriptor, labels less their ordinals; the lines outside functions -- metadata, head, tail -- as a set).

usage: python profiles/batch_tail_census.py PARENT_DIR THIS_DIR   (exit status 1 on any difference)"""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from variant_dispatch_census import assembly, census, demangle, units  # noqa: E402


def main(parent, this):
    names = lambda d: sorted(os.path.basename(f)[:-4] for f in glob.glob(d + '/*.res'))
    ok = True
    kern = {}
    for tag, d in (('parent', parent), ('this', this)):
        kern[tag] = {}
        for s in names(d):
            c = census('%s/%s.res' % (d, s))
            dm = demangle(list(c))
            for k, fig in c.items():
                assert dm[k] not in kern[tag], dm[k]
                kern[tag][dm[k]] = (s, fig)
    pa, th = kern['parent'], kern['this']
    print('kernels by demangled name: parent %d, this %d; gone %s; new %s' % (
        len(pa), len(th), sorted(set(pa) - set(th)), sorted(set(th) - set(pa))))
    ok = ok and set(pa) == set(th)
    differ = [k for k in pa if k in th and pa[k][1] != th[k][1]]
    print('figures (SGPRs, VGPRs, AGPRs, scratch, occupancy, spills, LDS) differ for: %s' % (differ or 'none'))
    ok = ok and not differ
    moved = sorted(k for k in pa if k in th and pa[k][0] != th[k][0])
    for k in moved:
        print('    moved %s.hip -> %s.hip: %s' % (pa[k][0], th[k][0], k.split('(')[0]))
    pooled = sorted({pa[k][0] for k in moved} | {th[k][0] for k in moved})
    for s in sorted(set(names(parent)) | set(names(this))):
        n = (sum(1 for v in pa.values() if v[0] == s), sum(1 for v in th.values() if v[0] == s))
        if s in pooled:
            print('%-16s %3d kernels -> %3d; pooled below' % (s + '.hip', n[0], n[1]))
            continue
        a, b = assembly('%s/%s.s' % (parent, s)), assembly('%s/%s.s' % (this, s))
        same = a == b
        ok = ok and same
        print('%-16s %3d kernels -> %3d; assembly (%d lines) %s' % (s + '.hip', n[0], n[1], len(b), 'identical' if same else 'DIFFERS'))
    if pooled:
        def pool(d):
            fn, rest = [], []
            for s in pooled:
                if os.path.exists('%s/%s.s' % (d, s)):
                    u = units(assembly('%s/%s.s' % (d, s)))
                    fn += u[0]
                    rest += u[1]
            return sorted(fn), sorted(set(rest))
        (fa, ra), (fb, rb) = pool(parent), pool(this)
        same = fa == fb
        ok = ok and same
        print('%s pooled: %d functions (code, kernel descriptor, compiler comments) -> %d, %s; lines outside functions (metadata, head, tail): %s' % (
            ' + '.join(s + '.hip' for s in pooled), len(fa), len(fb),
            'every one identical' if same else 'DIFFER', 'the same set' if ra == rb else 'DIFFER'))
        ok = ok and ra == rb
    print('verdict: %s' % ('same kernels, same figures, same code' if ok else 'DIFFERENCES'))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(*sys.argv[1:3])
