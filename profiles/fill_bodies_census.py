"""Kernel census of two trees after the covariance fills were folded onto one body per shape
(profiles/fill_bodies_isa_resources.txt).  The inputs are those of profiles/variant_dispatch_census.py: per changed source S
of gpyrn_amd/csrc (fill, grad, api_more) each directory holds S.res and S.s.

Per kernel, by demangled name: the same set; occupancy not lower; scratch and LDS not larger; VGPRs + AGPRs not above the
parent's unless occupancy is unchanged (then listed).  Every kernel whose figures moved is printed with both sets of
figures.  Assembly: line for line per source, and where it differs the functions that do.

usage: python profiles/fill_bodies_census.py PARENT_DIR THIS_DIR   (exit status 1 if a requirement fails)"""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from variant_dispatch_census import assembly, census, demangle, units  # noqa: E402

KEYS = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'SGPRs Spill', 'VGPRs Spill',
        'LDS Size [bytes/block]')


def figures(lines):
    d = dict(l.split(': ') for l in lines if ': ' in l)
    return {k: int(d[k]) for k in KEYS}


def short(name):
    return re.sub(r'^void ', '', name.split('(')[0])


def main(parent, this):
    ok = True
    for s in sorted(os.path.basename(f)[:-4] for f in glob.glob(this + '/*.res')):
        a, b = census('%s/%s.res' % (parent, s)), census('%s/%s.res' % (this, s))
        da, db = demangle(list(a)), demangle(list(b))
        pa, th = {da[k]: figures(a[k]) for k in a}, {db[k]: figures(b[k]) for k in b}
        same_set = set(pa) == set(th)
        ok = ok and same_set
        ta, tb = assembly('%s/%s.s' % (parent, s)), assembly('%s/%s.s' % (this, s))
        print('%s.hip: %d kernels -> %d, %s; assembly (%d lines) %s' % (
            s, len(pa), len(th), 'the same set' if same_set else 'gone %s, new %s' % (sorted(set(pa) - set(th)), sorted(set(th) - set(pa))),
            len(tb), 'identical line for line' if ta == tb else 'differs'))
        if ta != tb:
            fa, fb = units(ta)[0], units(tb)[0]
            name = lambda u: next((l.split()[0].rstrip(':') for l in u if re.match(r'^_Z\w+:', l)), '?')
            diff = sorted(set(demangle([name(u) for u in set(fb) - set(fa)]).values()))
            print('  functions whose code, descriptor or compiler comments differ (%d of %d): %s' % (
                len(diff), len(fb), ', '.join(short(x) for x in diff)))
        moved = [k for k in sorted(pa) if k in th and pa[k] != th[k]]
        print('  kernels whose figures moved: %d' % len(moved))
        for k in moved:
            p, t = pa[k], th[k]
            bad = []
            if t[KEYS[4]] < p[KEYS[4]]:
                bad.append('OCCUPANCY LOWER')
            if t[KEYS[3]] > p[KEYS[3]]:
                bad.append('SCRATCH LARGER')
            if t[KEYS[7]] > p[KEYS[7]]:
                bad.append('LDS LARGER')
            if t['VGPRs'] + t['AGPRs'] > p['VGPRs'] + p['AGPRs']:
                bad.append('VGPRs + AGPRs above the parent\'s' + (' (occupancy unchanged: listed)' if t[KEYS[4]] == p[KEYS[4]] else ', OCCUPANCY CHANGED'))
            ok = ok and not any(x.isupper() or 'CHANGED' in x for x in bad)
            print('    %-34s %s%s' % (short(k), '  '.join('%s %d -> %d' % (key.split(' [')[0], p[key], t[key]) for key in KEYS if p[key] != t[key]),
                                      ('   ** ' + '; '.join(bad)) if bad else ''))
    print('verdict: %s' % ('every requirement met' if ok else 'A REQUIREMENT FAILS'))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main(*sys.argv[1:3])
