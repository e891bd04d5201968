"""Kernel census and device assembly of two trees, side by side (profiles/variant_dispatch_isa_resources.txt).

For every source S of gpyrn_amd/csrc each directory holds S.res, the output of

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I/opt/rocm/include --cuda-device-only \
          -Rpass-analysis=kernel-resource-usage -c S.hip -o /dev/null

and S.s, the same command with -S -o S.s.  Usage: python profiles/variant_dispatch_census.py PARENT_DIR THIS_DIR

Census: per kernel the figures the compiler reports (SGPRs, VGPRs, AGPRs, scratch, occupancy, spills, LDS), compared by
demangled name; the one-tile kernels of smalln.hip after RENAME below.  Assembly: each file less the lines with file paths and
the __hip_cuid_* names, line for line; smalln.hip after ONE substitution of the parent's mangled kernel names by this tree's.
"""
import re
import subprocess
import sys

SOURCES = ('smalln', 'vecops', 'order', 'gemm_tile', 'grad', 'api_more', 'factor', 'mask', 'midn', 'fill', 'api', 'api_sweep', 'api_test')

# parent wrapper -> (this tree's wrapper, how its template arguments map)
RENAME = {
    'k_small_phase': ('k_small_phase', lambda w, t: (w, t, 'false')),
    'k_small_phase_m': ('k_small_phase', lambda w, t: (w, t, 'true')),
    'k_small_phase_b': ('k_small_phase_b', lambda w: (w, 'false')),
    'k_small_phase_bm': ('k_small_phase_b', lambda w: (w, 'true')),
    'k_small_tail': ('k_small_tail', lambda t: (t, 'false', 'false')),
    'k_small_tail_m': ('k_small_tail', lambda t: (t, 'true', 'false')),
    'k_small_tail_bound': ('k_small_tail', lambda t, m: (t, m, 'true')),
    'k_small_tail_b': ('k_small_tail_b', lambda t, f: (t, 'false', f, 'false')),
    'k_small_tail_bm': ('k_small_tail_b', lambda t, f: (t, 'true', f, 'false')),
    'k_small_tail_bound_b': ('k_small_tail_b', lambda t, m, f: (t, m, f, 'true')),
}


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, out))


def renamed(demangled):
    m = re.match(r'void (k_small_\w+)<([^>]*)>(\(.*)$', demangled)
    if not m or m.group(1) not in RENAME:
        return demangled
    name, args = RENAME[m.group(1)]
    return 'void %s<%s>%s' % (name, ', '.join(args(*[a.strip() for a in m.group(2).split(',')])), m.group(3))


def census(path):
    """{mangled name: (figure lines)}"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.search(r'remark:\s+(.*?) \[-Rpass-analysis', line)
        if m and cur is not None:
            cur.append(m.group(1))
    return {k: tuple(v) for k, v in out.items()}


def assembly(path):
    return [l for l in open(path).read().split('\n') if not re.search(r'__hip_cuid_|^\s*\.file\s|\.hip"|/opt/rocm', l)]


def units(lines):
    """The file as a multiset of pieces that do not depend on the order in which the functions were emitted: one per function
    (its section, code, kernel descriptor and the compiler's comments; labels and the comments that name them less the
    function's ordinal, runs of blanks as one), one per kernel
    of the metadata, and what is left (head, LDS variables, tail) as sorted lines."""
    lines = [re.sub(r'\s+', ' ', re.sub(r'\b(LBB|BB|Lfunc_begin|Lfunc_end|Ltmp|LJTI|LCPI|Lpost_getpc)\d+', r'\1', l)) for l in lines]
    starts = [i - 1 for i, l in enumerate(lines) if '; -- Begin function' in l]
    meta = [i for i, l in enumerate(lines) if l.startswith('  - .agpr_count:') or l.startswith('amdhsa.target')]
    tail = next(i for i in range(starts[-1] if starts else 0, len(lines)) if '.AMDGPU.gpr_maximums' in lines[i])
    if lines[tail - 2].startswith(' .p2alignl'):               # (the padding behind the last function: .text, .p2alignl, .fill)
        tail -= 3
    cuts = starts + [tail] + meta + [len(lines)]
    out = [tuple(lines[a:b]) for a, b in zip(cuts, cuts[1:]) if a not in (tail, meta[-1] if meta else -1)]
    rest = lines[:cuts[0]] + lines[tail:meta[0] if meta else len(lines)] + (lines[meta[-1]:] if meta else [])
    return sorted(out), sorted(rest)


def main(parent, this):
    total = [0, 0]
    for s in SOURCES:
        a, b = census('%s/%s.res' % (parent, s)), census('%s/%s.res' % (this, s))
        da, db = demangle(list(a)), demangle(list(b))
        total[0] += len(a)
        total[1] += len(b)
        new_by_name = {db[k]: k for k in b}
        sub, bad = {}, []
        for k in a:
            want = renamed(da[k])
            if want not in new_by_name:
                bad.append('gone: ' + da[k])
            elif a[k] != b[new_by_name[want]]:
                bad.append('figures differ: %s: %s -> %s' % (da[k], a[k], b[new_by_name[want]]))
            elif want != da[k]:
                sub[k] = new_by_name[want]
                print('    %-62s -> %-52s %s' % (da[k].split('(')[0][5:], want.split('(')[0][5:], ' '.join(
                    x.split(': ')[1] for x in a[k] if re.match(r'TotalSGPRs|VGPRs:|AGPRs|ScratchSize|Occupancy|LDS', x))))
        bad += ['new: ' + db[k] for k in b if db[k] not in {renamed(da[x]) for x in a}]
        ta, tb = '\n'.join(assembly('%s/%s.s' % (parent, s))), assembly('%s/%s.s' % (this, s))
        for old in sorted(sub, key=len, reverse=True):
            ta = ta.replace(old, sub[old])
        ta = ta.split('\n')
        same = ta == tb
        if not same and units(ta) == units(tb):
            same = 'every function, kernel descriptor and metadata entry identical, emitted in another order'
        print('%-14s %3d kernels -> %3d, %d renamed; census %s; assembly (%d lines) %s' % (
            s + '.hip', len(a), len(b), len(sub), 'identical' if not bad else 'DIFFERS', len(tb),
            'identical' if same is True else same or 'DIFFERS'))
        for x in bad:
            print('    ' + x)
    print('total: %d kernels -> %d' % tuple(total))


if __name__ == '__main__':
    main(*sys.argv[1:3])
