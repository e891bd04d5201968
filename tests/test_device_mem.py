"""Device and pinned memory has one allocator and two owners (gpyrn_amd/csrc/device_mem.h).  tests/device_mem_check.cpp, a
program that includes nothing but that header and puts malloc / free under it, is compiled with the host compiler under the
address and undefined-behaviour sanitizers and walks DeviceOwner and DevBuf through every path, each allocation of a sequence
failing in turn; a source test holds the four HIP allocation calls to the allocator's definition and the context's grow-only
buffers to DevBuf.  No GPU, no HIP."""
import glob
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'gpyrn_amd', 'csrc')
CXX = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
SANITIZE = '-fsanitize=address,undefined'


@pytest.mark.skipif(CXX is None, reason='no host C++ compiler')
def test_owners_walk_clean_under_sanitizers(tmp_path):
    # (a toolchain without the sanitizers' runtime cannot link even an empty program with them: the walk then runs plain)
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    have = subprocess.run([CXX, SANITIZE, str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode == 0
    print('sanitizers:', 'on' if have else 'NOT available to %s, plain build' % CXX)
    exe = str(tmp_path / 'device_mem_check')
    subprocess.run([CXX, '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + ([SANITIZE, '-fno-sanitize-recover=all'] if have else []) +
                   ['-I', CSRC, os.path.join(HERE, 'device_mem_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 live, 0 failures' in run.stdout and not run.stderr.strip(), run.stdout + run.stderr


def _code(text):
    """C++ source without its comments and the contents of its string literals."""
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def test_one_allocator():
    names = re.compile(r'\bhip(?:Malloc|Free|HostMalloc|HostFree)\b')
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert len(files) > 20
    for path in files:
        code = _code(open(path).read())
        if os.path.basename(path) == 'api.hip':
            # the definitions of the four raw functions, one block: from the first's signature to the last's closing brace
            start = code.index('int mem_dev_alloc(void** p')
            end = code.index('\n', code.index('void mem_pin_free(void* p)'))
            inside = code[start:end]
            assert len(names.findall(inside)) == 4 and inside.count('\n') < 32, inside
            code = code[:start] + code[end:]
        hits = [ln.strip() for ln in code.split('\n') if names.search(ln)]
        assert not hits, (os.path.basename(path), hits)
    # ... and no grow-by-hand pair is left in the context: a DevBuf carries its capacity
    header = _code(open(os.path.join(CSRC, 'gprn_internal.h')).read())
    ctx = header[header.index('struct gprn_ctx {'):header.index('void release_slots(')]
    bufs = re.findall(r'DevBuf<[^;]*?>\s*([^;]+);', ctx)
    bufs = [re.sub(r'[\[{].*', '', n).strip() for decl in bufs for n in decl.split(',')]
    assert {'tasks', 'sig', 'test', 'out', 'mu_old', 'pin_in', 'pin_out', 'grad_scratch'} <= set(bufs), bufs
    fields = set(re.findall(r'\b(\w+_(?:cap|bytes))\b', ctx))
    gone = {b + s for b in bufs for s in ('_cap', '_bytes')}
    assert not fields & gone, fields & gone
    assert not re.search(r'\bd_w\b', ctx)
