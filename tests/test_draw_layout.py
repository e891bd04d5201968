"""The layout of the draw pass's scratch (gpyrn_amd/csrc/batch_layout.h draw_scratch, behind gprn_elbocalc_batch_draws):
tests/draw_layout_check.cpp, a program that includes nothing but that header, is compiled with the host compiler and walks the
layout function over small shapes -- the size from the null base against the real walk, alignment, bounds, disjoint ranges,
the contiguous pointer tables, every row block the pass addresses.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'gpyrn_amd', 'csrc')
CXX = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason='no host C++ compiler')
def test_the_draw_scratch_layout_walks_clean(tmp_path):
    exe = str(tmp_path / 'draw_layout_check')
    subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, os.path.join(HERE, 'draw_layout_check.cpp'), '-o', exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failures' in run.stdout
