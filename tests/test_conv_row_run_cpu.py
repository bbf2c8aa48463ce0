"""The index map of the row-run activation path (csrc/conv_row_run.h: flat pixel of a tile's run <-> LDS row, separator rows)
checked exhaustively on the host: tests/conv_row_run_check.cpp includes the header the kernels include, is compiled with the host
compiler and run.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'background-debiased-video-cil_amd', 'csrc')


def _compiler():
    for cxx in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++', '/opt/rocm/bin/hipcc'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail('no host C++ compiler found (the library itself needs hipcc)')


def test_row_run_index_map(tmp_path):
    exe = str(tmp_path / 'conv_row_run_check')
    subprocess.run([_compiler(), '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, os.path.join(HERE, 'conv_row_run_check.cpp'), '-o', exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # 3 tile heights x sum of W over 1..300 starts
    assert r.stdout.split() == ['ok', str(3 * 300 * 301 // 2)]


def test_setter_is_bound():
    """The switch is exported, declared and in the binding's table; 0 / 1 only."""
    import bdvcil_amd as bd
    lib = bd._lib.lib()
    assert lib.bdv_conv_debug_row_run(0) == 0
    assert lib.bdv_conv_debug_row_run(1) == 0
    assert lib.bdv_conv_debug_row_run(2) != 0
    with open(os.path.join(os.path.dirname(HERE), 'include', 'bdvcil_hip.h')) as f:
        assert 'int bdv_conv_debug_row_run(int on);' in f.read()
