"""Caller-owned workspaces: the measure-or-carve walker of csrc/workspace.h, and the byte counts the size entry points return.

The walker is checked by a stand-alone host program (tests/workspace_layout_check.cpp: its own main, nothing loaded into
Python) built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer.  The sizes are part of what
callers allocate: they must stay what they were before the workspaces were described by one layout function each."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'x-detector_amd', 'csrc')


def test_walker_measures_what_it_carves_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'workspace_layout_check')
    cxx = os.environ.get('CXX', 'c++')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, os.path.join(ROOT, 'tests', 'workspace_layout_check.cpp'),
                           '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, (out, err)
    assert 'runtime error' not in err and 'AddressSanitizer' not in err, err
    assert out.startswith('ok: '), out


# Recorded from the library of the commit before the layout functions (b167e11): each entry point below was called through
# ctypes with these arguments on a machine without a GPU (the size functions touch no device) and its return value copied
# here.  0 = a refusal: arguments outside the op's limits.
RECORDED = {
    'xdet_proposals_workspace_bytes': {       # (N, n_anchor, pre_n, post_n)
        (1, 19800, 5000, 1000): 940544,
        (8, 19800, 5000, 300): 7489792,
        (63, 19800, 5000, 300): 58978560,
        (64, 19800, 5000, 300): 59913728,
        (65, 19800, 5000, 300): 60796160,     # (the cluster exchange is sized by min(N, 64))
        (3, 100, 7, 5): 375552,
    },
    'xdet_targets_workspace_bytes': {         # (N, n_candidates, G)
        (2, 0, 8): 1024,
        (2, 308, 8): 16128,
        (7, 8192, 512): 1476864,
        (1, 1, 1): 1792,
    },
    'xdet_losses_workspace_bytes': {          # (N, anchors_per_image)
        (1, 256): 104960,
        (128, 256): 625152,
        (8, 0): 100864,
        (1024, 0): 100864,
        (129, 256): 0,
        (1025, 0): 0,
    },
    'xdet_dense_backward_workspace_bytes': {  # (M, K, J)
        (70, 50, 25): 264,
        (128, 16, 16): 192,
        (129, 16, 16): 2304,
        (300, 2048, 25): 614964,
        (38400, 490, 2048): 37027904,
        (1, 4097, 1): 0,
    },
    'xdet_preprocess_train_workspace_bytes': {  # (N, G)
        (4, 8): 640,
        (1, 8): 160,
        (65535, 512): 10485600,
        (0, 8): 0,
    },
}


@pytest.mark.parametrize('entry', sorted(RECORDED))
def test_workspace_sizes_are_the_recorded_ones(entry):
    from xdet import _lib
    fn = getattr(_lib.lib(), entry)
    assert fn.restype is ctypes.c_size_t
    got = {args: fn(*args) for args in RECORDED[entry]}
    assert got == RECORDED[entry]
