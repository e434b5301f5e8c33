"""The block matrices of a spectral conv as one function for host and device: csrc/spectral_weights.h, checked by a stand-alone
host program (tests/spectral_weights_check.cpp: its own main, nothing loaded into Python) built with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and without FMA contraction.  The program carries the host loop nest the library
used before the header existed and compares the header's element function with it bit for bit at every (bin, row, column), for
(T, cin, cout) = (15, 24, 40), (3, 32, 32), (1, 5, 3) at F = 16, 30, 50, each with a random kernel, a kernel with one all-zero
output channel and an all-zero kernel (the -0 case).  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'x-detector_amd', 'csrc')


def test_element_function_equals_the_host_loop_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'spectral_weights_check')
    cxx = os.environ.get('CXX', 'c++')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-ffp-contract=off', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, os.path.join(ROOT, 'tests', 'spectral_weights_check.cpp'),
                           '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, (out, err)
    assert 'runtime error' not in err and 'AddressSanitizer' not in err, err
    assert out.startswith('ok: '), out


def test_the_library_builds_its_block_matrices_from_the_header():
    """spectral.hip no longer holds a second statement of the map, and the refresh kernels' unit is compiled without contraction"""
    from xdet import build
    text = open(os.path.join(CSRC, 'spectral.hip')).read()
    assert 'void spectral_weights(' not in text and 'void spectral_tables(' not in text
    assert ('conv_repack.hip', ['-ffp-contract=off']) in build.SOURCES
    assert 'spectral_weight_element' in open(os.path.join(CSRC, 'conv_repack.hip')).read()
