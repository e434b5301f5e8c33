"""host_depthwise_backward (xdet/train_ops.py), the NumPy statement of xdet_depthwise_backward: in float64 against torch.autograd
through torch.nn.functional.conv2d(groups=C, dilation=d, padding=d) on relu(x), on every case of
tests/depthwise_backward_cases.py; the f32 statement's distance from the float64 one, which
tests/golden/depthwise_backward_f32_distance.npz records and the GPU bar for dw is read from (measured here: 9.9e-08, so 4 x it
lies under the floor and the bar is 3 * 2^-22 = 7.2e-07); the mask, the image boundary and the exact power-of-two scaling of the statement;
the argument checks of the C door and of the Python door; and the workspace size against the layout walk of
csrc/depthwise_backward_layout.h."""
import os
import subprocess
import sys

import numpy as np
import pytest

import depthwise_backward_cases as DC

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_float64_statement_against_torch(name):
    import torch
    import torch.nn.functional as F
    c = DC.make_case(name)
    d = c['dilation']
    C = c['x'].shape[3]
    (dx, dw), _ = DC.case_reference(name)
    assert dx.dtype == dw.dtype == f64 and dx.shape == c['x'].shape and dw.shape == (3, 3, C, 1)
    x = torch.tensor(np.asarray(c['x'], f64).transpose(0, 3, 1, 2), requires_grad=True)
    w = torch.tensor(np.asarray(c['k'], f64)[:, :, :, 0].transpose(2, 0, 1)[:, None], requires_grad=True)     # [C,1,3,3]
    y = F.conv2d(torch.relu(x) if c['relu_in'] else x, w, groups=C, dilation=d, padding=d)
    (y * torch.tensor(np.asarray(c['dy'], f64).transpose(0, 3, 1, 2))).sum().backward()
    tdx = x.grad.numpy().transpose(0, 2, 3, 1)
    tdw = w.grad.numpy()[:, 0].transpose(1, 2, 0)[..., None]
    assert np.abs(dx - tdx).max() <= 1e-12 * np.abs(tdx).max()
    assert np.abs(dw - tdw).max() <= 1e-12 * np.abs(tdw).max()
    if name != 'two_images':
        assert dx.any() and dw.any()


def test_f32_statement_distance_is_the_recorded_one():
    """numpy builds may order their sums differently: the recorded figure must be of the size measured here (within 2x either
    way, the rule of the batch-norm and conv-backward goldens), so the GPU bar read from the file is the bar this module
    would compute"""
    d = DC.f32_statement_distance()
    rec = float(np.load(DC.GOLDEN)['f32_distance'])
    print('f32 statement vs float64: measured %.3e, recorded %.3e -> GPU bar %.3e (floor %.3e)' % (d, rec, DC.bar(), DC.FLOOR))
    assert 0 < d and rec / 2 <= d <= rec * 2, (d, rec)
    assert DC.bar() == max(4 * rec, DC.FLOOR)
    assert sorted(np.load(DC.GOLDEN)['cases'].tolist()) == sorted(DC.CASES)


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_f32_dx_close_to_float64_and_zero_under_the_mask(name):
    from xdet.ops import host_depthwise_backward
    c = DC.make_case(name)
    dx, dw = host_depthwise_backward(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'])
    (rdx, _), _ = DC.case_reference(name)
    assert dx.dtype == dw.dtype == f32
    assert np.abs(dx - rdx).max() <= 9 * 2.0 ** -23 * (np.abs(c['dy']).max() * np.abs(c['k']).max() * 9)
    if c['relu_in']:
        off = ~(c['x'] > 0)
        assert off.any() and not dx[off].any() and dx[~off].any()
    assert host_depthwise_backward(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'], with_dx=False)[0] is None


def test_mask_rule_zero_and_nan():
    """x > 0 is false for a zero and for a NaN: both give dx = 0 there and contribute nothing to dw"""
    from xdet.ops import host_depthwise_backward
    c = DC.make_case('ragged')
    x = c['x'].copy()
    pos = np.argwhere(x > 0)[:12]
    x[tuple(pos[:6].T)] = np.nan
    x[tuple(pos[6:].T)] = 0
    x0 = np.nan_to_num(x, nan=0.)
    for dtype in (f32, f64):
        got = host_depthwise_backward(x, c['k'], c['dy'], 1, True, dtype)
        want = host_depthwise_backward(x0, c['k'], c['dy'], 1, True, dtype)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert not got[0][tuple(pos.T)].any()


def test_no_bleed_across_images():
    from xdet.ops import host_depthwise_backward
    c = DC.make_case('two_images')
    assert c['dy'][0].any() and not c['dy'][1].any() and c['x'][1].any() and not c['x'][0].any()
    for dtype in (f32, f64):
        dx, dw = host_depthwise_backward(c['x'], c['k'], c['dy'], 1, False, dtype)
        assert dx[0].any() and not dx[1].any() and not dw.any()


@pytest.mark.parametrize('name', ['ragged', 'dilated', 'chunk_growth'])
def test_power_of_two_scaling_is_exact(name):
    from xdet.ops import host_depthwise_backward
    c = DC.make_case(name)
    s = f32(2.0 ** -20)
    a = host_depthwise_backward(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'])
    b = host_depthwise_backward(c['x'], c['k'], c['dy'] * s, c['dilation'], c['relu_in'])
    for u, v in zip(a, b):
        assert u.any() and np.array_equal((u * s).view(np.uint32), v.view(np.uint32))


def test_python_door_refuses_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import ops, runtime, train_ops

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops):
        monkeypatch.setattr(mod, 'to_device', no_gpu)
        monkeypatch.setattr(mod, 'DeviceBuffer', no_gpu)
    z = lambda *s: np.zeros(s, f32)
    for call in (lambda: xdet.depthwise_backward(z(1, 4, 4, 8), z(3, 3, 8, 1), z(1, 4, 4, 8), dilation=3),
                 lambda: xdet.depthwise_backward(z(1, 4, 4, 8), z(3, 3, 8, 1), z(1, 4, 4, 8), dilation=0),
                 lambda: xdet.depthwise_backward(z(1, 1, 1, 4097), z(3, 3, 4097, 1), z(1, 1, 1, 4097)),     # C above 4096
                 lambda: xdet.depthwise_backward(z(1, 4, 4, 8), z(3, 3, 7, 1), z(1, 4, 4, 8)),              # k's channels
                 lambda: xdet.depthwise_backward(z(1, 4, 4, 8), z(3, 3, 8, 2), z(1, 4, 4, 8)),              # a multiplier
                 lambda: xdet.depthwise_backward(z(1, 4, 4, 8), z(3, 3, 8, 1), z(1, 4, 5, 8)),              # dy's shape
                 lambda: xdet.depthwise_backward(z(4, 4, 8), z(3, 3, 8, 1), z(4, 4, 8)),                    # three dimensions
                 lambda: xdet.depthwise_backward(z(0, 4, 4, 8), z(3, 3, 8, 1), z(0, 4, 4, 8)),              # no pixels
                 lambda: xdet.add_rows_device(z(1, 4, 4, 8), z(1, 4, 4, 7)),
                 lambda: xdet.add_rows_device(z(1, 4, 4, 8), z(1, 4, 4, 8), out=z(1, 4, 4, 8))):            # out not on the device
        with pytest.raises(xdet.InvalidArgumentError):
            call()


def test_c_door_refuses_before_any_gpu_work():
    """every refusal of include/xdet.h, with pointers that are never dereferenced (the library loads without a GPU)"""
    from xdet._lib import lib
    l = lib()
    p = 4096
    base = dict(x=p, ld_x=64, k=p, dy=p, ld_dy=64, N=2, H=5, W=7, C=50, d=1, relu=1, dx=p, ld_dx=64, dw=p, ws=p)

    def call(**kw):
        v = dict(base, **kw)
        return l.xdet_depthwise_backward(v['x'], v['ld_x'], v['k'], v['dy'], v['ld_dy'], v['N'], v['H'], v['W'], v['C'], v['d'],
                                         v['relu'], v['dx'], v['ld_dx'], v['dw'], v['ws'], None)
    big_ld = 2 ** 31 // 70 + 1
    for kw in [dict(d=3), dict(d=0), dict(d=-1), dict(N=0), dict(H=0), dict(W=-1), dict(C=0),
               dict(C=4097, ld_x=4097, ld_dy=4097, ld_dx=4097), dict(N=2 ** 31 // (35 * 50) + 1), dict(N=2 ** 30, H=2 ** 30),
               dict(ld_x=big_ld), dict(ld_dy=big_ld), dict(ld_dx=big_ld), dict(ld_x=49), dict(ld_dy=49), dict(ld_dx=49),
               dict(x=None), dict(k=None), dict(dy=None), dict(dw=None), dict(ws=None)]:
        assert call(**kw) == -1, kw
        assert b'depthwise_backward' in l.xdet_last_error()
    size = l.xdet_depthwise_backward_workspace_bytes
    assert size(2, 5, 7, 50) > 0 and size(1, 1, 1, 1) > 0 and size(8, 30, 30, 1536) > 0 and size(1, 2 ** 31 // 4096 - 1, 1, 4096) > 0
    for args in ((0, 5, 7, 50), (2, 0, 7, 50), (2, 5, 0, 50), (2, 5, 7, 0), (2, 5, 7, 4097), (-1, 5, 7, 5),
                 (2 ** 31 // (35 * 50) + 1, 5, 7, 50), (2 ** 30, 2 ** 30, 4, 1)):
        assert size(*args) == 0, args

    add = dict(a=p, ld_a=64, b=p, ld_b=64, out=p, ld_out=64, M=70, C=50)

    def add_rows(**kw):
        v = dict(add, **kw)
        return l.xdet_add_rows(v['a'], v['ld_a'], v['b'], v['ld_b'], v['out'], v['ld_out'], v['M'], v['C'], None)
    for kw in [dict(M=0), dict(C=0), dict(M=-3), dict(ld_a=49), dict(ld_b=49), dict(ld_out=49), dict(ld_a=big_ld),
               dict(ld_b=big_ld), dict(ld_out=big_ld), dict(a=None), dict(b=None), dict(out=None),
               dict(M=1, C=2 ** 24 + 1, ld_a=2 ** 24 + 1, ld_b=2 ** 24 + 1, ld_out=2 ** 24 + 1)]:
        assert add_rows(**kw) == -1, kw
        assert b'add_rows' in l.xdet_last_error()


SIZES = [(1, 1, 1, 4), (2, 5, 7, 50), (1, 260, 260, 4), (8, 30, 30, 1536), (1, 2, 2, 4096), (1, 256, 256, 1), (3, 600, 600, 3)]


def test_workspace_size_is_the_layout_walk(tmp_path):
    """a stand-alone host program walks dwb_layout (csrc/depthwise_backward_layout.h) with a measuring and a carving WsWalk;
    the library's size entry point returns the same bytes, and the chunk rule is max(64, ceil(M / 1024)) pixels"""
    from xdet._lib import lib
    src = tmp_path / 'dwb_layout_check.cpp'
    src.write_text('#include "depthwise_backward_layout.h"\n#include <cstdio>\n#include <cstdlib>\n#include <vector>\n'
                   'using namespace xdet;\n'
                   'int main(int argc, char** argv) {\n'
                   '  for (int i = 1; i + 3 < argc; i += 4) {\n'
                   '    const int N = atoi(argv[i]), H = atoi(argv[i + 1]), W = atoi(argv[i + 2]), C = atoi(argv[i + 3]);\n'
                   '    const DwbSums p = dwb_sums(N, H, W);\n'
                   '    const size_t n = ws_measure(4, dwb_layout, p, C);\n'
                   '    std::vector<unsigned char> block(n);\n'
                   '    const DwbWorkspace w = ws_carve(block.data(), 4, dwb_layout, p, C);\n'
                   '    const bool ok = (unsigned char*)w.partial == block.data() &&\n'
                   '                    (unsigned char*)(w.partial + (size_t)p.n_chunks * DWB_TAPS * C) == block.data() + n;\n'
                   '    printf("%d %d %zu %d\\n", p.pixels_per_chunk, p.n_chunks, n, ok ? 1 : 0);\n'
                   '  }\n'
                   '  return 0;\n'
                   '}\n')
    exe = str(tmp_path / 'dwb_layout_check')
    subprocess.check_call([os.environ.get('CXX', 'c++'), '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'x-detector_amd', 'csrc'), str(src), '-o', exe])
    r = subprocess.run([exe] + [str(v) for s in SIZES for v in s], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(rows) == len(SIZES)
    for (N, H, W, C), (per, chunks, nbytes, ok) in zip(SIZES, rows):
        M = N * H * W
        want_per = max(64, -(-M // 1024))
        assert (per, chunks, ok) == (want_per, -(-M // want_per), 1), (N, H, W, C)
        assert chunks <= 1024 and nbytes == chunks * 9 * C * 4
        assert lib().xdet_depthwise_backward_workspace_bytes(N, H, W, C) == nbytes, (N, H, W, C)
    # `chunk_growth` is past the floor of the rule, every other case on it
    for name, (N, H, W, C, _, _) in DC.CASES.items():
        assert (max(64, -(-N * H * W // 1024)) > 64) == (name == 'chunk_growth'), name


def test_new_symbols_are_exported():
    import re
    from xdet import _lib
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    assert {'xdet_depthwise_backward', 'xdet_depthwise_backward_workspace_bytes', 'xdet_add_rows'} <= exported
    assert _lib.lib().xdet_depthwise_backward_workspace_bytes.restype is _lib.c_size_t


if __name__ == '__main__' and '--write' in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, 'x-detector_amd'))
    d = DC.f32_statement_distance()
    np.savez(DC.GOLDEN, f32_distance=np.float64(d), cases=np.array(sorted(DC.CASES)))
    print('wrote %s: %.3e' % (DC.GOLDEN, d))
