"""host_conv_backward (xdet/train_ops.py), the NumPy statement of xdet_conv_backward: in float64 against torch.autograd of
torch.nn.functional.conv2d on every case of tests/conv_backward_cases.py (both ReLU masks included), the adjoint identities,
1 x 1 against host_dense_backward, the mask rule for NaN in y and x, the argument checks of the C door -- and the f32
statement's distance from the float64 one, which tests/golden/conv_backward_f32_distance.npz records and the GPU bar is read
from."""
import sys

import numpy as np
import pytest

import conv_backward_cases as CC

f64 = np.float64


def _torch_backward(x, w, dy, y, relu_in):
    """d sum(dy * act(conv(xe, w) + b)) / d (x, w, b) by torch.autograd in float64 on the CPU; the bias is the one that
    reproduces y's zero pattern exactly: the mask is taken from y itself"""
    import torch
    import torch.nn.functional as F
    tx = torch.tensor(np.asarray(x, f64).transpose(0, 3, 1, 2), requires_grad=True)
    tw = torch.tensor(np.asarray(w, f64).transpose(3, 2, 0, 1), requires_grad=True)       # HWIO -> OIHW
    tb = torch.zeros(w.shape[3], dtype=torch.float64, requires_grad=True)
    kh, kw = w.shape[:2]
    z = F.conv2d(torch.relu(tx) if relu_in else tx, tw, tb, stride=1, padding=(kh // 2, kw // 2))
    g = torch.tensor(np.asarray(dy, f64).transpose(0, 3, 1, 2))
    if y is not None:
        g = g * torch.tensor((np.asarray(y) > 0).transpose(0, 3, 1, 2).astype(f64))      # d relu: 1 where y > 0
    (z * g).sum().backward()
    return (tx.grad.numpy().transpose(0, 2, 3, 1), tw.grad.numpy().transpose(2, 3, 1, 0), tb.grad.numpy())


@pytest.mark.parametrize('name', sorted(CC.CASES))
def test_float64_statement_against_torch_autograd(name):
    x, w, dy, y, relu_in = CC.make_case(name)
    ref, den = CC.case_reference(name)
    got = _torch_backward(x, w, dy, y, relu_in)
    d = CC.distances(got, ref, den)
    assert ref[0].shape == x.shape and ref[1].shape == w.shape and ref[2].shape == (w.shape[3],)
    assert max(d) <= 1e-12, (name, d)


def test_relu_masks_through_torch_relu():
    """the ReLU behind the conv taken by autograd itself (not from y), on a case whose pre-activations keep off the kink"""
    import torch
    import torch.nn.functional as F
    from xdet.ops import host_conv_backward
    rng = np.random.default_rng(3)
    x, w, b = rng.standard_normal((2, 4, 5, 3)), rng.standard_normal((3, 3, 3, 4)) / 5, rng.standard_normal(4)
    dy = rng.standard_normal((2, 4, 5, 4))
    z = CC.conv_forward64(x, w, True) + b
    assert np.abs(z).min() > 1e-6
    y = np.maximum(z, 0)
    tx = torch.tensor(x.transpose(0, 3, 1, 2), requires_grad=True)
    tw = torch.tensor(w.transpose(3, 2, 0, 1), requires_grad=True)
    tb = torch.tensor(b, requires_grad=True)
    out = torch.relu(F.conv2d(torch.relu(tx), tw, tb, padding=1))
    (out * torch.tensor(dy.transpose(0, 3, 1, 2))).sum().backward()
    dx, dw, db = host_conv_backward(x, w, dy, y, True, dtype=f64)
    assert np.abs(dx - tx.grad.numpy().transpose(0, 2, 3, 1)).max() <= 1e-12
    assert np.abs(dw - tw.grad.numpy().transpose(2, 3, 1, 0)).max() <= 1e-12
    assert np.abs(db - tb.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize('name', sorted(CC.CASES))
def test_adjoint_identities(name):
    """<conv(xe, W), g> = <xe, dx without the input mask> = <W, dw> in float64"""
    from xdet.ops import host_conv_backward
    x, w, dy, y, relu_in = CC.make_case(name)
    xe = np.maximum(np.asarray(x, f64), 0) if relu_in else np.asarray(x, f64)
    g = np.asarray(dy, f64) if y is None else np.where(np.asarray(y) > 0, np.asarray(dy, f64), 0.)
    dx, dw, _ = host_conv_backward(xe, w, g, None, False, dtype=f64)
    lhs = float((CC.conv_forward64(xe, w, False) * g).sum())
    scale = float((np.abs(CC.conv_forward64(np.abs(xe), np.abs(w), False)) * np.abs(g)).sum())
    assert abs(lhs - float((xe * dx).sum())) <= 1e-12 * scale
    assert abs(lhs - float((np.asarray(w, f64) * dw).sum())) <= 1e-12 * scale
    # the statement with its masks gives the same dw, and its dx is the unmasked one where x > 0
    mdx, mdw, _ = host_conv_backward(x, w, dy, y, relu_in, dtype=f64)
    assert np.array_equal(mdw, dw) and np.array_equal(mdx, np.where(np.asarray(x) > 0, dx, 0.) if relu_in else dx)


def test_pointwise_is_the_dense_layer():
    from xdet.ops import host_conv_backward, host_dense_backward
    x, w, dy, y, relu_in = CC.make_case('pointwise')
    C, J = w.shape[2:]
    a = host_conv_backward(x, w, dy, y, relu_in, dtype=f64)
    b = host_dense_backward(x.reshape(-1, C), w.reshape(C, J), dy.reshape(-1, J), y.reshape(-1, J), dtype=f64)
    _, den = CC.case_reference('pointwise')
    assert max(CC.distances((a[0].reshape(-1, C), a[1].reshape(C, J), a[2]), b, den)) <= 1e-12


def test_mask_rule_zero_and_nan():
    """a NaN in y masks the gradient there; with relu_in a NaN in x counts as 0 in dw and gets the gradient 0"""
    from xdet.ops import host_conv_backward
    rng = np.random.default_rng(9)
    x, w, dy = rng.standard_normal((1, 3, 3, 2)), rng.standard_normal((3, 3, 2, 2)), rng.standard_normal((1, 3, 3, 2))
    y = np.abs(rng.standard_normal((1, 3, 3, 2)))
    y[0, 1, 1, 0], y[0, 0, 2, 1], x[0, 2, 0, 1] = np.nan, 0., np.nan
    dy_nan = dy.copy()
    dy_nan[0, 1, 1, 0] = np.nan                                          # a NaN in a masked dy is dropped
    for dtype in (np.float32, f64):
        got = host_conv_backward(x, w, dy_nan, y, True, dtype=dtype)
        y0, x0, dy0 = np.nan_to_num(y, nan=0.), np.nan_to_num(x, nan=0.), dy.copy()
        dy0[0, 1, 1, 0] = 0
        want = host_conv_backward(x0, w, dy0, y0, True, dtype=dtype)
        for u, v in zip(got, want):
            assert u.dtype == dtype and np.isfinite(u).all() and np.array_equal(u, v)
        assert got[0][0, 2, 0, 1] == 0
    assert np.isnan(host_conv_backward(x, w, dy, None, False)[1]).any()   # no relu_in: the NaN in x is an input like any other


def test_dx_skipped_and_padded_views():
    from xdet.ops import host_conv_backward
    x, w, dy, y, relu_in = CC.make_case('ragged_3x3')
    full = host_conv_backward(x, w, dy, y, relu_in)
    dx, dw, db = host_conv_backward(x, w, dy, y, relu_in, with_dx=False)
    assert dx is None and np.array_equal(dw, full[1]) and np.array_equal(db, full[2])

    def padded(a, extra):
        p = np.full(a.shape[:3] + (a.shape[3] + extra,), np.nan, np.float32)
        p[..., :a.shape[3]] = a
        return p[..., :a.shape[3]]
    for u, v in zip(host_conv_backward(padded(x, 14), w, padded(dy, 7), padded(y, 3), relu_in), full):
        assert np.isfinite(u).all() and np.array_equal(u, v)


def test_python_door_refuses_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import ops, runtime, train_ops

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops):
        monkeypatch.setattr(mod, 'to_device', no_gpu)
        monkeypatch.setattr(mod, 'DeviceBuffer', no_gpu)
    z = lambda *s: np.zeros(s, np.float32)
    for call in (lambda: xdet.conv_backward(z(1, 4, 4, 3), z(3, 3, 2, 5), z(1, 4, 4, 5)),             # w's C is not x's
                 lambda: xdet.conv_backward(z(1, 4, 4, 3), z(3, 3, 3, 5), z(1, 4, 3, 5)),             # dy's pixels
                 lambda: xdet.conv_backward(z(1, 4, 4, 3), z(3, 3, 3, 5), z(1, 4, 4, 5), z(1, 4, 4, 4)),   # y's channels
                 lambda: xdet.conv_backward(z(16, 3), z(3, 3, 3, 5), z(1, 4, 4, 5)),                  # not NHWC
                 lambda: xdet.conv_backward(z(1, 4, 4, 3), z(2, 3, 3, 5), z(1, 4, 4, 5)),             # even kh
                 lambda: xdet.conv_backward(z(1, 4, 4, 3), z(3, 17, 3, 5), z(1, 4, 4, 5)),            # kw above 15
                 lambda: xdet.conv_backward(z(0, 4, 4, 3), z(3, 3, 3, 5), z(0, 4, 4, 5)),             # no pixels
                 lambda: xdet.conv_backward(z(1, 1, 1, 4097), z(1, 1, 4097, 1), z(1, 1, 1, 1))):      # C above 4096
        with pytest.raises(xdet.InvalidArgumentError):
            call()


def test_c_door_refuses_before_any_gpu_work():
    """every refusal of include/xdet.h, with pointers that are never dereferenced (the library loads without a GPU)"""
    from xdet._lib import lib
    l = lib()
    p = 4096
    ok = dict(x=p, ld_x=50, w=p, y=p, ld_y=25, dy=p, ld_dy=25, N=2, H=5, W=7, C=50, J=25, kh=3, kw=3, relu_in=1, dx=p, ld_dx=50,
              dw=p, db=p, ws=p)

    def call(**kw):
        v = dict(ok, **kw)
        return l.xdet_conv_backward(v['x'], v['ld_x'], v['w'], v['y'], v['ld_y'], v['dy'], v['ld_dy'], v['N'], v['H'], v['W'],
                                    v['C'], v['J'], v['kh'], v['kw'], v['relu_in'], v['dx'], v['ld_dx'], v['dw'], v['db'], v['ws'],
                                    None)
    big_n = 2 ** 31 // (35 * 50) + 1
    bad = [dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(J=0), dict(kh=0), dict(kw=-3), dict(kh=2), dict(kw=4), dict(kh=17),
           dict(kw=17), dict(C=4097, ld_x=4097, ld_dx=4097), dict(J=4097, ld_dy=4097, ld_y=4097), dict(N=big_n),
           dict(ld_x=2 ** 31 // 70 + 1), dict(ld_dy=2 ** 31 // 70 + 1), dict(ld_x=49), dict(ld_dy=24), dict(ld_y=24), dict(ld_dx=49),
           dict(x=None), dict(w=None), dict(dy=None), dict(dw=None), dict(db=None), dict(ws=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b'conv_backward' in l.xdet_last_error()
    size = l.xdet_conv_backward_workspace_bytes
    assert size(2, 5, 7, 50, 25, 3, 3) > 0 and size(1, 1, 1, 1, 1, 15, 15) > 0 and size(8, 30, 30, 728, 512, 3, 3) > 0
    for args in ((0, 5, 7, 50, 25, 3, 3), (2, 0, 7, 50, 25, 3, 3), (2, 5, 7, 0, 25, 3, 3), (2, 5, 7, 50, 0, 3, 3),
                 (2, 5, 7, 50, 25, 2, 3), (2, 5, 7, 50, 25, 3, 17), (2, 5, 7, 4097, 25, 3, 3), (big_n, 5, 7, 50, 25, 3, 3)):
        assert size(*args) == 0, args
    # dW's slabs: 147 pixels of two 128-row tiles (9 taps x 16 channels) are two ranges, 128 pixels one (which writes dW
    # itself); db's chunks of 64 pixels are three against two
    one, two = size(2, 8, 8, 16, 16, 3, 3), size(3, 7, 7, 16, 16, 3, 3)
    assert two - one == 2 * 144 * 16 * 4 + 16 * 4, (one, two)


def test_new_symbols_are_exported():
    import re
    import subprocess
    from xdet import _lib
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    assert {'xdet_conv_backward', 'xdet_conv_backward_workspace_bytes'} <= exported
    assert _lib.lib().xdet_conv_backward_workspace_bytes.restype is _lib.c_size_t


def test_f32_statement_distance_is_the_recorded_one():
    """BLAS builds order their sums differently: the recorded figure must be of the size measured here (within 2x either
    way), so the GPU bar read from the file is the bar this module would compute"""
    d = CC.f32_statement_distance()
    rec = float(np.load(CC.GOLDEN)['f32_distance'])
    print('f32 statement vs float64: measured %.3e, recorded %.3e -> GPU bar %.3e (floor %.3e)' % (d, rec, CC.bar(), CC.FLOOR))
    assert 0 < d and rec / 2 <= d <= rec * 2, (d, rec)
    assert CC.bar() == max(4 * rec, CC.FLOOR)
    assert sorted(np.load(CC.GOLDEN)['cases'].tolist()) == sorted(CC.CASES)


if __name__ == '__main__' and '--write' in sys.argv:
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'x-detector_amd'))
    d = CC.f32_statement_distance()
    np.savez(CC.GOLDEN, f32_distance=np.float64(d), cases=np.array(sorted(CC.CASES)))
    print('wrote %s: %.3e' % (CC.GOLDEN, d))
