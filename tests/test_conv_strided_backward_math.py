"""host_conv_backward_strided (xdet/train_ops.py), the NumPy statement of xdet_conv_backward_strided: in float64 against
torch.autograd of torch.nn.functional.conv2d on every case of tests/conv_strided_backward_cases.py ('SAME' as an explicit F.pad
with TensorFlow's front / back split), stride 1 'SAME' against host_conv_backward bit for bit, 1 x 1 at stride 2 against
host_subsample2 / host_add_upsample2 around the 1 x 1 backward, exact zeros under no window, the refusals of the Python doors and
of the C door -- and the f32 statement's distance from the float64 one, which
tests/golden/conv_strided_backward_f32_distance.npz records (with the f32 stem chain's, tests/test_gpu_stem_chain.py) and the GPU
bars are read from."""
import sys

import numpy as np
import pytest

import conv_backward_cases as CC
import conv_strided_backward_cases as CS

f64 = np.float64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _torch_backward(x, w, dy, y, relu_in, stride, padding):
    """d sum(g * conv(xe, w)) / d (x, w) and sum g by torch.autograd in float64 on the CPU, the mask taken from y itself"""
    import torch
    import torch.nn.functional as F
    N, H, W, C = x.shape
    kh, kw = w.shape[:2]
    Ho, Wo, pt, pl = CS.geometry(H, W, kh, kw, stride, padding)[:4]
    pb, pr = max((Ho - 1) * stride + kh - H - pt, 0), max((Wo - 1) * stride + kw - W - pl, 0)
    tx = torch.tensor(np.asarray(x, f64).transpose(0, 3, 1, 2), requires_grad=True)
    tw = torch.tensor(np.asarray(w, f64).transpose(3, 2, 0, 1), requires_grad=True)       # HWIO -> OIHW
    tb = torch.zeros(w.shape[3], dtype=torch.float64, requires_grad=True)
    z = F.conv2d(F.pad(torch.relu(tx) if relu_in else tx, (pl, pr, pt, pb)), tw, tb, stride=stride)
    assert tuple(z.shape[2:]) == (Ho, Wo)
    g = torch.tensor(np.asarray(dy, f64).transpose(0, 3, 1, 2))
    if y is not None:
        g = g * torch.tensor((np.asarray(y) > 0).transpose(0, 3, 1, 2).astype(f64))
    (z * g).sum().backward()
    return (tx.grad.numpy().transpose(0, 2, 3, 1), tw.grad.numpy().transpose(2, 3, 1, 0), tb.grad.numpy())


@pytest.mark.parametrize('name', sorted(CS.CASES))
def test_float64_statement_against_torch_autograd(name):
    x, w, dy, y, relu_in, stride, padding = CS.make_case(name)
    ref, den = CS.case_reference(name)
    d = CS.distances(_torch_backward(x, w, dy, y, relu_in, stride, padding), ref, den)
    assert ref[0].shape == x.shape and ref[1].shape == w.shape and ref[2].shape == (w.shape[3],)
    assert max(d) <= 1e-12, (name, d)


def test_same_padding_is_tensorflows():
    """the smaller half in front: 8 rows at stride 2 pad 0 / 1, 7 rows 1 / 1; 'VALID' leaves the last row of an even map out"""
    assert CS.geometry(8, 6, 3, 3, 2, 'SAME') == (4, 3, 0, 0, 8, 6)
    assert CS.geometry(7, 9, 3, 3, 2, 'SAME') == (4, 5, 1, 1, 7, 9)
    assert CS.geometry(10, 8, 3, 3, 2, 'VALID') == (4, 3, 0, 0, 9, 7)
    assert CS.geometry(9, 11, 3, 3, 2, 'VALID') == (4, 5, 0, 0, 9, 11)
    from xdet.train_ops import _strided_geometry
    for H, W, kh, kw, s, p in ((8, 6, 3, 3, 2, 'SAME'), (7, 9, 3, 3, 2, 'SAME'), (10, 8, 3, 3, 2, 'VALID'), (13, 13, 7, 7, 2, 'VALID'),
                               (5, 7, 3, 3, 1, 'SAME'), (5, 5, 1, 1, 2, 'SAME')):
        assert _strided_geometry(H, W, kh, kw, s, p) == CS.geometry(H, W, kh, kw, s, p)[:4]


@pytest.mark.parametrize('name', sorted(CS.SAME_S1_IS_OLD))
@pytest.mark.parametrize('dtype', [np.float32, f64])
def test_same_s1_is_old(name, dtype):
    """stride 1 'SAME' is host_conv_backward (which is this statement at that geometry), bit for bit, with and without dx"""
    from xdet.ops import host_conv_backward, host_conv_backward_strided
    x, w, dy, y, relu_in, stride, padding = CS.make_case(name)
    assert (stride, padding) == (1, 'SAME')
    old = host_conv_backward(*CC.make_case(CS.SAME_S1_IS_OLD[name]), dtype=dtype)
    for new in (host_conv_backward_strided(x, w, dy, y, relu_in, dtype=dtype),                       # the defaults
                host_conv_backward_strided(x, w, dy, y, relu_in, dtype=dtype, stride=1, padding='SAME')):
        for u, v in zip(new, old):
            assert u.dtype == dtype and np.array_equal(bits(u), bits(v))
    no_dx = host_conv_backward_strided(x, w, dy, y, relu_in, dtype=dtype, with_dx=False)
    assert no_dx[0] is None and np.array_equal(bits(no_dx[1]), bits(old[1])) and np.array_equal(bits(no_dx[2]), bits(old[2]))


def test_pointwise_s2_is_subsample_dense_upsample():
    """1 x 1 at stride 2 'SAME': the 1 x 1 backward on host_subsample2(x), its dx spread by host_add_upsample2 over zeros"""
    from xdet.ops import host_conv_backward, host_conv_backward_strided, host_subsample2, host_add_upsample2
    x, w, dy, y, relu_in, stride, padding = CS.make_case('pointwise_s2')
    for dtype in (np.float32, f64):
        got = host_conv_backward_strided(x, w, dy, y, relu_in, dtype=dtype, stride=stride, padding=padding)
        dxs, dw, db = host_conv_backward(host_subsample2(x, dtype), w, dy, y, relu_in, dtype=dtype)
        assert np.array_equal(got[0], host_add_upsample2(np.zeros(x.shape, dtype), dxs, dtype))
        assert np.array_equal(got[1], dw) and np.array_equal(got[2], db)
        assert not got[0][:, 1::2].any() and not got[0][:, :, 1::2].any() and got[0][:, ::2, ::2].all()


@pytest.mark.parametrize('name', ['stem1_even', 'ranges'])
def test_pixels_under_no_window_get_exact_zeros_and_are_not_used(name):
    from xdet.ops import host_conv_backward_strided
    x, w, dy, y, relu_in, stride, padding = CS.make_case(name)
    N, H, W, C = x.shape
    Hc, Wc = CS.geometry(H, W, w.shape[0], w.shape[1], stride, padding)[4:]
    assert Hc < H or Wc < W
    clean = host_conv_backward_strided(x, w, dy, y, relu_in, stride=stride, padding=padding)
    assert not clean[0][:, Hc:].any() and not clean[0][:, :, Wc:].any() and clean[0][:, :Hc, :Wc].any()
    assert not np.signbit(clean[0][:, Hc:]).any() and not np.signbit(clean[0][:, :, Wc:]).any()
    dirty = np.array(x)
    dirty[:, Hc:], dirty[:, :, Wc:] = np.nan, np.nan
    for ri in (False, True):
        a = host_conv_backward_strided(x, w, dy, y, ri, stride=stride, padding=padding)
        b = host_conv_backward_strided(dirty, w, dy, y, ri, stride=stride, padding=padding)
        for u, v in zip(a, b):
            assert np.isfinite(v).all() and np.array_equal(bits(u), bits(v))


def test_dx_skipped():
    from xdet.ops import host_conv_backward_strided
    x, w, dy, y, relu_in, stride, padding = CS.make_case('same_s2_odd')
    full = host_conv_backward_strided(x, w, dy, y, relu_in, stride=stride, padding=padding)
    dx, dw, db = host_conv_backward_strided(x, w, dy, y, relu_in, with_dx=False, stride=stride, padding=padding)
    assert dx is None and np.array_equal(dw, full[1]) and np.array_equal(db, full[2])
    assert (np.asarray(x) <= 0).any() and not full[0][np.asarray(x) <= 0].any()         # relu_in


def test_python_doors_refuse_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import ops, runtime, train_ops

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops):
        monkeypatch.setattr(mod, 'to_device', no_gpu)
        monkeypatch.setattr(mod, 'DeviceBuffer', no_gpu)
    z = lambda *s: np.zeros(s, np.float32)
    door = xdet.conv_backward_strided
    calls = {
        'x is not NHWC': lambda: door(z(16, 3), z(3, 3, 3, 5), z(1, 4, 4, 5)),
        'w has three dimensions': lambda: door(z(1, 4, 4, 3), z(3, 3, 15), z(1, 4, 4, 5)),
        'dy has three dimensions': lambda: door(z(1, 4, 4, 3), z(3, 3, 3, 5), z(4, 4, 5)),
        'y has three dimensions': lambda: door(z(1, 4, 4, 3), z(3, 3, 3, 5), z(1, 4, 4, 5), z(4, 4, 5)),
        "w's C is not x's": lambda: door(z(1, 4, 4, 3), z(3, 3, 2, 5), z(1, 4, 4, 5)),
        'dy is the input map at stride 2': lambda: door(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 9, 9, 5), stride=2, padding='VALID'),
        "dy is 'SAME''s map under 'VALID'": lambda: door(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 5, 5, 5), stride=2, padding='VALID'),
        "y's channels": lambda: door(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 4, 4, 5), z(1, 4, 4, 4), stride=2, padding='VALID'),
        "y's pixels": lambda: door(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 4, 4, 5), z(1, 5, 5, 5), stride=2, padding='VALID'),
        'stride 3': lambda: door(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 3, 3, 5), stride=3),
        'stride 0': lambda: door(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 9, 9, 5), stride=0),
        "padding 'EXPLICIT'": lambda: door(z(1, 4, 4, 3), z(3, 3, 3, 5), z(1, 4, 4, 5), padding='EXPLICIT'),
        'padding as a number': lambda: door(z(1, 4, 4, 3), z(3, 3, 3, 5), z(1, 4, 4, 5), padding=1),
        'even kh': lambda: door(z(1, 4, 4, 3), z(2, 3, 3, 5), z(1, 4, 4, 5)),
        'kw above 15': lambda: door(z(1, 4, 4, 3), z(3, 17, 3, 5), z(1, 4, 4, 5)),
        "a 'VALID' kernel larger than the map": lambda: door(z(1, 4, 2, 3), z(3, 3, 3, 5), z(1, 2, 1, 5), padding='VALID'),
        'no pixels': lambda: door(z(0, 4, 4, 3), z(3, 3, 3, 5), z(0, 4, 4, 5)),
        'C above 4096': lambda: door(z(1, 1, 1, 4097), z(1, 1, 4097, 1), z(1, 1, 1, 1)),
    }
    for what, call in calls.items():
        with pytest.raises(xdet.InvalidArgumentError) as e:
            call()
        assert str(e.value).startswith('xdet error -1: conv_backward_strided: '), (what, str(e.value))
    with pytest.raises(xdet.InvalidArgumentError) as e:
        door(z(1, 9, 11, 3), z(3, 3, 3, 5), z(1, 9, 11, 5), stride=2, padding='VALID')
    assert 'Ho = 4' in str(e.value) and 'Wo = 5' in str(e.value)                 # the message names the expected map
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.conv_backward_strided_device(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 9, 9, 5), stride=2)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.host_conv_backward_strided(z(1, 9, 9, 3), z(3, 3, 3, 5), z(1, 9, 9, 5), stride=2)


def c_call(l, ok, **kw):
    v = dict(ok, **kw)
    return l.xdet_conv_backward_strided(v['x'], v['ld_x'], v['w'], v['y'], v['ld_y'], v['dy'], v['ld_dy'], v['N'], v['H'], v['W'],
                                        v['C'], v['J'], v['kh'], v['kw'], v['stride'], v['padding'], v['relu_in'], v['dx'],
                                        v['ld_dx'], v['dw'], v['db'], v['ws'], None)


def test_c_door_refuses_before_any_gpu_work():
    """every refusal of include/xdet.h, with pointers that are never dereferenced (the library loads without a GPU)"""
    from xdet._lib import lib
    l = lib()
    p = 4096
    ok = dict(x=p, ld_x=50, w=p, y=p, ld_y=25, dy=p, ld_dy=25, N=2, H=5, W=7, C=50, J=25, kh=3, kw=3, stride=2, padding=0,
              relu_in=1, dx=p, ld_dx=50, dw=p, db=p, ws=p)
    big_n = 2 ** 31 // (35 * 50) + 1
    bad = [dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(J=0), dict(kh=0), dict(kw=-3), dict(kh=2), dict(kw=4), dict(kh=17),
           dict(kw=17), dict(C=4097, ld_x=4097, ld_dx=4097), dict(J=4097, ld_dy=4097, ld_y=4097), dict(N=big_n),
           dict(ld_x=2 ** 31 // 70 + 1), dict(ld_dy=2 ** 31 // 12 + 1), dict(ld_x=49), dict(ld_dy=24), dict(ld_y=24), dict(ld_dx=49),
           dict(x=None), dict(w=None), dict(dy=None), dict(dw=None), dict(db=None), dict(ws=None),
           dict(stride=0), dict(stride=3), dict(stride=-1), dict(padding=2), dict(padding=-1),
           dict(H=2), dict(W=2), dict(kh=7), dict(kh=5, kw=9)]              # 'VALID': Ho < 1 or Wo < 1
    for kw in bad:
        assert c_call(l, ok, **kw) == -1, kw
        assert b'conv_backward_strided' in l.xdet_last_error()
    size = l.xdet_conv_backward_strided_workspace_bytes
    assert size(2, 5, 7, 50, 25, 3, 3, 2, 0) > 0 and size(1, 1, 1, 1, 1, 15, 15, 1, 1) > 0 and size(8, 480, 480, 3, 32, 3, 3, 2, 0) > 0
    for args in ((0, 5, 7, 50, 25, 3, 3, 1, 1), (2, 0, 7, 50, 25, 3, 3, 1, 1), (2, 5, 7, 0, 25, 3, 3, 1, 1), (2, 5, 7, 50, 0, 3, 3, 1, 1),
                 (2, 5, 7, 50, 25, 2, 3, 1, 1), (2, 5, 7, 50, 25, 3, 17, 1, 1), (2, 5, 7, 4097, 25, 3, 3, 1, 1),
                 (big_n, 5, 7, 50, 25, 3, 3, 1, 1), (2, 5, 7, 50, 25, 3, 3, 3, 1), (2, 5, 7, 50, 25, 3, 3, 0, 1),
                 (2, 5, 7, 50, 25, 3, 3, 1, 2), (2, 5, 7, 50, 25, 7, 3, 1, 0), (2, 5, 7, 50, 25, 3, 9, 2, 0)):
        assert size(*args) == 0, args
    # stride 1 'SAME' needs xdet_conv_backward's workspace; the sums are sized by the OUTPUT map: 'ranges' has four dW ranges
    old = l.xdet_conv_backward_workspace_bytes
    assert size(3, 7, 7, 16, 16, 3, 3, 1, 1) == old(3, 7, 7, 16, 16, 3, 3)
    N, H, W, C, J, kh, kw, s, _ = CS.CASES['ranges'][:9]
    per, n = CS.dw_ranges(N * 8 * 12, kh * kw * C, J)
    assert (per, n) == (128, 4)
    chunks = -(-N * 8 * 12 // 64)
    assert size(N, H, W, C, J, kh, kw, s, 0) == 16 * 4 + chunks * J * 4 + n * kh * kw * C * J * 4


def test_new_symbols_are_exported():
    import re
    import subprocess
    from xdet import _lib
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    assert {'xdet_conv_backward_strided', 'xdet_conv_backward_strided_workspace_bytes'} <= exported
    assert _lib.lib().xdet_conv_backward_strided_workspace_bytes.restype is _lib.c_size_t


def test_f32_distances_are_the_recorded_ones():
    """BLAS builds order their sums differently: each recorded figure must be of the size measured here (within 2x either
    way), so the GPU bars read from the file are the bars this module would compute"""
    import test_gpu_stem_chain as chain
    rec = np.load(CS.GOLDEN)
    for what, d, r in (('statement', CS.f32_statement_distance(), float(rec['f32_distance'])),
                       ('stem chain', chain.f32_chain_distance(), float(rec['stem_chain_f32_distance']))):
        print('f32 %s vs float64: measured %.3e, recorded %.3e' % (what, d, r))
        assert 0 < d and r / 2 <= d <= r * 2, (what, d, r)
    assert CS.bar() == max(4 * float(rec['f32_distance']), CS.FLOOR) and CS.chain_bar() == 4 * float(rec['stem_chain_f32_distance'])
    assert sorted(rec['cases'].tolist()) == sorted(CS.CASES)


if __name__ == '__main__' and '--write' in sys.argv:
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'x-detector_amd'))
    import test_gpu_stem_chain as chain
    d, c = CS.f32_statement_distance(), chain.f32_chain_distance()
    np.savez(CS.GOLDEN, f32_distance=np.float64(d), stem_chain_f32_distance=np.float64(c), cases=np.array(sorted(CS.CASES)))
    print('wrote %s: statement %.3e, stem chain %.3e' % (CS.GOLDEN, d, c))
