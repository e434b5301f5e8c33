"""host_dense_backward (xdet/train_ops.py), the NumPy statement of xdet_dense_backward: in float64 against central differences of
sum(c * act(x w + b)), the mask rule (exact zeros and NaN in y), dx skipped, padded rows with NaN behind the width, the
argument checks of the GPU door -- and the f32 statement's distance from the float64 one over the cases of
tests/dense_backward_cases.py, which tests/golden/dense_backward_f32_distance.npz records and the GPU bar is read from."""
import sys

import numpy as np
import pytest

import dense_backward_cases as DC

f64 = np.float64


def _layer(x, w, b, relu):
    z = x @ w + b
    return np.maximum(z, 0) if relu else z


@pytest.mark.parametrize('relu', [False, True])
def test_float64_statement_against_central_differences(relu):
    from xdet.ops import host_dense_backward
    rng = np.random.default_rng(5 + relu)
    M, K, J = 5, 7, 4
    x, w, b, c = rng.standard_normal((M, K)), rng.standard_normal((K, J)), rng.standard_normal(J), rng.standard_normal((M, J))
    z = x @ w + b
    b = b + np.where(np.abs(z) < 0.05, 0.2, 0.).max(0)          # keep every pre-activation away from the ReLU kink
    assert np.abs(x @ w + b).min() > 1e-3
    y = _layer(x, w, b, relu)
    dx, dw, db = host_dense_backward(x, w, c, y if relu else None, dtype=f64)
    loss = lambda x_, w_, b_: float((c * _layer(x_, w_, b_, relu)).sum())
    h = 1e-6
    for arr, grad in ((x, dx), (w, dw), (b, db)):
        num = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            p, m = arr.copy(), arr.copy()
            p[i] += h
            m[i] -= h
            a = [x, w, b]
            ap, am = list(a), list(a)
            k = [j for j, t in enumerate(a) if t is arr][0]
            ap[k], am[k] = p, m
            num[i] = (loss(*ap) - loss(*am)) / (2 * h)
        assert np.abs(num - grad).max() <= 1e-8 * max(1., np.abs(grad).max()), np.abs(num - grad).max()


def test_mask_rule_zero_and_nan():
    from xdet.ops import host_dense_backward
    x = np.array([[1., 2.], [3., 4.], [5., 6.]], np.float32)
    w = np.array([[1., -1.], [0.5, 2.]], np.float32)
    dy = np.array([[1., 10.], [2., 20.], [np.nan, 30.]], np.float32)
    y = np.array([[0., 1.], [np.nan, 2.], [-1., 3.]], np.float32)      # zero, NaN and a negative value mask; NaN in a masked dy is dropped
    for dtype in (np.float32, np.float64):
        dx, dw, db = host_dense_backward(x, w, dy, y, dtype=dtype)
        g = np.array([[0., 10.], [0., 20.], [0., 30.]])
        assert dx.dtype == dtype and np.array_equal(dx, g @ w.T.astype(f64)) and np.array_equal(dw, x.T.astype(f64) @ g)
        assert np.array_equal(db, [0., 60.])
    dx, dw, db = host_dense_backward(x[:2], w, dy[:2], None)
    assert np.array_equal(db, [3., 30.])                              # no y: no mask


def test_dx_skipped():
    from xdet.ops import host_dense_backward
    x, w, dy, y = DC.make_case('ragged')
    dx, dw, db = host_dense_backward(x, w, dy, y, with_dx=False)
    full = host_dense_backward(x, w, dy, y)
    assert dx is None and np.array_equal(dw, full[1]) and np.array_equal(db, full[2]) and full[0].shape == x.shape


def test_wider_rows_with_nan_padding():
    """views of padded buffers (ld above the width, NaN behind it) give what the dense matrices give"""
    from xdet.ops import host_dense_backward
    x, w, dy, y = DC.make_case('ragged')

    def padded(a, extra):
        p = np.full((a.shape[0], a.shape[1] + extra), np.nan, np.float32)
        p[:, :a.shape[1]] = a
        return p[:, :a.shape[1]]
    a = host_dense_backward(padded(x, 14), w, padded(dy, 7), padded(y, 3))
    b = host_dense_backward(x, w, dy, y)
    for u, v in zip(a, b):
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
    for call in (lambda: ops.dense_backward(z(4, 3), z(2, 5), z(4, 5)),            # w's rows are not x's columns
                 lambda: ops.dense_backward(z(4, 3), z(3, 5), z(3, 5)),            # dy's rows
                 lambda: ops.dense_backward(z(4, 3), z(3, 5), z(4, 5), z(4, 4)),   # y's width
                 lambda: ops.dense_backward(z(4, 3, 1), z(3, 5), z(4, 5)),         # not a matrix
                 lambda: ops.dense_backward(z(0, 3), z(3, 5), z(0, 5)),            # no rows
                 lambda: ops.dense_backward(z(1, 4097), z(4097, 1), z(1, 1))):     # K above 4096
        with pytest.raises(xdet.InvalidArgumentError):
            call()


def test_c_door_refuses_before_any_gpu_work():
    """every refusal of include/xdet.h, with pointers that are never dereferenced"""
    from xdet._lib import lib
    l = lib()
    p = 4096
    ok = dict(x=p, ld_x=50, w=p, y=p, ld_y=25, dy=p, ld_dy=25, M=70, K=50, J=25, dx=p, ld_dx=50, dw=p, db=p, ws=p)

    def call(**kw):
        v = dict(ok, **kw)
        return l.xdet_dense_backward(v['x'], v['ld_x'], v['w'], v['y'], v['ld_y'], v['dy'], v['ld_dy'], v['M'], v['K'], v['J'],
                                     v['dx'], v['ld_dx'], v['dw'], v['db'], v['ws'], None)
    bad = [dict(M=0), dict(K=0), dict(J=-1), dict(K=4097, ld_x=4097, ld_dx=4097), dict(J=4097, ld_dy=4097, ld_y=4097),
           dict(M=2 ** 31 // 50 + 1), dict(ld_x=49), dict(ld_dy=24), dict(ld_y=24), dict(ld_dx=49), dict(x=None), dict(w=None),
           dict(dy=None), dict(dw=None), dict(db=None), dict(ws=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b'dense_backward' in l.xdet_last_error()
    assert l.xdet_dense_backward_workspace_bytes(70, 50, 25) > 0
    for m, k, j in ((0, 50, 25), (70, 0, 25), (70, 50, 0), (70, 4097, 25), (2 ** 31 // 50 + 1, 50, 25)):
        assert l.xdet_dense_backward_workspace_bytes(m, k, j) == 0
    # dW's slabs: 129 rows of a single 16 x 16 tile are two ranges, 128 rows one (which writes dW itself)
    one, two = l.xdet_dense_backward_workspace_bytes(128, 16, 16), l.xdet_dense_backward_workspace_bytes(129, 16, 16)
    assert two - one == 2 * 16 * 16 * 4 + 16 * 4, (one, two)


def test_f32_statement_distance_is_the_recorded_one():
    """BLAS builds order their sums differently: the recorded figure must be of the size measured here (within 2x either
    way), so the GPU bar read from the file is the bar this module would compute"""
    d = DC.f32_statement_distance()
    rec = float(np.load(DC.GOLDEN)['f32_distance'])
    print('f32 statement vs float64: measured %.3e, recorded %.3e -> GPU bar %.3e (floor %.3e)' % (d, rec, DC.bar(), DC.FLOOR))
    assert 0 < d and rec / 2 <= d <= rec * 2, (d, rec)
    assert DC.bar() == max(4 * rec, DC.FLOOR)


if __name__ == '__main__' and '--write' in sys.argv:
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'x-detector_amd'))
    d = DC.f32_statement_distance()
    np.savez(DC.GOLDEN, f32_distance=np.float64(d), cases=np.array(sorted(DC.CASES)))
    print('wrote %s: %.3e' % (DC.GOLDEN, d))
