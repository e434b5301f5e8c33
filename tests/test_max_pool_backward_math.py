"""ops.host_max_pool_backward, host_subsample2 and host_add_upsample2 (xdet/train_ops.py), the NumPy statements of
xdet_maxpool3x3s2_backward, xdet_subsample2 and xdet_add_upsample2: in float64 against torch.autograd, exactly
(np.array_equal) -- a max pool's gradient only moves and adds values of dy, and the adds of at most four shares happen in the
same order on both sides, or in any order where a pixel gets at most two.  The tie rule is the point: the first maximum in
row-major window order takes the share (torch's CPU max_pool2d on the -inf-padded input; integer-valued maps make every window
tie).  And the refusals of the C door, which come before any GPU work and so need no GPU."""
import numpy as np
import pytest

import max_pool_backward_cases as PC

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize('kind', ['random', 'ties'])
@pytest.mark.parametrize('hw', PC.MATH_MAPS, ids=lambda hw: '%dx%d' % hw)
def test_float64_statement_equals_torch_autograd(hw, kind):
    from xdet.ops import host_max_pool_backward
    N, C = 2, 3
    rng = np.random.default_rng(hw[0] * 31 + hw[1] + (7 if kind == 'ties' else 0))
    x = PC.make_x(rng, (N,) + hw + (C,), kind)
    dy = rng.standard_normal((N, PC.out_extent(hw[0])[0], PC.out_extent(hw[1])[0], C))
    got = host_max_pool_backward(x, dy, f64)
    want = PC.torch_max_pool_backward(x, dy)
    assert got.dtype == f64 and got.shape == x.shape
    assert np.array_equal(got, want), (hw, kind, np.abs(got - want).max())
    if kind == 'random':
        # tie-free: every dy lands exactly once, so the sums agree up to the rounding of two different summation orders
        assert np.allclose(got.sum(axis=(0, 1, 2)), dy.sum(axis=(0, 1, 2)), rtol=0, atol=1e-12 * max(1., np.abs(dy).sum()))
    else:
        ties = 0
        (Ho, pt), (Wo, pl) = PC.out_extent(hw[0]), PC.out_extent(hw[1])
        for oh in range(Ho):
            for ow in range(Wo):
                win = x[:, max(2 * oh - pt, 0):2 * oh - pt + 3, max(2 * ow - pl, 0):2 * ow - pl + 3]
                ties += int(((win == win.max(axis=(1, 2), keepdims=True)).sum(axis=(1, 2)) > 1).sum())
        assert ties > 0 or hw == (1, 1)


@pytest.mark.parametrize('name', sorted(PC.CASES))
def test_float32_statement_on_the_gpu_cases(name):
    """the cases the GPU test demands bit equality on: the f32 statement is the f64 one rounded nowhere but in the adds, so on
    f32 inputs it equals torch's f32 gradient; and the case table holds what its docstring says"""
    from xdet.ops import host_max_pool_backward
    c = PC.make_case(name)
    got = host_max_pool_backward(c['x'], c['dy'])
    assert got.dtype == f32
    assert np.array_equal(got, PC.torch_max_pool_backward(c['x'], c['dy'])), name
    kind = PC.CASES[name][4]
    N, H, W, C = c['x'].shape
    if kind == 'positions':
        # every window position is the argmax somewhere: channel k's nonzeros sit at window position k
        (Ho, pt), (Wo, pl) = PC.out_extent(H), PC.out_extent(W)
        for k in range(9):
            a, b = divmod(k, 3)
            hits = sum(got[0, 2 * oh - pt + a, 2 * ow - pl + b, k] != 0 for oh in range(Ho) for ow in range(Wo)
                       if 0 <= 2 * oh - pt + a < H and 0 <= 2 * ow - pl + b < W)
            assert hits > 0, k
    Ho = PC.out_extent(H)[0]
    if kind == 'boundary_even':                      # image 0's last row keeps the shares of its last windows
        assert np.allclose(got[0, H - 1].sum(axis=0), c['dy'][0, Ho - 1].sum(axis=0), rtol=0, atol=1e-5)
    if kind == 'boundary_odd':                       # ... and image 1's first row those of its first windows
        assert np.allclose(got[1, 0].sum(axis=0), c['dy'][1, 0].sum(axis=0), rtol=0, atol=1e-5)
    if kind == 'equal':                              # the first in-image element of every window, and nothing else
        (Ho, pt), (Wo, pl) = PC.out_extent(H), PC.out_extent(W)
        want = np.zeros_like(got)
        for oh in range(Ho):
            for ow in range(Wo):
                want[:, max(2 * oh - pt, 0), max(2 * ow - pl, 0)] += c['dy'][:, oh, ow]
        assert np.array_equal(got, want)


def test_a_pixel_in_four_windows_adds_in_ascending_order():
    """x with one dominant pixel at an (even, even) place of an odd map lies in 2 x 2 windows; its four shares are added to 0 in
    ascending (oh, ow) order, each add rounded in f32 -- an order that matters for these values"""
    from xdet.ops import host_max_pool_backward
    x = np.zeros((1, 5, 5, 1), f32)
    x[0, 1, 1, 0] = 9                                # pt = pl = 1: row 1 is the last row of window 0 and the first of window 1
    dy = np.zeros((1, 3, 3, 1), f32)
    shares = np.array([1e8, 1.0, -1e8, 1.0], f32)
    dy[0, :2, :2, 0] = shares.reshape(2, 2)
    got = host_max_pool_backward(x, dy)[0, 1, 1, 0]
    s = f32(0)
    for v in shares:
        s = f32(s + v)
    assert got == s and got != f32(np.sum(shares.astype(f64)))


def test_subsample_and_upsample_against_autograd():
    import torch
    from xdet.ops import host_subsample2, host_add_upsample2
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (5, 4), (6, 7), (2, 2)):
        x = rng.standard_normal((2, H, W, 3))
        xs = host_subsample2(x, f64)
        assert xs.flags['C_CONTIGUOUS'] and np.array_equal(xs, x[:, ::2, ::2])
        g = rng.standard_normal(xs.shape)
        a = rng.standard_normal(x.shape)
        t = torch.tensor(x, requires_grad=True)
        (t[:, ::2, ::2] * torch.tensor(g)).sum().backward()
        # the adjoint of the slice, added to a
        assert np.array_equal(host_add_upsample2(a, g, f64), a + t.grad.numpy())
        # a's bits where nothing arrives, -0.0 included
        a32 = a.astype(f32)
        a32[:, -1, -1] = -0.0 if (H % 2 == 0 or W % 2 == 0) else a32[:, -1, -1]
        out = host_add_upsample2(a32, g.astype(f32))
        miss = np.ones((H, W), bool)
        miss[::2, ::2] = False
        assert np.array_equal(out[:, miss].view(np.uint32), a32[:, miss].view(np.uint32))
    with pytest.raises(ValueError):
        host_add_upsample2(np.zeros((1, 4, 4, 2)), np.zeros((1, 3, 2, 2)))
    with pytest.raises(ValueError):
        from xdet.ops import host_max_pool_backward
        host_max_pool_backward(np.zeros((1, 4, 4, 2)), np.zeros((1, 3, 2, 2)))


def test_c_door_refuses_before_any_gpu_work():
    """XDET_ERR_INVALID_ARG with no device needed: sizes, strides, NULL pointers and N*H*W*C >= 2^31 (the pointers are never
    dereferenced: the checks come first)"""
    from xdet._lib import lib
    L = lib()
    XDET_ERR_INVALID_ARG = -1
    p = 4096                                          # a non-NULL address that is never touched
    pool = lambda x=p, ldx=8, dy=p, ldy=8, N=1, H=4, W=4, C=8, dx=p, ldd=8: \
        L.xdet_maxpool3x3s2_backward(x, ldx, dy, ldy, N, H, W, C, dx, ldd, None)
    for kw in (dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=4097), dict(ldx=7), dict(ldy=7), dict(ldd=7), dict(x=None),
               dict(dy=None), dict(dx=None), dict(N=2, H=32768, W=32768, C=1, ldx=1, ldy=1, ldd=1),
               dict(N=1, H=16384, W=16384, C=8), dict(N=1, H=8192, W=8192, C=8, ldd=32)):
        assert pool(**kw) == XDET_ERR_INVALID_ARG, kw
        assert b'maxpool3x3s2_backward' in L.xdet_last_error()
    sub = lambda x=p, ldx=8, N=1, H=4, W=4, C=8, out=p, ldo=8: L.xdet_subsample2(x, ldx, N, H, W, C, out, ldo, None)
    for kw in (dict(N=0), dict(C=4097), dict(ldx=7), dict(ldo=7), dict(x=None), dict(out=None), dict(N=1, H=16384, W=16384, C=8)):
        assert sub(**kw) == XDET_ERR_INVALID_ARG, kw
    up = lambda a=p, lda=8, b=p, ldb=8, N=1, H=4, W=4, C=8, out=p, ldo=8: L.xdet_add_upsample2(a, lda, b, ldb, N, H, W, C, out, ldo, None)
    for kw in (dict(H=0), dict(C=4097), dict(lda=7), dict(ldb=7), dict(ldo=7), dict(a=None), dict(b=None), dict(out=None),
               dict(N=1, H=16384, W=16384, C=8)):
        assert up(**kw) == XDET_ERR_INVALID_ARG, kw


def test_python_door_refusals_need_no_gpu(monkeypatch):
    import xdet
    from xdet import ops, runtime, train_ops

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops):             # (DeviceTensor.from_numpy and .empty allocate through runtime's names)
        monkeypatch.setattr(mod, 'to_device', no_gpu)
        monkeypatch.setattr(mod, 'DeviceBuffer', no_gpu)
    z = lambda *s: np.zeros(s, f32)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.add_rows_device(z(1, 4, 4, 8), z(1, 4, 3, 8))              # b of another shape
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.max_pool_backward(z(1, 4, 4, 8), z(1, 2, 3, 8))            # dy of another map
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.max_pool_backward(z(1, 4, 4, 8), z(1, 2, 2, 4))
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.max_pool_backward(z(1, 1, 1, 4097), z(1, 1, 1, 4097))
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.add_upsample2_device(z(1, 4, 4, 8), z(1, 2, 3, 8))
    # N*H*W*C = 2^31: views of no memory, refused ahead of any allocation or launch
    from xdet.runtime import DeviceTensor
    big, half = DeviceTensor(4096, (1, 2 ** 16, 2 ** 15, 1), 1), DeviceTensor(4096, (1, 2 ** 15, 2 ** 14, 1), 1)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.max_pool_backward_device(big, half)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.subsample2_device(big)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.add_upsample2_device(big, half)
    # a caller's dx / out of another shape, with NumPy operands: refused ahead of their upload
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.max_pool_backward_device(z(1, 4, 4, 8), z(1, 2, 2, 8), dx=DeviceTensor(4096, (1, 4, 4, 4), 4))
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.subsample2_device(z(1, 4, 4, 8), out=DeviceTensor(4096, (1, 4, 4, 8), 8))
