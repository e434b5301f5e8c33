"""The operand conventions of the *_device doors of xdet/train_ops.py, at one small ragged shape per door.  The same call is made
with NumPy operands, with DeviceTensor.from_numpy operands (ld 64 for 40 channels) and, where the door takes dx= / out=, into a
caller's DeviceTensor of ld 96: all give the same bits (compared as uint32), because the kernels' sums depend on the sizes alone
(csrc/backward_gemm.h, csrc/pool_backward.hip) and never on a pixel stride.  A fresh result has the operand's ld for a
DeviceTensor operand, the width for a NumPy operand of the GEMM / batch-norm / depthwise doors (uploaded densely) and
channel_ld(C) for one of the pool / add doors (uploaded as DeviceTensor.from_numpy pads it); a caller's tensor comes back as the
same object.  Two doors state their own ld whatever the operand's: dense_backward_device's dx is [M,1,1,K] with ld K, and
subsample2_device's fresh out has ld channel_ld(C).  Kernels (w, k) on the device are dense, as the doors demand."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
N, H, W, C, J = 2, 5, 7, 40, 24
M, K = 70, 40
LD_DEV, LD_MINE = 64, 96                    # channel_ld(40); a caller's tensor


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(*arrays):
    return all(a.shape == arrays[0].shape and np.array_equal(bits(a), bits(arrays[0])) for a in arrays[1:])


def rng():
    return np.random.default_rng(20)


def normal(r, *shape):
    return r.standard_normal(shape).astype(f32)


def act(a):
    from xdet.runtime import DeviceTensor
    t = DeviceTensor.from_numpy(a if a.ndim == 4 else a.reshape(a.shape[0], 1, 1, a.shape[1]))
    assert t.ld == LD_DEV or a.shape[-1] != C
    return t


def dense(a):
    """a kernel on the device, ld = its last dimension"""
    from xdet.runtime import DeviceTensor, to_device
    buf = to_device(np.ascontiguousarray(a, f32))
    return DeviceTensor(buf.ptr, a.shape if a.ndim == 4 else (1, 1) + a.shape, a.shape[-1], buf)


def mine(*shape):
    from xdet.runtime import DeviceTensor
    return DeviceTensor.empty(shape, ld=LD_MINE)


def host(t, shape=None):
    """a result after the synchronisation: a DeviceTensor's values, or a DeviceBuffer's as `shape`"""
    from xdet.runtime import DeviceTensor, to_host
    return t.numpy() if isinstance(t, DeviceTensor) else to_host(t.ptr, shape, f32)


def test_dense():
    from xdet.train_ops import dense_backward_device
    from xdet.runtime import synchronize
    r = rng()
    x, w, dy = normal(r, M, K), normal(r, K, J), normal(r, M, J)
    y = np.maximum(normal(r, M, J), 0)
    a = dense_backward_device(x, w, dy, y)
    b = dense_backward_device(act(x), dense(w), act(dy), act(y))
    synchronize()
    for got in (a, b):
        assert got[0].shape == (M, 1, 1, K) and got[0].ld == K           # this door's dx is dense whatever x's ld
    for i, shape in enumerate((None, (K, J), (J,))):
        assert same(host(a[i], shape), host(b[i], shape)), i
    assert host(a[0]).any() and host(a[1], (K, J)).any()


def test_conv():
    from xdet.train_ops import conv_backward_device
    from xdet.runtime import synchronize
    r = rng()
    x, w, dy = normal(r, N, H, W, C), normal(r, 3, 3, C, J), normal(r, N, H, W, J)
    y = np.maximum(normal(r, N, H, W, J), 0)
    tx, tw, td, ty = act(x), dense(w), act(dy), act(y)
    a = conv_backward_device(x, w, dy, y)
    b = conv_backward_device(tx, tw, td, ty)
    own = mine(N, H, W, C)
    c = conv_backward_device(tx, tw, td, ty, dx=own)
    synchronize()
    assert a[0].ld == C and b[0].ld == LD_DEV and b[0].ptr != tx.ptr and c[0] is own and own.ld == LD_MINE
    for i, shape in enumerate((None, (3, 3, C, J), (J,))):
        assert same(host(a[i], shape), host(b[i], shape), host(c[i], shape)), i
    assert host(a[0]).any() and host(a[0]).shape == (N, H, W, C)


def test_depthwise():
    from xdet.train_ops import depthwise_backward_device
    from xdet.runtime import synchronize
    r = rng()
    x, k, dy = normal(r, N, H, W, C), normal(r, 3, 3, C, 1), normal(r, N, H, W, C)
    tx, tk, td = act(x), dense(k), act(dy)
    a = depthwise_backward_device(x, k, dy, 2, True)
    b = depthwise_backward_device(tx, tk, td, 2, True)
    own = mine(N, H, W, C)
    c = depthwise_backward_device(tx, tk, td, 2, True, dx=own)
    synchronize()
    assert a[0].ld == C and b[0].ld == LD_DEV and b[0].ptr != tx.ptr and c[0] is own and own.ld == LD_MINE
    for i, shape in enumerate((None, (3, 3, C, 1))):
        assert same(host(a[i], shape), host(b[i], shape), host(c[i], shape)), i
    dx = host(a[0])
    assert dx.any() and not dx[~(x > 0)].any()                            # relu_in: no gradient where x > 0 is false


def test_batch_norm():
    from xdet.train_ops import batch_norm_forward_device, batch_norm_backward_device
    from xdet.runtime import synchronize
    r = rng()
    x, dy = normal(r, N, H, W, C), normal(r, N, H, W, C)
    gamma, beta, mm, mv = normal(r, C), normal(r, C), normal(r, C), np.abs(normal(r, C)) + f32(0.5)
    tx = act(x)
    fa = batch_norm_forward_device(x, gamma, beta, 1e-5, True, 0.9, mm, mv, relu=True)
    fb = batch_norm_forward_device(tx, gamma, beta, 1e-5, True, 0.9, mm, mv, relu=True)
    synchronize()
    assert fa[0].ld == C and fb[0].ld == LD_DEV and fb[0].ptr != tx.ptr and fa[0].shape == fb[0].shape == (N, H, W, C)
    y = host(fa[0])
    assert same(y, host(fb[0])) and (y == 0).any() and (y > 0).any()     # the ReLU mask the backward reads masks something
    for i in range(1, 5):
        assert same(host(fa[i], (C,)), host(fb[i], (C,))), i
    assert not same(host(fa[3], (C,)), mm)                                # the moving mean moved
    ba = batch_norm_backward_device(x, y, dy, gamma, fa[1], fa[2])
    bb = batch_norm_backward_device(tx, fb[0], act(dy), gamma, fb[1], fb[2])
    own = mine(N, H, W, C)
    bc = batch_norm_backward_device(tx, fb[0], act(dy), gamma, fb[1], fb[2], dx=own)
    synchronize()
    assert ba[0].ld == C and bb[0].ld == LD_DEV and bb[0].ptr != tx.ptr and bc[0] is own and own.ld == LD_MINE
    for i, shape in enumerate((None, (C,), (C,))):
        assert same(host(ba[i], shape), host(bb[i], shape), host(bc[i], shape)), i
    assert host(ba[0]).any()


def test_max_pool():
    from xdet.train_ops import max_pool_backward_device
    from xdet.runtime import synchronize
    r = rng()
    x, dy = normal(r, N, H, W, C), normal(r, N, 3, 4, C)
    tx, td = act(x), act(dy)
    a = max_pool_backward_device(x, dy)
    b = max_pool_backward_device(tx, td)
    own = mine(N, H, W, C)
    c = max_pool_backward_device(tx, td, dx=own)
    synchronize()
    assert a.ld == LD_DEV and b.ld == tx.ld == LD_DEV and b.ptr != tx.ptr and c is own and own.ld == LD_MINE
    assert same(host(a), host(b), host(c)) and host(a).any()


def test_subsample2():
    from xdet.train_ops import subsample2_device, host_subsample2
    from xdet.runtime import synchronize
    x = normal(rng(), N, H, W, C)
    tx = act(x)
    a, b, own = subsample2_device(x), subsample2_device(tx), mine(N, 3, 4, C)
    c = subsample2_device(tx, out=own)
    synchronize()
    assert a.ld == LD_DEV and b.ld == LD_DEV and c is own and own.ld == LD_MINE and a.shape == (N, 3, 4, C)
    assert same(host(a), host(b), host(c), host_subsample2(x))


def test_add_rows_and_add_upsample2():
    from xdet.train_ops import add_rows_device, add_upsample2_device
    from xdet.runtime import synchronize
    r = rng()
    p, q, half = normal(r, N, H, W, C), normal(r, N, H, W, C), normal(r, N, 3, 4, C)
    for door, second in ((add_rows_device, q), (add_upsample2_device, half)):
        ta, tb = act(p), act(second)
        a, b, own = door(p, second), door(ta, tb), mine(N, H, W, C)
        c = door(ta, tb, out=own)
        synchronize()
        assert a.ld == LD_DEV and b.ld == ta.ld == LD_DEV and b.ptr != ta.ptr and c is own and own.ld == LD_MINE
        assert same(host(a), host(b), host(c)) and not same(host(a), p)
        # out = a: the result replaces a, which keeps b alive (on top of what it kept) until the stream has run the call
        want = host(a)
        back = door(ta, tb, out=ta)
        assert back is ta and any(k is tb for k in ta._keep) and not any(k is ta for k in ta._keep)
        del tb, b, c
        synchronize()
        assert same(host(ta), want), door.__name__
