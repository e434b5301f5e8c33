"""xdet_maxpool3x3s2_backward, xdet_subsample2 and xdet_add_upsample2 (csrc/pool_backward.hip) against the host statements
(ops.host_max_pool_backward, host_subsample2, host_add_upsample2, pinned against torch.autograd by
tests/test_max_pool_backward_math.py), on the cases of tests/max_pool_backward_cases.py.  There is no tolerance: every result
must have the f32 statement's bits (compared as uint32, so the sign of a zero counts too).
Each case runs dense through the Python door and again through the C door with every pixel stride above C: NaN behind the
channels of x and dy, which must reach no result, and a sentinel behind those of dx, which must survive."""
import numpy as np
import pytest

import max_pool_backward_cases as PC

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-12345.5)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def padded(a, extra, fill=np.nan):
    p = np.full(a.shape[:-1] + (a.shape[-1] + extra,), fill, f32)
    p[..., :a.shape[-1]] = a
    return p


def raw_pool(x, dy, pad=(0, 0, 0)):
    """the C door on padded device copies -> (dx, dx's padding)"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, synchronize
    N, H, W, C = x.shape
    d_x, d_dy = to_device(padded(x, pad[0])), to_device(padded(dy, pad[1]))
    d_dx = to_device(np.full((N, H, W, C + pad[2]), SENTINEL, f32))
    check(lib().xdet_maxpool3x3s2_backward(d_x.ptr, C + pad[0], d_dy.ptr, C + pad[1], N, H, W, C, d_dx.ptr, C + pad[2], None))
    synchronize()
    full = to_host(d_dx.ptr, (N, H, W, C + pad[2]), f32)
    return np.ascontiguousarray(full[..., :C]), full[..., C:]


@pytest.mark.parametrize('name', sorted(PC.CASES))
def test_cases(name):
    from xdet.ops import max_pool_backward, host_max_pool_backward
    c = PC.make_case(name)
    want = host_max_pool_backward(c['x'], c['dy'])
    got = max_pool_backward(c['x'], c['dy'])
    assert got.shape == c['x'].shape and got.dtype == f32
    assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
    assert np.array_equal(bits(max_pool_backward(c['x'], c['dy'])), bits(got))                 # the same call, the same bits
    C = c['x'].shape[3]
    for pad in ((3, 5, 7), (64 - C % 64,) * 3, (0, 0, 0)):            # scalar accesses, float4 accesses with ld > C, dense
        dx, tail = raw_pool(c['x'], c['dy'], pad)
        assert np.array_equal(bits(dx), bits(want)), (name, pad)
        assert (tail == SENTINEL).all(), (name, pad)
    # dy * 2^k -> dx * 2^k exactly: the op only moves and adds
    s = f32(2.0 ** -7)
    assert want.any() and np.array_equal(bits(raw_pool(c['x'], c['dy'] * s)[0]), bits(want * s))


def test_dx_into_a_callers_tensor():
    from xdet.ops import max_pool_backward_device, host_max_pool_backward
    from xdet.runtime import DeviceTensor, synchronize
    c = PC.make_case('c64')
    N, H, W, C = c['x'].shape
    x, dy = DeviceTensor.from_numpy(c['x']), DeviceTensor.from_numpy(c['dy'])
    mine = DeviceTensor.empty((N, H, W, C), ld=96)
    out = max_pool_backward_device(x, dy, dx=mine)
    synchronize()
    assert out is mine and np.array_equal(bits(mine.numpy()), bits(host_max_pool_backward(c['x'], c['dy'])))
    fresh = max_pool_backward_device(x, dy)
    synchronize()
    assert fresh.ptr != x.ptr and fresh.ld == x.ld and np.array_equal(bits(fresh.numpy()), bits(mine.numpy()))


@pytest.mark.parametrize('shape', [(2, 7, 5, 8), (2, 6, 8, 5), (1, 5, 6, 64), (1, 1, 1, 3), (1, 2, 2, 728), (1, 1, 5, 8)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_subsample_and_add_upsample(shape):
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, synchronize
    from xdet.ops import host_subsample2, host_add_upsample2
    N, H, W, C = shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    rng = np.random.default_rng(H * 100 + W * 10 + C)
    x = rng.standard_normal(shape).astype(f32)
    b = rng.standard_normal((N, Ho, Wo, C)).astype(f32)
    a = x.copy()
    if W > 1:
        a[:, 0, 1] = -0.0
    elif H > 1:
        a[:, 1, 0] = -0.0
    miss = np.ones((H, W), bool)
    miss[::2, ::2] = False
    want_sub, want_up = host_subsample2(x), host_add_upsample2(a, b)
    if miss.any():
        assert (bits(a[:, miss]) == 0x80000000).any()               # a -0.0 at a pixel nothing is added to
    for px, pb, po in ((3, 5, 7), (64 - C % 64,) * 3, (0, 0, 0)):
        d_x = to_device(padded(x, px))
        d_o = to_device(np.full((N, Ho, Wo, C + po), SENTINEL, f32))
        check(lib().xdet_subsample2(d_x.ptr, C + px, N, H, W, C, d_o.ptr, C + po, None))
        synchronize()
        out = to_host(d_o.ptr, (N, Ho, Wo, C + po), f32)
        assert np.array_equal(bits(out[..., :C]), bits(want_sub)) and (out[..., C:] == SENTINEL).all()
        d_a, d_b = to_device(padded(a, px)), to_device(padded(b, pb))
        d_o = to_device(np.full((N, H, W, C + po), SENTINEL, f32))
        check(lib().xdet_add_upsample2(d_a.ptr, C + px, d_b.ptr, C + pb, N, H, W, C, d_o.ptr, C + po, None))
        synchronize()
        out = to_host(d_o.ptr, (N, H, W, C + po), f32)
        assert np.array_equal(bits(out[..., :C]), bits(want_up)) and (out[..., C:] == SENTINEL).all()
        # out = a: a's padding stays what it was
        d_a = to_device(padded(a, px, SENTINEL))
        check(lib().xdet_add_upsample2(d_a.ptr, C + px, d_b.ptr, C + pb, N, H, W, C, d_a.ptr, C + px, None))
        synchronize()
        out = to_host(d_a.ptr, (N, H, W, C + px), f32)
        assert np.array_equal(bits(out[..., :C]), bits(want_up)) and (out[..., C:] == SENTINEL).all()


def test_python_doors_of_the_gather_and_the_join():
    from xdet.ops import subsample2_device, add_upsample2_device, host_subsample2, host_add_upsample2
    from xdet.runtime import DeviceTensor, synchronize
    rng = np.random.default_rng(9)
    x = rng.standard_normal((2, 5, 6, 40)).astype(f32)
    b = rng.standard_normal((2, 3, 3, 40)).astype(f32)
    tx, tb = DeviceTensor.from_numpy(x), DeviceTensor.from_numpy(b)
    xs = subsample2_device(tx)
    mine = DeviceTensor.empty((2, 3, 3, 40), ld=128)
    assert subsample2_device(x, out=mine) is mine
    fresh = add_upsample2_device(tx, tb)
    synchronize()
    assert np.array_equal(bits(xs.numpy()), bits(host_subsample2(x))) and np.array_equal(bits(mine.numpy()), bits(host_subsample2(x)))
    assert fresh.ptr != tx.ptr and fresh.ld == tx.ld and np.array_equal(bits(fresh.numpy()), bits(host_add_upsample2(x, b)))
    same = add_upsample2_device(tx, tb, out=tx)
    synchronize()
    assert same is tx and np.array_equal(bits(tx.numpy()), bits(host_add_upsample2(x, b)))


def test_refusals(monkeypatch):
    """the refusals of tests/test_max_pool_backward_math.py with a device present (the Python doors' with every upload and
    allocation turned into a failure, as there), and dx / out of the wrong shape"""
    import xdet
    from xdet.runtime import DeviceTensor
    import test_max_pool_backward_math as T
    T.test_c_door_refuses_before_any_gpu_work()
    with monkeypatch.context() as m:
        T.test_python_door_refusals_need_no_gpu(m)
    z = lambda *s: np.zeros(s, f32)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.max_pool_backward_device(z(1, 4, 4, 8), z(1, 2, 2, 8), dx=DeviceTensor.empty((1, 4, 5, 8)))
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.max_pool_backward_device(z(1, 4, 4, 8), z(1, 2, 2, 8), dx=z(1, 4, 4, 8))
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.subsample2_device(z(1, 4, 4, 8), out=DeviceTensor.empty((1, 4, 4, 8)))
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.add_upsample2_device(z(1, 4, 4, 8), z(1, 2, 2, 8), out=DeviceTensor.empty((1, 2, 2, 8)))
