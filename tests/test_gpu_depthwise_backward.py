"""xdet_depthwise_backward and xdet_add_rows (csrc/depthwise_backward.hip) against the host statements
(ops.host_depthwise_backward, pinned by tests/test_depthwise_backward_math.py), with the cases, the metric and the bar of
tests/depthwise_backward_cases.py: dx must EQUAL the f32 statement (np.array_equal: every bit but the sign of a zero); dw per
tensor max |got - ref64| / max sum |xe| |g| <= max(4 x the f32 statement's distance, 3 * 2^-22) = 7.2e-07 (the statement's
distance is 9.9e-08, so the floor is the bar).
Measured on an MI355X, worst dw distance / bar over all cases of this file: 0.14 (`widest`: four pixels; `chunk_growth` 0.02)."""
import numpy as np
import pytest

import depthwise_backward_cases as DC

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-12345.5)


@pytest.fixture(scope='module')
def bar():
    return DC.bar()


def bits(a):
    return np.asarray(a).view(np.uint32)


def padded(a, extra, fill=np.nan):
    p = np.full(a.shape[:-1] + (a.shape[-1] + extra,), fill, f32)
    p[..., :a.shape[-1]] = a
    return p


def raw(c, pad=(0, 0, 0), x=None, dy=None, with_dx=True, ws_extra=0, poison_ws=False):
    """The C door on padded device copies: pad = extra channels of (x, dy, dx), NaN in the inputs' padding, a sentinel in
    dx's -> (dx or None, dw, dx's padding or None)"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    x, dy = c['x'] if x is None else x, c['dy'] if dy is None else dy
    N, H, W, C = x.shape
    d_x, d_dy, d_k = to_device(padded(x, pad[0])), to_device(padded(dy, pad[1])), to_device(c['k'])
    ld_dx = C + pad[2]
    d_dx = to_device(np.full((N, H, W, ld_dx), SENTINEL, f32)) if with_dx else None
    d_dw = to_device(np.full((max(9 * C, 4),), SENTINEL, f32))
    nb = lib().xdet_depthwise_backward_workspace_bytes(N, H, W, C)
    assert nb > 0
    ws = to_device(np.full(((nb + ws_extra) // 4,), np.nan, f32)) if poison_ws else DeviceBuffer(nb + ws_extra)
    check(lib().xdet_depthwise_backward(d_x.ptr, C + pad[0], d_k.ptr, d_dy.ptr, C + pad[1], N, H, W, C, c['dilation'],
                                        1 if c['relu_in'] else 0, d_dx.ptr if with_dx else None, ld_dx, d_dw.ptr, ws.ptr, None))
    synchronize()
    dx = tail = None
    if with_dx:
        full = to_host(d_dx.ptr, (N, H, W, ld_dx), f32)
        dx, tail = np.ascontiguousarray(full[..., :C]), full[..., C:]
    return dx, to_host(d_dw.ptr, (3, 3, C, 1), f32), tail


_worst = [0.]


def judge(name, c, got, bar, x=None, label=''):
    """dx equal to the f32 statement, dw inside the bar"""
    from xdet.ops import host_depthwise_backward
    xx = c['x'] if x is None else x
    want_dx = host_depthwise_backward(xx, c['k'], c['dy'], c['dilation'], c['relu_in'])[0]
    (_, ref_dw), den = DC.case_reference(name) if x is None else DC.reference64(xx, c['k'], c['dy'], c['dilation'], c['relu_in'])
    if got[0] is not None:
        assert got[0].shape == xx.shape and np.array_equal(got[0], want_dx), name
    d = DC.dw_distance(got[1], ref_dw, den)
    _worst[0] = max(_worst[0], d / bar)
    print('%s%s: dw distance / bar = %.4f (worst so far %.4f)' % (name, label, d / bar, _worst[0]))
    assert d <= bar, (name, d / bar)


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_cases_dense(name, bar):
    """ld = C through the Python door; twice: the same bits; without dx: the same dw bits"""
    from xdet.ops import depthwise_backward
    c = DC.make_case(name)
    got = depthwise_backward(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'])
    judge(name, c, got, bar)
    again = depthwise_backward(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'])
    assert np.array_equal(bits(got[0]), bits(again[0])) and np.array_equal(bits(got[1]), bits(again[1]))
    no_dx = depthwise_backward(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'], with_dx=False)
    assert no_dx[0] is None and np.array_equal(bits(no_dx[1]), bits(got[1]))
    if name == 'two_images':
        assert got[0][0].any() and not got[0][1].any() and not got[1].any()
    if name == 'one_pixel':       # only the centre tap exists
        assert np.array_equal(got[0], c['dy'] * c['k'][1, 1, :, 0]) and not np.delete(got[1].reshape(9, -1), 4, axis=0).any()


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_cases_padded(name, bar):
    """every ld = C + 3 (scalar accesses wherever C + 3 is no multiple of 4) with NaN in the inputs' padding and in the
    workspace, a sentinel behind dx's width that survives; the same bits as the dense call and as a float4-aligned one"""
    c = DC.make_case(name)
    C = c['x'].shape[3]
    dense = raw(c)
    wide = raw(c, pad=(3, 3, 3), ws_extra=4096, poison_ws=True)
    judge(name, c, wide, bar, label=' padded')
    assert wide[2].shape[-1] == 3 and (wide[2] == SENTINEL).all()
    p = 64 - C % 64
    aligned = raw(c, pad=(p, p, p))
    assert (aligned[2] == SENTINEL).all()
    no_dx = raw(c, pad=(3, 3, 0), with_dx=False, poison_ws=True)
    for other in (wide, aligned):
        assert np.array_equal(bits(dense[0]), bits(other[0])) and np.array_equal(bits(dense[1]), bits(other[1]))
    assert no_dx[0] is None and np.array_equal(bits(no_dx[1]), bits(dense[1]))


@pytest.mark.parametrize('name', ['ragged', 'dilated', 'exit_width'])
def test_power_of_two_scaling_is_exact(name):
    c = DC.make_case(name)
    s = f32(2.0 ** -20)
    a, b = raw(c), raw(c, dy=c['dy'] * s)
    for u, v in zip(a[:2], b[:2]):
        assert u.any() and np.array_equal(bits(u * s), bits(v))


def test_nan_in_x_under_relu_in(bar):
    """x > 0 is false for a NaN: dx is 0 there and the sums stay finite -- the same bits as with a zero in its place"""
    c = DC.make_case('ragged')
    x = c['x'].copy()
    pos = np.argwhere(x > 0)[:12]
    x[tuple(pos[:6].T)] = np.nan
    x[tuple(pos[6:].T)] = 0
    got = raw(c, x=x, pad=(2, 2, 2))
    want = raw(c, x=np.nan_to_num(x, nan=0.))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and not got[0][tuple(pos.T)].any()
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    judge('ragged', c, want, bar, x=np.nan_to_num(x, nan=0.), label=' with planted NaN')
    assert not np.array_equal(raw(c)[1], got[1])


def test_refusals():
    """the refusals of tests/test_depthwise_backward_math.py with a device present, and through the Python door"""
    import xdet
    from test_depthwise_backward_math import test_c_door_refuses_before_any_gpu_work as refusals
    refusals()
    z = lambda *s: np.zeros(s, f32)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.depthwise_backward(z(1, 4, 4, 8), z(3, 3, 8, 1), z(1, 4, 4, 8), dilation=3)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.depthwise_backward(z(1, 1, 1, 4097), z(3, 3, 4097, 1), z(1, 1, 1, 4097))


def test_add_rows():
    """exact against numpy on 70 rows of 50 channels with three different padded lds; out aliasing a; padding untouched"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, synchronize, DeviceTensor
    from xdet.ops import add_rows_device
    rng = np.random.default_rng(3)
    M, C = 70, 50
    a, b = rng.standard_normal((M, C)).astype(f32), rng.standard_normal((M, C)).astype(f32)
    for pa, pb, po in ((3, 5, 7), (14, 14, 14), (0, 0, 0)):
        d_a, d_b = to_device(padded(a, pa)), to_device(padded(b, pb))
        d_o = to_device(np.full((M, C + po), SENTINEL, f32))
        check(lib().xdet_add_rows(d_a.ptr, C + pa, d_b.ptr, C + pb, d_o.ptr, C + po, M, C, None))
        synchronize()
        out = to_host(d_o.ptr, (M, C + po), f32)
        assert np.array_equal(bits(out[:, :C]), bits(a + b)) and (out[:, C:] == SENTINEL).all()
        # out = a: the padding of a stays what it was
        d_a2 = to_device(padded(a, pa, SENTINEL))
        check(lib().xdet_add_rows(d_a2.ptr, C + pa, d_b.ptr, C + pb, d_a2.ptr, C + pa, M, C, None))
        synchronize()
        out = to_host(d_a2.ptr, (M, C + pa), f32)
        assert np.array_equal(bits(out[:, :C]), bits(a + b)) and (out[:, C:] == SENTINEL).all()
    ta, tb = DeviceTensor.from_numpy(a.reshape(2, 5, 7, C)), DeviceTensor.from_numpy(b.reshape(2, 5, 7, C))
    fresh = add_rows_device(ta, tb)
    assert fresh.ptr != ta.ptr and fresh.ld == ta.ld and np.array_equal(bits(fresh.numpy()), bits((a + b).reshape(2, 5, 7, C)))
    same = add_rows_device(ta, tb, out=ta)
    synchronize()
    assert same is ta and np.array_equal(bits(ta.numpy()), bits((a + b).reshape(2, 5, 7, C)))
