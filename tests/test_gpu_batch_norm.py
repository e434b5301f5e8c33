"""xdet_batch_norm_forward / xdet_batch_norm_backward (csrc/batchnorm.hip) against the float64 statements
(ops.host_batch_norm_forward / host_batch_norm_backward, pinned by tests/test_batch_norm_math.py), with the cases, the metric
and the bar of tests/batch_norm_cases.py: per tensor max |got - ref| / max |magnitude| <= max(4 x the f32 statement's
distance, 3 * 2^-22) = 3.8e-05 (the statement's distance is 9.4e-06: numpy's sequential f32 sum of 65537 squares on
`chunk_growth`).  Each check measures one step: the statistics against float64 of x, y against float64 with the op's own
statistics, the backward against float64 fed the op's statistics and the op's y.
Measured on an MI355X, worst distance / bar over all cases of this file: 0.0175 (the variance of `chunk_growth` in training
mode: 1009 chunks of 65 rows against numpy's one sequential sum; `chunk_tail` 0.0065); every y, dx, dgamma and dbeta stays under
0.004.  Mutations run on the GPU: without the xhat dgamma / M term of dx every training-mode case but `one_row` fails, with the
padded cases, the planted-mask case and the chain through the net; with an E[x^2] - E[x]^2 variance `offset` fails in training
mode; fed a y recomputed from x instead of the one given, test_nan_and_planted_zeros_in_y_mask fails in both modes (on the
forward's own y a recomputed mask has the same bits, so the shape cases cannot see it)."""
import numpy as np
import pytest

import batch_norm_cases as BC

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-12345.5)


@pytest.fixture(scope='module')
def bar():
    return BC.bar()


def bits(a):
    return np.asarray(a).view(np.uint32)


def padded(a, extra, fill=np.nan):
    p = np.full((a.shape[0], a.shape[1] + extra), fill, f32)
    p[:, :a.shape[1]] = a
    return p


def raw_forward(c, training, pad=(0, 0), moving=True, ws_extra=0, poison_ws=False):
    """The C door on padded device copies: pad = extra channels of (x, y), NaN in x's padding, a sentinel in y's.
    -> (y, mean, invstd, moving_mean, moving_var, y's padding)"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    x = c['x']
    M, C = x.shape
    d_x, d_g, d_b = to_device(padded(x, pad[0])), to_device(c['gamma']), to_device(c['beta'])
    d_mm = to_device(c['moving_mean']) if moving else None
    d_mv = to_device(c['moving_var']) if moving else None
    ld_y = C + pad[1]
    d_y = to_device(np.full((M, ld_y), SENTINEL, f32))
    d_mean, d_inv = to_device(np.full((max(C, 4),), SENTINEL, f32)), to_device(np.full((max(C, 4),), SENTINEL, f32))
    nb = lib().xdet_batch_norm_workspace_bytes(M, C)
    assert nb > 0
    ws = to_device(np.full(((nb + ws_extra) // 4,), np.nan, f32)) if poison_ws else DeviceBuffer(nb + ws_extra)
    check(lib().xdet_batch_norm_forward(d_x.ptr, C + pad[0], M, C, d_g.ptr, d_b.ptr, BC.EPS, 1 if training else 0, BC.MOMENTUM,
                                        d_mm.ptr if moving else None, d_mv.ptr if moving else None, 1 if c['relu'] else 0,
                                        d_y.ptr, ld_y, d_mean.ptr, d_inv.ptr, ws.ptr, None))
    synchronize()
    full = to_host(d_y.ptr, (M, ld_y), f32)
    vec = lambda b: to_host(b.ptr, (C,), f32) if b is not None else None
    return np.ascontiguousarray(full[:, :C]), vec(d_mean), vec(d_inv), vec(d_mm), vec(d_mv), full[:, C:]


def raw_backward(c, training, y, mean, invstd, dy=None, pad=(0, 0, 0, 0), with_dx=True, ws_extra=0, poison_ws=False):
    """pad = extra channels of (x, y, dy, dx): NaN in the inputs' padding, a sentinel in dx's -> (dx or None, dgamma, dbeta,
    dx's padding or None)"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    x, dy = c['x'], c['dy'] if dy is None else dy
    M, C = x.shape
    d_x, d_dy, d_g = to_device(padded(x, pad[0])), to_device(padded(dy, pad[2])), to_device(c['gamma'])
    d_y = to_device(padded(y, pad[1])) if y is not None else None
    d_mean, d_inv = to_device(mean), to_device(invstd)
    ld_dx = C + pad[3]
    d_dx = to_device(np.full((M, ld_dx), SENTINEL, f32)) if with_dx else None
    d_dg, d_db = to_device(np.full((max(C, 4),), SENTINEL, f32)), to_device(np.full((max(C, 4),), SENTINEL, f32))
    nb = lib().xdet_batch_norm_workspace_bytes(M, C)
    ws = to_device(np.full(((nb + ws_extra) // 4,), np.nan, f32)) if poison_ws else DeviceBuffer(nb + ws_extra)
    check(lib().xdet_batch_norm_backward(d_x.ptr, C + pad[0], d_y.ptr if y is not None else None, C + pad[1], d_dy.ptr,
                                         C + pad[2], M, C, d_g.ptr, d_mean.ptr, d_inv.ptr, 1 if training else 0,
                                         d_dx.ptr if with_dx else None, ld_dx, d_dg.ptr, d_db.ptr, ws.ptr, None))
    synchronize()
    dx = tail = None
    if with_dx:
        full = to_host(d_dx.ptr, (M, ld_dx), f32)
        dx, tail = np.ascontiguousarray(full[:, :C]), full[:, C:]
    return dx, to_host(d_dg.ptr, (C,), f32), to_host(d_db.ptr, (C,), f32), tail


_worst = [0.]


def judge(what, d, bar):
    print('%s: distance / bar = %s' % (what, ', '.join('%s %.4f' % (k, v / bar) for k, v in sorted(d.items()))))
    assert max(d.values()) <= bar, (what, {k: v / bar for k, v in d.items()})
    _worst[0] = max(_worst[0], max(d.values()) / bar)
    print('worst distance / bar so far: %.4f' % _worst[0])


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('name', sorted(BC.CASES))
def test_cases_through_the_python_door(name, training, bar):
    """forward with the moving statistics, then the backward fed the forward's own statistics and y"""
    from xdet.ops import batch_norm_forward, batch_norm_backward
    c = BC.make_case(name)
    fw = batch_norm_forward(c['x'], c['gamma'], c['beta'], BC.EPS, training, BC.MOMENTUM, c['moving_mean'], c['moving_var'],
                            c['relu'])
    y, mean, invstd, mm, mv = fw
    assert y.shape == c['x'].shape and mean.shape == invstd.shape == mm.shape == mv.shape == (c['x'].shape[1],)
    assert all(np.isfinite(a).all() for a in fw)
    if c['relu']:
        assert (y == 0).any() and (y > 0).any()
    judge('%s forward' % name, BC.forward_distances(name, training, fw), bar)
    if not training:        # bit for bit untouched, and what was used is what is saved
        assert np.array_equal(bits(mm), bits(c['moving_mean'])) and np.array_equal(bits(mv), bits(c['moving_var']))
        assert np.array_equal(bits(mean), bits(c['moving_mean']))
    yy = y if c['relu'] else None
    bw = batch_norm_backward(c['x'], yy, c['dy'], c['gamma'], mean, invstd, training)
    assert bw[0].shape == c['x'].shape and all(np.isfinite(a).all() for a in bw)
    judge('%s backward' % name, BC.backward_distances(name, training, yy, mean, invstd, bw), bar)
    if name == 'one_row' and training:
        assert not bw[0].any() and not bw[1].any() and np.array_equal(bits(bw[2]), bits(c['dy'][0]))


def test_moving_statistics_are_skipped_without_pointers(bar):
    c = BC.make_case('ragged')
    with_m, without = raw_forward(c, True), raw_forward(c, True, moving=False)
    assert without[3] is None and without[4] is None
    for a, b in zip(with_m[:3], without[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(with_m[3], c['moving_mean']) and not np.array_equal(with_m[4], c['moving_var'])
    judge('ragged moving', BC.forward_distances('ragged', True, with_m[:5]), bar)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('name', ['ragged', 'large_sep_widths', 'chunk_tail', 'one_channel'])
def test_padding_sentinel_null_dx_and_workspace(name, training, bar):
    """every ld wider than C with NaN in the inputs' padding and in the workspace, a sentinel behind y's and dx's width that
    survives; the same bits as the dense-stride call (vector or scalar loads do not change the sums); dx = NULL leaves
    dgamma and dbeta as they are; a larger workspace changes nothing"""
    c = BC.make_case(name)
    dense = raw_forward(c, training)
    wide = raw_forward(c, training, pad=(14, 5), ws_extra=4096, poison_ws=True)
    aligned = raw_forward(c, training, pad=(64 - c['x'].shape[1] % 64, 64 - c['x'].shape[1] % 64))    # float4 rows
    judge(name + ' padded forward', BC.forward_distances(name, training, wide[:5]), bar)
    assert wide[5].shape[1] == 5 and (wide[5] == SENTINEL).all() and (aligned[5] == SENTINEL).all()
    for other in (wide, aligned):
        for a, b in zip(dense[:5], other[:5]):
            assert np.array_equal(bits(a), bits(b))
    y, mean, invstd = dense[0] if c['relu'] else None, dense[1], dense[2]
    bd = raw_backward(c, training, y, mean, invstd)
    bw = raw_backward(c, training, y, mean, invstd, pad=(14, 7, 3, 5), ws_extra=4096, poison_ws=True)
    p = 64 - c['x'].shape[1] % 64
    ba = raw_backward(c, training, y, mean, invstd, pad=(p, p, p, p))
    judge(name + ' padded backward', BC.backward_distances(name, training, y, mean, invstd, bw[:3]), bar)
    assert bw[3].shape[1] == 5 and (bw[3] == SENTINEL).all() and (ba[3] == SENTINEL).all()
    for other in (bw, ba, raw_backward(c, training, y, mean, invstd, ws_extra=1 << 16)):
        for a, b in zip(bd[:3], other[:3]):
            assert np.array_equal(bits(a), bits(b))
    no_dx = raw_backward(c, training, y, mean, invstd, pad=(14, 7, 3, 0), with_dx=False)
    assert no_dx[0] is None and np.array_equal(bits(no_dx[1]), bits(bd[1])) and np.array_equal(bits(no_dx[2]), bits(bd[2]))


@pytest.mark.parametrize('name', ['large_sep_widths', 'chunk_growth'])
def test_two_calls_give_the_same_bits(name):
    c = BC.make_case(name)
    a, b = raw_forward(c, True, poison_ws=True), raw_forward(c, True)
    for u, v in zip(a[:5], b[:5]):
        assert np.array_equal(bits(u), bits(v))
    y = a[0] if c['relu'] else None
    p, q = raw_backward(c, True, y, a[1], a[2], poison_ws=True), raw_backward(c, True, y, a[1], a[2])
    for u, v in zip(p[:3], q[:3]):
        assert np.array_equal(bits(u), bits(v))


@pytest.mark.parametrize('training', [True, False])
def test_power_of_two_scaling_is_exact(training):
    """dy * 2^-20 gives 2^-20 times dx, dgamma and dbeta, bit for bit"""
    c = BC.make_case('large_sep_widths')
    fw = raw_forward(c, training)
    s = f32(2.0 ** -20)
    a = raw_backward(c, training, fw[0], fw[1], fw[2])
    b = raw_backward(c, training, fw[0], fw[1], fw[2], dy=c['dy'] * s)
    for u, v in zip(a[:3], b[:3]):
        assert u.any() and np.array_equal(bits(u * s), bits(v))


@pytest.mark.parametrize('training', [True, False])
def test_nan_and_planted_zeros_in_y_mask(training, bar):
    """the mask is the given y: NaNs and zeros planted where the forward's y is positive mask there (a y recomputed from x
    would not), the sums stay finite, and in eval mode dx is exactly 0 there"""
    c = BC.make_case('ragged')
    fw = raw_forward(c, training)
    y = fw[0].copy()
    pos = np.argwhere(y > 0)
    assert len(pos) > 40
    y[tuple(pos[:10].T)] = np.nan
    y[tuple(pos[10:20].T)] = 0
    dy = c['dy'].copy()
    dy[tuple(pos[:3].T)] = np.nan                       # a NaN in a masked dy is dropped
    got = raw_backward(c, training, y, fw[1], fw[2], dy=dy, pad=(2, 2, 2, 2))
    assert all(np.isfinite(a).all() for a in got[:3])
    y0, dy0 = np.nan_to_num(y, nan=0.), c['dy'].copy()
    dy0[tuple(pos[:3].T)] = 0
    want = raw_backward(c, training, y0, fw[1], fw[2], dy=dy0)
    for u, v in zip(got[:3], want[:3]):
        assert np.array_equal(bits(u), bits(v))
    judge('planted mask', BC.backward_distances('ragged', training, y0, fw[1], fw[2], want[:3]), bar)
    if not training:
        assert not got[0][tuple(pos[:20].T)].any()
    plain = raw_backward(c, training, fw[0], fw[1], fw[2])
    assert not np.array_equal(plain[2], got[2])


def test_constant_channel_is_finite(bar):
    c = BC.make_case('constant_channel')
    fw = raw_forward(c, True, pad=(3, 3))
    assert all(np.isfinite(a).all() for a in fw[:5])
    assert fw[1][3] == f32(0.75) and abs(fw[2][3] - 1 / np.sqrt(BC.EPS)) <= 1e-3 * fw[2][3]
    assert np.array_equal(fw[0][:, 3], np.full(64, max(c['beta'][3], 0), f32))      # xhat = 0 there: y = max(beta, 0)
    bw = raw_backward(c, True, fw[0], fw[1], fw[2])
    assert all(np.isfinite(a).all() for a in bw[:3]) and bw[1][3] == 0


def test_abi_refusals():
    """the refusals of tests/test_batch_norm_math.py with a device present, and through the Python door"""
    import xdet
    from test_batch_norm_math import test_c_door_refuses_before_any_gpu_work as refusals
    refusals()
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.batch_norm_forward(np.zeros((4, 3), f32), np.ones(3, f32), np.zeros(3, f32), 1e-5, training=False)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.batch_norm_forward(np.zeros((4, 3), f32), np.ones(2, f32), np.zeros(3, f32), 1e-5)
