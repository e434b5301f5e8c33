"""xdet_dense_backward (csrc/dense_backward.hip) and model.head_backward against the float64 statement
(ops.host_dense_backward, pinned by tests/test_dense_backward_math.py), with the metric and the bar of
tests/dense_backward_cases.py: per output tensor max |got - ref| / max (|A| . |B|) <= max(4 x the f32 statement's distance,
3 * 2^-22) = 7.2e-07 (the statement's distance is 1.7e-07, so the floor decides).
The largest distance measured on an MI355X over all cases of this file is 0.32 of that bar (d pooled of subnet_fc through the
net; the shape cases reach 0.26, db stays under 0.11)."""
import ctypes

import numpy as np
import pytest

import dense_backward_cases as DC

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-12345.5)


@pytest.fixture(scope='module')
def bar():
    return DC.bar()


def run_raw(x, w, dy, y=None, pad=(0, 0, 0, 0), with_dx=True, ws_extra=0, poison_ws=False):
    """The C door on padded device copies: pad = extra columns of (x, y, dy, dx), NaN in the inputs' padding and a sentinel
    in dx's.  -> (dx or None, dw, db, dx's padding or None)"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    M, K = x.shape
    J = w.shape[1]

    def padded(a, extra, fill=np.nan):
        p = np.full((a.shape[0], a.shape[1] + extra), fill, f32)
        p[:, :a.shape[1]] = a
        return p
    d_x, d_w, d_dy = to_device(padded(x, pad[0])), to_device(np.ascontiguousarray(w, f32)), to_device(padded(dy, pad[2]))
    d_y = to_device(padded(y, pad[1])) if y is not None else None
    ld_dx = K + pad[3]
    d_dx = to_device(np.full((M, ld_dx), SENTINEL, f32)) if with_dx else None
    d_dw, d_db = to_device(np.full((K, J), SENTINEL, f32)), to_device(np.full((max(J, 4),), SENTINEL, f32))
    nb = lib().xdet_dense_backward_workspace_bytes(M, K, J)
    assert nb > 0
    ws = to_device(np.full(((nb + ws_extra) // 4,), np.nan, f32)) if poison_ws else DeviceBuffer(nb + ws_extra)
    check(lib().xdet_dense_backward(d_x.ptr, K + pad[0], d_w.ptr, d_y.ptr if y is not None else None, J + pad[1], d_dy.ptr,
                                    J + pad[2], M, K, J, d_dx.ptr if with_dx else None, ld_dx, d_dw.ptr, d_db.ptr, ws.ptr, None))
    synchronize()
    dx = tail = None
    if with_dx:
        full = to_host(d_dx.ptr, (M, ld_dx), f32)
        dx, tail = np.ascontiguousarray(full[:, :K]), full[:, K:]
    return dx, to_host(d_dw.ptr, (K, J), f32), to_host(d_db.ptr, (J,), f32), tail


def judge(what, got, x, w, dy, y, bar, ref=None):
    ref, den = ref if ref is not None else DC.reference64(x, w, dy, y)
    d = DC.distances(got[:3], ref, den)
    print('%s: distance / bar = %s' % (what, ', '.join('%.4f' % (v / bar) for v in d)))
    assert max(d) <= bar, (what, [v / bar for v in d])


def bits(a):
    return np.asarray(a).view(np.uint32)


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_shapes(name, bar):
    """every shape through the Python door (dense rows); y with its exact zeros where the case has a ReLU"""
    from xdet.ops import dense_backward
    x, w, dy, y = DC.make_case(name)
    got = dense_backward(x, w, dy, y)
    assert got[0].shape == x.shape and got[1].shape == w.shape and got[2].shape == (w.shape[1],)
    judge(name, got, x, w, dy, y, bar, DC.case_reference(name))


@pytest.mark.parametrize('name', ['ragged', 'ragged_linear', 'last_range_single_row'])
def test_padding_sentinel_null_dx_and_workspace(name, bar):
    """all four ld wider than their widths with NaN in the padding and in the workspace, a sentinel behind dx's width that
    survives; the same bits as the dense call; dx = NULL leaves dw and db as they are; a larger workspace changes nothing"""
    x, w, dy, y = DC.make_case(name)
    dense = run_raw(x, w, dy, y)
    wide = run_raw(x, w, dy, y, pad=(14, 7, 3, 5), ws_extra=4096, poison_ws=True)
    judge(name + ' padded', wide, x, w, dy, y, bar, DC.case_reference(name))
    assert wide[3].shape[1] == 5 and (wide[3] == SENTINEL).all()
    for a, b in zip(dense[:3], wide[:3]):
        assert np.array_equal(bits(a), bits(b))
    no_dx = run_raw(x, w, dy, y, pad=(14, 7, 3, 0), with_dx=False)
    assert no_dx[0] is None and np.array_equal(bits(no_dx[1]), bits(dense[1])) and np.array_equal(bits(no_dx[2]), bits(dense[2]))


def test_zero_and_single_row_gradients(bar):
    x, w, dy, y = DC.make_case('ragged')
    z = run_raw(x, w, np.zeros_like(dy), y, pad=(2, 2, 2, 2))
    assert not z[0].any() and not z[1].any() and not z[2].any() and (z[3] == SENTINEL).all()
    one = np.zeros_like(dy)
    one[37] = dy[37]
    got = run_raw(x, w, one, y)
    judge('single row', got, x, w, one, y, bar)
    assert not np.delete(got[0], 37, axis=0).any() and got[0][37].any()      # rows with no gradient are exact zeros
    zero_x = run_raw(np.zeros_like(x), w, dy, y)                              # an all-zero operand of the other product
    assert not zero_x[1].any() and zero_x[0].any()


def test_power_of_two_scaling_is_exact():
    """dy * 2^-30 gives 2^-30 times every output, bit for bit"""
    x, w, dy, y = DC.make_case('real_k_row_over_tile')
    s = f32(2.0 ** -30)
    a, b = run_raw(x, w, dy, y), run_raw(x, w, dy * s, y)
    for u, v in zip(a[:3], b[:3]):
        assert u.any() and np.array_equal(bits(u * s), bits(v))


def test_operands_of_1e3_and_1e_minus_7(bar):
    x, w, dy, y = DC.make_case('ragged')
    xs, dys = (x * f32(1e3)).astype(f32), (dy * f32(1e-3)).astype(f32)       # |x| about 1e3, |dy| about 1e-7
    assert 1e2 < np.abs(xs).max() < 1e4 and 1e-8 < np.abs(dys).max() < 1e-6
    judge('1e3 x 1e-7', run_raw(xs, w, dys, y), xs, w, dys, y, bar)


def test_two_calls_give_the_same_bits():
    x, w, dy, y = DC.make_case('subnet_fc_widths')
    a, b = run_raw(x, w, dy, y, poison_ws=True), run_raw(x, w, dy, y)
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(bits(u), bits(v))


def test_abi_refusals():
    """the refusals of tests/test_dense_backward_math.py::test_c_door_refuses_before_any_gpu_work with a device present,
    and through the Python door"""
    import xdet
    from test_dense_backward_math import test_c_door_refuses_before_any_gpu_work as refusals
    refusals()
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.dense_backward(np.zeros((4, 3), f32), np.zeros((2, 5), f32), np.zeros((4, 5), f32))


def test_head_backward_through_the_net(lh_weights, bar):
    """a 64-ROI head detector: get_head in training mode with OHEM 32, then head_backward -- the six weight gradients and
    d loss / d pooled against the float64 statement fed the buffers' own contents; rows of ROIs OHEM dropped are exact zeros"""
    from xdet import model as M, losses as L
    from xdet.model import LightHeadDetector
    from xdet.ops import host_dense_backward
    S, P, nc = 256, 64, 21
    head = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P)
    rng = np.random.default_rng(11)
    with head.scope():
        shp = head.buffer('feat', 2).shape
        feat = rng.standard_normal(shp).astype(f32)
        c, hw = rng.uniform(0.25, 0.75, (2, P, 2)), rng.uniform(0.1, 0.4, (2, P, 2))
        rois = np.concatenate([c - hw / 2, c + hw / 2], -1).astype(f32)
        labels = rng.integers(-1, nc, (2, P)).astype(np.int32)
        targets = (rng.standard_normal((2, P, 4)) * 0.2).astype(f32)
        with pytest.raises(ValueError):
            M.head_backward(L.HeadLoss(labels, targets, 0.25))                  # the losses have not run
        loss_func = L.HeadLoss(labels, targets, 0.25)
        M.get_head(feat, None, 7, 7, loss_func, rois, nc, True, True, 32, 'channels_first', 'final_head')
        grads = M.head_backward(loss_func)
        pooled = head.buffer('pooled', 2).numpy().reshape(2 * P, -1)
        fc = head.buffer('fc', 2).numpy().reshape(2 * P, -1)
    res = loss_func.result
    dy = np.concatenate([res.grad_cls, res.grad_reg], -1).reshape(2 * P, nc + 4)
    assert dy.any() and pooled.shape[1] == 490 and fc.shape[1] == 2048 and (fc == 0).any()
    w0 = lh_weights['final_head/subnet_fc/kernel']
    w1 = np.concatenate([lh_weights['final_head/fc_cls/kernel'], lh_weights['final_head/fc_loc/kernel']], 1)
    d_fc = grads['fc'].numpy().reshape(2 * P, -1)
    d_pooled = grads['pooled'].numpy().reshape(2 * P, -1)
    assert grads['pooled'].shape == (2, P, 1, 490)
    kw1 = np.concatenate([grads['final_head/fc_cls/kernel'], grads['final_head/fc_loc/kernel']], 1)
    kb1 = np.concatenate([grads['final_head/fc_cls/bias'], grads['final_head/fc_loc/bias']])
    assert grads['final_head/fc_cls/kernel'].shape == (2048, nc) and grads['final_head/fc_loc/bias'].shape == (4,)
    judge('fc_cls+fc_loc', (d_fc, kw1, kb1), fc, w1, dy, None, bar)
    # the second layer's dy is the first call's dx as the GPU left it
    judge('subnet_fc', (d_pooled, grads['final_head/subnet_fc/kernel'], grads['final_head/subnet_fc/bias']), pooled, w0, d_fc, fc, bar)
    kept = np.zeros((2, P), bool)
    for n in range(2):
        kept[n, res.select[n]] = True
    assert res.select.shape == (2, 32) and not d_pooled[~kept.reshape(-1)].any() and d_pooled[kept.reshape(-1)].any()
    assert not host_dense_backward(fc, w1, dy, None, dtype=np.float64)[0][~kept.reshape(-1)].any()
