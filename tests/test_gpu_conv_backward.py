"""xdet_conv_backward (csrc/conv_backward.hip) and model.rpn_backward against the float64 statement
(ops.host_conv_backward, pinned by tests/test_conv_backward_math.py), with the metric and the bar of
tests/conv_backward_cases.py: per output tensor max |got - ref| / max (|A| . |B|) <= max(4 x the f32 statement's distance,
3 * 2^-22) = 7.2e-07 (the statement's distance is 1.3e-07, so the floor decides).
The largest distance measured on an MI355X over all cases of this file is 0.56 of that bar (dW of rpn_head/conv2d through the
net; its dx 0.42; the shape cases reach 0.25, db stays under 0.18)."""
import numpy as np
import pytest

import conv_backward_cases as CC

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-12345.5)


@pytest.fixture(scope='module')
def bar():
    return CC.bar()


def run_raw(x, w, dy, y=None, relu_in=False, pad=(0, 0, 0, 0), with_dx=True, ws_extra=0, poison_ws=False):
    """The C door on padded device copies: pad = extra channels of (x, y, dy, dx), NaN in the inputs' padding and a sentinel
    in dx's.  -> (dx or None, dw, db, dx's padding or None)"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    N, H, W, C = x.shape
    kh, kw, _, J = w.shape

    def padded(a, extra, fill=np.nan):
        p = np.full(a.shape[:3] + (a.shape[3] + extra,), fill, f32)
        p[..., :a.shape[3]] = a
        return p
    d_x, d_w, d_dy = to_device(padded(x, pad[0])), to_device(np.ascontiguousarray(w, f32)), to_device(padded(dy, pad[2]))
    d_y = to_device(padded(y, pad[1])) if y is not None else None
    ld_dx = C + pad[3]
    d_dx = to_device(np.full((N, H, W, ld_dx), SENTINEL, f32)) if with_dx else None
    d_dw, d_db = to_device(np.full(w.shape, SENTINEL, f32)), to_device(np.full((max(J, 4),), SENTINEL, f32))
    nb = lib().xdet_conv_backward_workspace_bytes(N, H, W, C, J, kh, kw)
    assert nb > 0
    ws = to_device(np.full(((nb + ws_extra) // 4,), np.nan, f32)) if poison_ws else DeviceBuffer(nb + ws_extra)
    check(lib().xdet_conv_backward(d_x.ptr, C + pad[0], d_w.ptr, d_y.ptr if y is not None else None, J + pad[1], d_dy.ptr,
                                   J + pad[2], N, H, W, C, J, kh, kw, 1 if relu_in else 0, d_dx.ptr if with_dx else None, ld_dx,
                                   d_dw.ptr, d_db.ptr, ws.ptr, None))
    synchronize()
    dx = tail = None
    if with_dx:
        full = to_host(d_dx.ptr, (N, H, W, ld_dx), f32)
        dx, tail = np.ascontiguousarray(full[..., :C]), full[..., C:]
    return dx, to_host(d_dw.ptr, w.shape, f32), to_host(d_db.ptr, (J,), f32), tail


def judge(what, got, x, w, dy, y, relu_in, bar, ref=None):
    ref, den = ref if ref is not None else CC.reference64(x, w, dy, y, relu_in)
    d = CC.distances(got[:3], ref, den)
    print('%s: distance / bar = %s' % (what, ', '.join('%.4f' % (v / bar) for v in d)))
    assert max(d) <= bar, (what, [v / bar for v in d])
    return max(d) / bar


def bits(a):
    return np.asarray(a).view(np.uint32)


_worst = [0.]


@pytest.mark.parametrize('name', sorted(CC.CASES))
def test_shapes(name, bar):
    """every shape through the Python door (dense pixels); y with its exact zeros where the case has a ReLU"""
    from xdet.ops import conv_backward
    x, w, dy, y, relu_in = CC.make_case(name)
    got = conv_backward(x, w, dy, y, relu_in)
    assert got[0].shape == x.shape and got[1].shape == w.shape and got[2].shape == (w.shape[3],)
    _worst[0] = max(_worst[0], judge(name, got, x, w, dy, y, relu_in, bar, CC.case_reference(name)))
    print('worst distance / bar over the shape cases so far: %.4f' % _worst[0])


@pytest.mark.parametrize('name', ['ragged_3x3', 'range_cuts_row', 'tall_15x1', 'narrow_shape'])
def test_padding_sentinel_null_dx_and_workspace(name, bar):
    """all four ld wider than their widths with NaN in the padding and in the workspace, a sentinel behind dx's width that
    survives; the same bits as the dense-stride call; dx = NULL leaves dw and db as they are; a larger workspace changes
    nothing.  narrow_shape (conv_backward_cases.MORE): a dW of at most 32 x 32, which this door sums on the 128-row tile"""
    x, w, dy, y, relu_in = CC.make_case(name)
    dense = run_raw(x, w, dy, y, relu_in)
    wide = run_raw(x, w, dy, y, relu_in, pad=(14, 7, 3, 5), ws_extra=4096, poison_ws=True)
    judge(name + ' padded', wide, x, w, dy, y, relu_in, bar, CC.case_reference(name))
    assert wide[3].shape[3] == 5 and (wide[3] == SENTINEL).all()
    for a, b in zip(dense[:3], wide[:3]):
        assert np.array_equal(bits(a), bits(b))
    no_dx = run_raw(x, w, dy, y, relu_in, pad=(14, 7, 3, 0), with_dx=False)
    assert no_dx[0] is None and np.array_equal(bits(no_dx[1]), bits(dense[1])) and np.array_equal(bits(no_dx[2]), bits(dense[2]))
    bigger = run_raw(x, w, dy, y, relu_in, ws_extra=1 << 16)
    for a, b in zip(dense[:3], bigger[:3]):
        assert np.array_equal(bits(a), bits(b))


def test_no_reach_across_the_image_border(bar):
    """a gradient at pixel (0, 0) of image 1 only: dx lives in that image's 2 x 2 corner, image 0 gets nothing, and the taps
    that would read x outside the image have dw exactly zero"""
    x, w, dy, y, relu_in = CC.make_case('range_is_image')
    one = np.zeros_like(dy)
    one[1, 0, 0] = dy[1, 0, 0]
    assert (one * (y > 0)).any()
    got = run_raw(x, w, one, y, relu_in)
    judge('corner pixel', got, x, w, one, y, relu_in, bar)
    dx, dw = got[0], got[1]
    assert not dx[0].any()
    inside = np.zeros(dx.shape[1:3], bool)
    inside[:2, :2] = True
    assert not dx[1][~inside].any() and dx[1][inside].all()
    live = np.zeros((3, 3), bool)
    live[1:, 1:] = True                                   # taps (a, b) read x at (a - 1, b - 1): inside for a, b >= 1
    assert not dw[~live].any() and all(dw[a, b].any() for a, b in zip(*np.nonzero(live)))


def test_no_reach_into_the_next_row(bar):
    """1 x 15 with the gradient at the end of a row: nothing lands in the next row or the next image"""
    x, w, dy, y, relu_in = CC.make_case('wide_1x15')
    N, H, W, C = x.shape
    one = np.zeros_like(dy)
    one[0, 1, W - 1] = dy[0, 1, W - 1]
    xpos = np.abs(x) + f32(0.5)                           # relu_in: every x > 0, so the input mask hides nothing
    got = run_raw(xpos, w, one, y, relu_in)
    judge('end of row', got, xpos, w, one, y, relu_in, bar)
    dx, dw = got[0], got[1]
    keep = np.zeros((N, H), bool)
    keep[0, 1] = True
    assert not dx[~keep].any() and dx[0, 1, W - 8:].all() and not dx[0, 1, :W - 8].any()
    # tap b reads x at column W - 1 + b - 7: inside the row for b <= 7 only
    assert not dw[0, 8:].any() and all(dw[0, b].any() for b in range(8))


def test_zero_gradients_and_zero_input():
    x, w, dy, y, relu_in = CC.make_case('ragged_3x3')
    z = run_raw(x, w, np.zeros_like(dy), y, relu_in, pad=(2, 2, 2, 2))
    assert not z[0].any() and not z[1].any() and not z[2].any() and (z[3] == SENTINEL).all()
    x, w, dy, y, relu_in = CC.make_case('ragged_3x3_linear')
    zero_x = run_raw(np.zeros_like(x), w, dy, y, relu_in)        # an all-zero operand of the other product
    assert not zero_x[1].any() and zero_x[0].any()


def test_power_of_two_scaling_is_exact():
    """dy * 2^-30 gives 2^-30 times every output, bit for bit"""
    x, w, dy, y, relu_in = CC.make_case('rpn_widths')
    s = f32(2.0 ** -30)
    a, b = run_raw(x, w, dy, y, relu_in), run_raw(x, w, dy * s, y, relu_in)
    for u, v in zip(a[:3], b[:3]):
        assert u.any() and np.array_equal(bits(u * s), bits(v))


def test_operands_of_1e3_and_1e_minus_7(bar):
    x, w, dy, y, relu_in = CC.make_case('ragged_3x3')
    xs, dys = (x * f32(1e3)).astype(f32), (dy * f32(1e-3)).astype(f32)       # |x| about 1e3, |dy| about 1e-7
    assert 1e2 < np.abs(xs).max() < 1e4 and 1e-8 < np.abs(dys).max() < 1e-6
    judge('1e3 x 1e-7', run_raw(xs, w, dys, y, relu_in), xs, w, dys, y, relu_in, bar)


@pytest.mark.parametrize('name', ['rpn_widths', 'range_cuts_row'])
def test_two_calls_give_the_same_bits(name):
    x, w, dy, y, relu_in = CC.make_case(name)
    a, b = run_raw(x, w, dy, y, relu_in, poison_ws=True), run_raw(x, w, dy, y, relu_in)
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(bits(u), bits(v))


def test_abi_refusals():
    """the refusals of tests/test_conv_backward_math.py with a device present, and through the Python door"""
    import xdet
    from test_conv_backward_math import test_c_door_refuses_before_any_gpu_work as refusals
    refusals()
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.conv_backward(np.zeros((1, 4, 4, 3), f32), np.zeros((3, 3, 2, 5), f32), np.zeros((1, 4, 4, 5), f32))


# ---- through the net -------------------------------------------------------------------------------------------------

def test_rpn_backward_through_the_net(lh_weights, bar):
    """a detector that keeps the RPN's hidden activation: rpn_out has the bits of a detector that does not; rpn_loss with the
    gradient kept on the device, then rpn_backward -- the six weight gradients, d loss / d rpn_hidden and d loss / d mid_x
    against the float64 statements fed the buffers' own contents"""
    import types
    import dense_backward_cases as DC
    import target_cases as C
    from xdet import model as M, losses as L, targets as T, weights as W
    from xdet import InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor, to_host
    S, P, A = 256, 64, 22
    anchor = C.anchors(S)
    labels, boxes = C.make_ground_truth(61, 2, anchor)
    a_l, a_t, _ = T.host_encode_anchors(anchor, labels, boxes)
    images = W.synthetic_images(2, S, seed=3)

    def rpn(det):
        mid, _ = M.XceptionBody(images, 21, is_training=False, data_format='channels_first')
        return M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
    plain = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P)
    with plain.scope():
        cls, box = rpn(plain)
        plain_out = plain.buffer('rpn_out', 2).numpy()
        with pytest.raises(InvalidArgumentError):
            plain.buffer('rpn_hidden', 2)                                   # the name is refused, as pool_index is
        kept = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5, keep_device=True)
        with pytest.raises(InvalidArgumentError):
            M.rpn_backward(kept)                                            # a detector built without the option
    det = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, rpn_hidden=True)
    with det.scope():
        cls, box = rpn(det)
        assert np.array_equal(bits(det.buffer('rpn_out', 2).numpy()), bits(plain_out))
        hid_t, mid_t = det.buffer('rpn_hidden', 2), det.buffer('mid_x', 2)
        hid, mid_x = hid_t.numpy(), mid_t.numpy()
        assert hid.shape == (2, 16, 16, 512) and hid.min() >= 0 and (hid == 0).any() and (hid > 0).any()
        res = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5, keep_device=True)
        losses, sel_index, counts, grad_cls, grad_loc = res                 # the five fields unpack as ever
        plain_res = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5)
        assert plain_res.grad_device is None and all(np.array_equal(bits(a), bits(b)) for a, b in zip(res, plain_res))
        assert res.grad_device.shape == (2, 16, 16, 6 * A) and res.grad_device.ld == det.buffer('rpn_out', 2).ld
        with pytest.raises(InvalidArgumentError):
            M.rpn_backward(plain_res)                                       # not kept on the device
        with pytest.raises(InvalidArgumentError):
            M.rpn_backward(types.SimpleNamespace(grad_device=DeviceTensor.empty((2, 8, 8, 6 * A))))   # another map size
        grads = M.rpn_backward(res)
        d_hid, d_mid = grads['rpn_hidden'].numpy(), grads['mid'].numpy()
        d_mid_raw = to_host(grads['mid'].ptr, (2, 16, 16, grads['mid'].ld))
    assert counts[3] > 0 and grad_cls.any() and grad_loc.any()
    assert grads['mid'].shape == mid_t.shape and grads['mid'].ld == mid_t.ld and d_hid.shape == hid.shape
    k0 = lh_weights['rpn_head/conv2d/kernel']
    k1 = np.concatenate([lh_weights['rpn_head/conv2d_1/kernel'], lh_weights['rpn_head/conv2d_2/kernel']], 3).reshape(512, 6 * A)
    for name in ('conv2d', 'conv2d_1', 'conv2d_2'):
        assert grads['rpn_head/%s/kernel' % name].shape == lh_weights['rpn_head/%s/kernel' % name].shape
        assert grads['rpn_head/%s/bias' % name].shape == lh_weights['rpn_head/%s/bias' % name].shape
    # the two 1x1 heads as one dense layer on the kept gradient
    dy = np.concatenate([grad_cls, grad_loc], -1).reshape(-1, 6 * A)
    kw1 = np.concatenate([grads['rpn_head/conv2d_1/kernel'], grads['rpn_head/conv2d_2/kernel']], 3).reshape(512, 6 * A)
    kb1 = np.concatenate([grads['rpn_head/conv2d_1/bias'], grads['rpn_head/conv2d_2/bias']])
    ref, den = DC.reference64(hid.reshape(-1, 512), k1, dy, None)
    d = DC.distances((d_hid.reshape(-1, 512), kw1, kb1), ref, den)
    print('conv2d_1+conv2d_2: distance / bar = %s' % ', '.join('%.4f' % (v / bar) for v in d))
    assert max(d) <= bar
    # the 3x3 conv: its dy is the first call's dx as the GPU left it
    judge('conv2d', (d_mid, grads['rpn_head/conv2d/kernel'], grads['rpn_head/conv2d/bias']), mid_x, k0, d_hid, hid, True, bar)
    assert (mid_x <= 0).any() and not d_mid[mid_x <= 0].any() and d_mid[mid_x > 0].any()
    assert d_mid_raw.shape[3] > 728 and not d_mid_raw[..., 728:].any()
