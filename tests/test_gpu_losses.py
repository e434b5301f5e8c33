"""xdet_rpn_loss / xdet_head_loss (csrc/losses.hip) against the NumPy statement of the same contract (xdet/losses.py, itself
pinned by tests/test_losses_math.py): the selections, counts and the zero / non-zero pattern of every gradient bit for
bit; losses, per-ROI values and gradients against the float64 statement, within four times the f32 statement's own largest
distance from it over the cases of tests/loss_cases.py (relative to max(1, |value|); expf / logf may round differently by an
ulp and the reduction tree is not NumPy's pairwise sum).  That distance, measured on the CPU: 2.3e-07, so the bar is 9.3e-07.
The largest distance measured on an MI355X over all cases of this file is 0.24 of that bar (per_roi of the OHEM cases; the
scalar losses reach 0.13, the gradients 0.01)."""

import numpy as np
import pytest

import loss_cases as LC
from test_losses_math import rpn_distance, head_distance, bad_calls

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope='module')
def bar():
    """four times the largest distance of the f32 statement from the float64 one, over every case"""
    d = max([rpn_distance(n)[0] for n in LC.RPN_CASES] + [head_distance(n)[0] for n in LC.HEAD_CASES])
    print('f32 statement vs float64: %.3e -> bar %.3e' % (d, 4 * d))
    assert d > 0
    return 4 * d


def assert_floats(what, bar, pairs):
    worst = 0.
    for name, got, want64 in pairs:
        d = LC.distance(got, want64)
        print('%s: %s, distance / bar = %.4f over %d values' % (what, name, d / bar, np.asarray(got).size))
        worst = max(worst, d)
    assert worst <= bar, (what, worst / bar)


def same_pattern(got, want):
    return np.array_equal(np.asarray(got) != 0, np.asarray(want) != 0)


def check_rpn(name, bar):
    from xdet import losses as L
    cls, loc, labels, targets, api, fg, seed = LC.rpn_case(name)
    _, w32, w64 = rpn_distance(name)
    got = L.rpn_loss(cls, loc, labels, targets, api, fg, seed)
    assert np.array_equal(got.sel_index, w32.sel_index) and np.array_equal(got.counts, w32.counts), (name, got.counts, w32.counts)
    g_cls, g_loc = LC.anchor_major(got.grad_cls, 2), LC.anchor_major(got.grad_loc, 4)
    assert same_pattern(g_cls, w32.grad_cls) and same_pattern(g_loc, w32.grad_loc), name
    assert_floats(name, bar, (('losses', got.losses, w64.losses), ('grad_cls', g_cls, w64.grad_cls), ('grad_loc', g_loc, w64.grad_loc)))
    return got


@pytest.mark.parametrize('name', sorted(LC.RPN_CASES))
def test_rpn_loss(name, bar):
    got = check_rpn(name, bar)
    if name == 'nothing':
        assert (got.sel_index == -1).all() and not got.losses.any() and got.counts[2] == 0
    if name == 'no_pos':
        assert got.losses[1] == 0 and got.counts[3] == 0 and got.losses[0] > 0
    if name in ('down_both_128x480', 'dense_128x64'):
        assert got.counts[2] == 128 * 256 and got.counts[3] == 8192


def check_head(name, bar):
    from xdet import losses as L
    args = LC.head_case(name)
    _, w32, w64 = head_distance(name)
    got = L.head_loss(*args)
    assert np.array_equal(got.select, w32.select), name
    assert same_pattern(got.grad_cls, w32.grad_cls) and same_pattern(got.grad_reg, w32.grad_reg), name
    assert_floats(name, bar, (('losses', got.losses, w64.losses), ('per_roi', got.per_roi, w64.per_roi),
                              ('grad_cls', got.grad_cls, w64.grad_cls), ('grad_reg', got.grad_reg, w64.grad_reg)))
    return got, args


@pytest.mark.parametrize('name', sorted(LC.HEAD_CASES))
def test_head_loss(name, bar):
    got, args = check_head(name, bar)
    if name == 'image_all_ignored':
        assert not got.per_roi[1].any() and not got.grad_cls[1].any() and np.array_equal(got.select[1], np.arange(16))
    if name == 'logits_to_50':
        assert np.isfinite(got.per_roi).all() and got.per_roi.max() > 40
    if name == 'no_ohem':
        assert np.array_equal(got.select, np.tile(np.arange(64), (4, 1)))
    # the per-ROI value of bit-equal rows is bit-equal
    grp = LC.duplicate_groups(*args[:4])
    for n in range(grp.shape[0]):
        for g in np.unique(grp[n]):
            assert len(set(got.per_roi[n][grp[n] == g].view(np.uint32).tolist())) == 1


# ---- control words, determinism ----------------------------------------------------------------------------------------

def raw_rpn(case, ws, out, poison=False):
    """the C ABI on caller-owned buffers (ld 132: cls at 0, box at 44) -> every output as host arrays"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, synchronize
    cls, loc, labels, targets, api, fg, seed = case
    N, hw = cls.shape[:2]
    S = N * api
    packed = np.concatenate([cls, loc], -1)
    dev = [to_device(packed), to_device(labels), to_device(targets)]
    if poison:
        check(lib().xdet_memset(ws.ptr, 0xA5, ws.nbytes, None))
        check(lib().xdet_memset(out[3].ptr, 0xA5, N * hw * 132 * 4, None))
    check(lib().xdet_rpn_loss(dev[0].ptr, 132, 0, 44, N, hw, 1, LC.A, dev[1].ptr, dev[2].ptr, api, fg, seed, 1., ws.ptr, out[0].ptr,
                              out[1].ptr, out[2].ptr, out[3].ptr, None))
    synchronize()
    return (to_host(out[0].ptr, (S,), np.int32), to_host(out[1].ptr, (4,), np.int32), to_host(out[2].ptr, (3,), f32),
            to_host(out[3].ptr, (N, hw, 132), f32))


def test_rpn_workspace_reuse_poison_and_determinism(bar):
    """a call with a smaller N in the workspace (and output buffers) of a larger one; the workspace and the gradient buffer
    poisoned before the call; the same call twice -> identical bits in every output"""
    from xdet import losses as L
    from xdet._lib import lib
    from xdet.runtime import DeviceBuffer
    big, small = LC.rpn_case('short_pos'), LC.rpn_case('short_neg_tail')
    N, hw = big[0].shape[:2]
    ws = DeviceBuffer(lib().xdet_losses_workspace_bytes(N, 256))
    out = [DeviceBuffer(N * 256 * 4), DeviceBuffer(16), DeviceBuffer(16), DeviceBuffer(N * hw * 132 * 4)]
    first = raw_rpn(big, ws, out, poison=True)
    again = raw_rpn(big, ws, out)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    w = L.host_rpn_loss(LC.anchor_major(big[0], 2), LC.anchor_major(big[1], 4), *big[2:])
    assert np.array_equal(first[0], w.sel_index) and np.array_equal(first[1], w.counts)
    w64 = L.host_rpn_loss(LC.anchor_major(small[0], 2), LC.anchor_major(small[1], 4), *small[2:], dtype=np.float64)
    for case in (small, small):
        got = raw_rpn(case, ws, out)
        w = L.host_rpn_loss(LC.anchor_major(case[0], 2), LC.anchor_major(case[1], 4), *case[2:])
        assert np.array_equal(got[0], w.sel_index) and np.array_equal(got[1], w.counts)
        g_cls, g_loc = got[3][..., :44].reshape(-1, 2), got[3][..., 44:].reshape(-1, 4)
        assert same_pattern(g_cls, w.grad_cls) and same_pattern(g_loc, w.grad_loc)
        assert_floats('smaller N in the larger workspace', bar, (('losses', got[2], w64.losses), ('grad_cls', g_cls, w64.grad_cls),
                                                                  ('grad_loc', g_loc, w64.grad_loc)))
    poisoned = raw_rpn(small, ws, out, poison=True)
    for a, b in zip(got, poisoned):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_head_loss_twice_and_poisoned_workspace():
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    cls, reg, labels, targets, fg, k = LC.head_case('ohem_k_lt_p')
    N, P, Cn = cls.shape
    packed = np.zeros((N, P, 28), f32)
    packed[..., :Cn], packed[..., Cn:Cn + 4] = cls, reg
    dev = [to_device(packed), to_device(labels), to_device(targets)]
    ws = DeviceBuffer(lib().xdet_losses_workspace_bytes(16, 0))
    out = [DeviceBuffer(16), DeviceBuffer(N * P * 4), DeviceBuffer(N * k * 4), DeviceBuffer(N * P * 28 * 4)]
    runs = []
    for poison in (True, False, True):
        if poison:
            check(lib().xdet_memset(ws.ptr, 0xA5, ws.nbytes, None))
            check(lib().xdet_memset(out[3].ptr, 0xA5, N * P * 28 * 4, None))
        check(lib().xdet_head_loss(dev[0].ptr, 28, 0, Cn, N, P, Cn, dev[1].ptr, dev[2].ptr, fg, k, 1., ws.ptr, out[0].ptr, out[1].ptr,
                                   out[2].ptr, out[3].ptr, None))
        synchronize()
        runs.append((to_host(out[0].ptr, (3,), f32), to_host(out[1].ptr, (N, P), f32), to_host(out[2].ptr, (N, k), np.int32),
                     to_host(out[3].ptr, (N, P, 28), f32)[..., :Cn + 4]))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_argument_errors_are_raised_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import runtime

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    monkeypatch.setattr(runtime, 'to_device', no_gpu)
    monkeypatch.setattr(runtime, 'DeviceBuffer', no_gpu)
    for call in bad_calls():
        with pytest.raises(xdet.InvalidArgumentError):
            call()


# ---- through the net -------------------------------------------------------------------------------------------------

def test_through_the_net(lh_weights, bar):
    """rpn_out of a detector -> rpn_loss on the device views == the call on their NumPy copies, bit for bit;
    get_proposals(is_training=True) -> get_head(is_training=True, using_ohem=True, 32) on a 64-ROI head detector ==
    host_head_loss on that detector's eval get_head logits, select exact"""
    import target_cases as C
    from xdet import model as M, losses as L, targets as T
    from xdet import weights as W
    from xdet.model import LightHeadDetector
    S, R, pre, P = 256, 300, 5000, 64
    det = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_pre_nms_top_n=pre, rpn_post_nms_top_n=R)
    head = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_pre_nms_top_n=pre, rpn_post_nms_top_n=P)
    anchor = C.anchors(S)
    labels, boxes = C.make_ground_truth(61, 2, anchor)
    a_l, a_t, _ = T.host_encode_anchors(anchor, labels, boxes)
    with det.scope():
        mid, out = M.XceptionBody(W.synthetic_images(2, S, seed=3), 21, is_training=False, data_format='channels_first')
        cls, box = M.get_rpn(mid, 22, False, 'channels_first', 'rpn_head')
        on_dev = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5)
        on_host = L.rpn_loss(cls.numpy(), box.numpy(), a_l, a_t, 256, 0.25, seed=5)
        for a, b in zip(on_dev, on_host):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        w = L.host_rpn_loss(LC.anchor_major(cls.numpy(), 2), LC.anchor_major(box.numpy(), 4), a_l, a_t, 256, 0.25, seed=5)
        assert np.array_equal(on_dev.sel_index, w.sel_index) and np.array_equal(on_dev.counts, w.counts) and w.counts[3] > 0
        assert LC.distance(on_dev.losses, w.losses.astype(np.float64)) <= bar
        feat = M.large_sep_kernel(out, 256, 490, False, 'channels_first', 'large_sep_feature').numpy()
        obj, rb = M.rpn_decode(cls, box)
        props = M.get_proposals(obj, rb, None, pre, R, 0.7, 16. / 480, False, 'channels_first')
        for n in range(2):                         # boxes the proposals can match: some of the forward's own
            boxes[n][0] = props[n, 0]
            boxes[n][-1] = props[n, 5]
        enc = T.AnchorEncoder([anchor], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.)
        r, t, l, s = M.get_proposals(obj, rb, lambda rois: enc.ext_encode_rois(rois, labels, boxes, P, 0.25, 0.1, seed=4), pre, R,
                                     0.7, 16. / 480, True, 'channels_first')
        assert r.shape == (2, P, 4) and (l > 0).any()
        with pytest.raises(ValueError):           # this detector's head has R rows
            M.get_head(feat, None, 7, 7, L.HeadLoss(l, t, 0.25), r, 21, True, True, 32, 'channels_first', 'final_head')
    with head.scope():
        loss_func = L.HeadLoss(l, t, 0.25)
        loss = M.get_head(feat, None, 7, 7, loss_func, r, 21, True, True, 32, 'channels_first', 'final_head')
        c, g = M.get_head(feat, None, 7, 7, None, r, 21, False, False, 32, 'channels_first', 'final_head')
        with pytest.raises(ValueError):
            M.get_head(feat, None, 7, 7, None, r, 21, True, True, 32, 'channels_first', 'final_head')
    res = loss_func.result
    w32 = L.host_head_loss(c, g, l, t, 0.25, 32)
    w64 = L.host_head_loss(c, g, l, t, 0.25, 32, dtype=np.float64)
    assert np.array_equal(res.select, w32.select) and res.select.shape == (2, 32)
    assert loss == float(res.losses[0])
    assert same_pattern(res.grad_cls, w32.grad_cls) and same_pattern(res.grad_reg, w32.grad_reg)
    assert_floats('through the net', bar, (('losses', res.losses, w64.losses), ('per_roi', res.per_roi, w64.per_roi),
                                           ('grad_cls', res.grad_cls, w64.grad_cls), ('grad_reg', res.grad_reg, w64.grad_reg)))
