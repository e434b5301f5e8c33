"""The native eval net refreshed from trained weights on the device (LightHeadDetector.refresh_weights, xdet_net_refresh_weights;
MomentumOptimizer.refresh_eval_net), on the detector of the flow tests (S = 256, P = 64, max_batch 2, the TRAIN flags of
tests/test_gpu_entry_flow_backward.py).  One module fixture runs everything; the tests read what it recorded.
(a) f16x3, uncalibrated: one training pass, opt.step, refresh_eval_net -- then what the staged calls leave (XceptionBody:
    stem_out, entry_x, mid_x, out; get_rpn: rpn_out; large_sep_kernel: feat; rpn_decode, get_proposals and get_head:
    cls_reg), what the graph forward leaves (feat, rpn_out, cls_reg) and its detections equal, bit for bit, those of a
    detector built from opt.export_weights with the checkpoint's large-separable moving statistics (the training pass moves
    them, and they are outside the refresh's reach); entry_x moved, stem_out did not, and the graph captured before the
    refresh is still the only one.
(b) the same under f32, on `out` and the detections.
(c) a calibrated net: the hot weights Wh are the checkpoint with block7_sepconv2's depthwise kernel x 2^K and its pointwise
    kernel x 2^-K (the same function; the depthwise result leaves the f16 range).  K = the first of 18, 19, ... at which
    calibrate names the unit (the fixture records it; 18 on an MI355X).  A refresh with Wh itself, and one
    with the stepped weights followed by Wh again, leave every bit and every exponent as they were.
(d) calibrate after refresh: a cold net refreshed with Wh overflows as a net built from Wh does, calibrates to the same
    exponents and then agrees with it bit for bit.  Both nets of (d) are built with check_range=True: the overflow of a tensor
    inside the body becomes NaN in the pointwise product and the next ReLU turns NaN into 0, so it never reaches the head
    logits and their always-on guard (with the default detector neither net raises, at any K up to 34, and no buffer from
    mid_x on holds a non-finite word); the validation pass is the project's door for a range violation inside the body
    (tests/test_gpu_proposals.py).
(e) refusals, each with the net's outputs unchanged."""
import numpy as np
import pytest

from flow_train_cases import S, P, NC, bits, head_and_rpn_inputs, downstream
from test_gpu_entry_flow_backward import TRAIN

pytestmark = pytest.mark.gpu
f32 = np.float32
UNIT = 'block7_sepconv2'
LR = 1e-3                                               # a tenth of tests/test_gpu_train_step.py's first rate: at 1e-2 the eval net
                                                        # built from the stepped weights leaves the f16 range on these images
BUFFERS = ('stem_out', 'entry_x', 'mid_x', 'out', 'feat', 'rpn_out', 'cls_reg')


def staged(det, images, head=False):
    """XceptionBody, get_rpn, large_sep_kernel and (head=True: the comparisons of (a) and (b); the chain passes its proposals
    through the host) rpn_decode, get_proposals and get_head on `images`, stage by stage -> {buffer: bits} of what they leave"""
    from xdet import model as M
    n = images.shape[0]
    with det.scope():
        mid, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r = {name: bits(det.buffer(name, n).numpy()) for name in ('stem_out', 'entry_x', 'mid_x', 'out')}
        cls, box = M.get_rpn(mid, 22, False, 'channels_first', 'rpn_head')
        feat = M.large_sep_kernel(out, 256, 490, False, 'channels_first', 'large_sep_feature')
        det.stream.synchronize()
        r.update({'staged/' + name: bits(det.buffer(name, n).numpy()) for name in ('rpn_out', 'feat')})
        if head:
            c = det.cfg
            props = M.get_proposals(*M.rpn_decode(cls, box), None, c.rpn_pre_nms_top_n, c.rpn_post_nms_top_n, c.rpn_nms_thres,
                                    c.rpn_min_size, False, 'channels_first')
            M.get_head(feat, None, 7, 7, None, props, NC, False, False, 0, 'channels_first', 'final_head')
            det.stream.synchronize()
            r['staged/cls_reg'] = bits(det.buffer('cls_reg', n).numpy())
    return r


def detections(det, images):
    """the graph forward -> the bits of what the branches behind the body leave and of the raw detection buffers (read without
    forward()'s finiteness check: equal bits are asked for whatever the values are)"""
    from xdet.runtime import to_host
    n, nc, k = det.set_images(images), det.num_classes - 1, det.nms_topk
    det.forward_device(n, use_graph=True)
    det.stream.synchronize()
    r = {name: bits(det.buffer(name, n).numpy()) for name in ('feat', 'rpn_out', 'cls_reg')}
    r['scores'] = bits(to_host(det._det_scores.ptr, (n, nc, k)))
    r['boxes'] = bits(to_host(det._det_boxes.ptr, (n, nc, k, 4)))
    return r


def everything(det, images, head=False):
    r = staged(det, images, head)
    r.update(detections(det, images))
    return r


def graph_count(det):
    import ctypes
    from xdet._lib import lib, check
    n = ctypes.c_int()
    check(lib().xdet_net_graph_count(det.handle, ctypes.byref(n)))
    return n.value


def equal(a, b, keys=None):
    keys = sorted(set(a) & set(b)) if keys is None else keys
    return {k: int((a[k] != b[k]).sum()) for k in keys if not np.array_equal(a[k], b[k])}


def train_step_and_refresh(w, images, r, tag):
    from xdet import model as M
    from xdet.model import LightHeadDetector
    det = LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
    r[tag + 'before'] = everything(det, images)
    inputs = head_and_rpn_inputs()
    opt = M.MomentumOptimizer(det)
    with det.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        M.entry_flow_train()
        mid_t = M.middle_flow_train()
        lsep, rpn = downstream(M.exit_flow_train(), mid_t, inputs)
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'], weight_grads='device')
        mf = M.middle_flow_backward(ef['mid'], weight_grads='device')
        en = M.entry_flow_backward(mf['entry'], weight_grads='device')
        grads = {}
        for g in (ef, mf, en):
            grads.update(g)
        opt.step(grads, LR)
    stepped = opt.export_weights(w)
    # the training pass also moved the large-separable block's moving statistics, which export_weights carries and which are
    # outside the refresh's reach (the block is not in the optimizer): the rebuilt net keeps the checkpoint's, as `det` does
    stepped.update({name: w[name] for name in M.LARGE_SEP_MOVING})
    det2 = LightHeadDetector(stepped, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
    r[tag + 'rebuilt'] = everything(det2, images, head=True)
    r[tag + 'graphs_before'] = graph_count(det)
    r[tag + 'layers'] = opt.refresh_eval_net()
    r[tag + 'graphs_after'] = graph_count(det)
    r[tag + 'after'] = everything(det, images, head=True)
    r[tag + 'graphs_replayed'] = graph_count(det)
    return det, opt, stepped


@pytest.fixture(scope='module')
def run(lh_weights):
    import xdet
    from xdet import weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision, to_device
    r = {}
    w = lh_weights
    images = W.synthetic_images(2, S, seed=3)
    before = get_precision()
    try:
        set_precision('f16x3')
        det, opt, stepped = train_step_and_refresh(w, images, r, 'a/')
        # (e) refusals on the refreshed net of (a)
        tensors = opt.eval_net_tensors()
        r['e/errors'] = {}
        for what, table in (('rpn', dict(tensors, **{'rpn_head/conv2d/kernel': tensors['conv2d_4/kernel']})),
                            ('partial', {k: v for k, v in tensors.items() if k != UNIT + '_bn/moving_variance'}),
                            ('host', dict(tensors, **{'conv2d_4/kernel': np.zeros((1, 1, 728, 1024), f32)}))):
            with pytest.raises(xdet.InvalidArgumentError) as e:
                det.refresh_weights(table)
            r['e/errors'][what] = str(e.value)
        # the library's own refusals, past the Python checks: a duplicate and a partial group in the C table
        import ctypes
        from xdet._lib import NetWeightDev, lib
        names = sorted(tensors)
        for what, rows in (('duplicate', names + ['conv2d_4/kernel']), ('c_partial', [n for n in names if n != UNIT + '/pointwise_kernel']),
                           ('c_rpn', names + ['rpn_head/conv2d/kernel'])):
            table = (NetWeightDev * len(rows))(*[NetWeightDev(n.encode(), tensors.get(n, tensors['conv2d_4/kernel']).ptr) for n in rows])
            rc = lib().xdet_net_refresh_weights(det.handle, table, len(rows), det.stream.handle)
            r['e/errors'][what] = (rc, lib().xdet_last_error().decode())
        r['e/after'] = everything(det, images)

        # (c) a calibrated net
        k = 18
        while True:
            hot = dict(w)
            hot[UNIT + '/depthwise_kernel'] = np.ldexp(w[UNIT + '/depthwise_kernel'], k).astype(f32)
            hot[UNIT + '/pointwise_kernel'] = np.ldexp(w[UNIT + '/pointwise_kernel'], -k).astype(f32)
            cal = LightHeadDetector(hot, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
            scaled = cal.calibrate(images)
            if any(UNIT in name for name in scaled) or k >= 30:
                break
            k += 1
        r['c/k'], r['c/scaled'] = k, scaled
        r['c/scales0'], r['c/bits0'] = cal.plane_scales(), everything(cal, images)
        reach = sorted(tensors)
        dev = lambda weights: {n: to_device(np.ascontiguousarray(weights[n], f32)) for n in reach}
        d_hot, d_step = dev(hot), dev(stepped)
        cal.refresh_weights(d_hot)
        r['c/scales1'], r['c/bits1'] = cal.plane_scales(), everything(cal, images)
        cal.refresh_weights(d_step)
        r['c/scales2'], r['c/bits_stepped'] = cal.plane_scales(), everything(cal, images)
        cal.refresh_weights(d_hot)
        r['c/scales3'], r['c/bits3'] = cal.plane_scales(), everything(cal, images)

        # (d) calibrate after refresh
        # (check_range=True: an overflow inside the body becomes NaN, which the next ReLU turns into 0 -- it never reaches the
        #  head logits and the always-on guard; the validation pass is the door that sees it, tests/test_gpu_proposals.py)
        cold = LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, check_range=True, **TRAIN)
        cold.refresh_weights(d_hot)
        ref = LightHeadDetector(hot, image_size=S, max_batch=2, rpn_post_nms_top_n=P, check_range=True, **TRAIN)
        r['d/raises'] = []
        for d in (cold, ref):
            try:
                d.forward(images)
                r['d/raises'].append(None)
            except xdet.XdetError as e:
                r['d/raises'].append(str(e))
        r['d/cold_scaled'], r['d/ref_scaled'] = cold.calibrate(images[:1]), ref.calibrate(images[:1])
        r['d/cold'], r['d/ref'] = everything(cold, images), everything(ref, images)

        # (b) f32
        set_precision('f32')
        train_step_and_refresh(w, images, r, 'b/')
    finally:
        set_precision(before)
    return r


def test_a_refreshed_net_equals_a_rebuilt_one(run):
    assert run['a/layers'] == 72
    assert set(BUFFERS) | {'scores', 'boxes', 'staged/rpn_out', 'staged/feat', 'staged/cls_reg'} <= set(run['a/after'])
    assert equal(run['a/after'], run['a/rebuilt']) == {}


def test_a_the_refresh_did_something_and_left_the_stem(run):
    assert not np.array_equal(run['a/after']['entry_x'], run['a/before']['entry_x'])
    assert not np.array_equal(run['a/after']['out'], run['a/before']['out'])
    assert np.array_equal(run['a/after']['stem_out'], run['a/before']['stem_out'])


def test_a_the_graph_cache_stays(run):
    assert run['a/graphs_before'] == run['a/graphs_after'] == run['a/graphs_replayed'] == 1


def test_b_f32(run):
    assert run['b/layers'] == 72
    assert equal(run['b/after'], run['b/rebuilt'], ['out', 'scores', 'boxes']) == {}
    assert not np.array_equal(run['b/after']['out'], run['b/before']['out'])


def test_c_a_calibrated_net_round_trips(run):
    print('k =', run['c/k'], run['c/scaled'])
    assert run['c/scaled'] and any(UNIT in name for name in run['c/scaled'])
    assert equal(run['c/bits1'], run['c/bits0']) == {}
    assert equal(run['c/bits3'], run['c/bits0']) == {}
    assert not np.array_equal(run['c/bits_stepped']['out'], run['c/bits0']['out'])
    assert run['c/scales0'] == run['c/scales1'] == run['c/scales2'] == run['c/scales3']


def test_d_calibrate_after_refresh(run):
    cold, ref = run['d/raises']
    assert cold is not None and ref is not None and 'non-finite' in cold and 'non-finite' in ref
    assert run['d/cold_scaled'] == run['d/ref_scaled'] and run['d/cold_scaled']
    assert equal(run['d/cold'], run['d/ref']) == {}


def test_e_refusals_leave_the_net_unchanged(run):
    err = run['e/errors']
    assert 'rpn_head/conv2d/kernel' in err['rpn'] and 'outside the reach' in err['rpn']
    assert UNIT + '_bn/moving_variance' in err['partial'] and 'in part' in err['partial']
    assert 'conv2d_4/kernel' in err['host'] and 'device memory' in err['host']
    assert err['duplicate'][0] == -1 and 'conv2d_4/kernel is given twice' in err['duplicate'][1]
    assert err['c_partial'][0] == -1 and UNIT + '/pointwise_kernel is missing' in err['c_partial'][1]
    assert err['c_rpn'][0] == -1 and 'rpn_head/conv2d/kernel is outside the reach' in err['c_rpn'][1]
    assert equal(run['e/after'], run['a/after']) == {}
