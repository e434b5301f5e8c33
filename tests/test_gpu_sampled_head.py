"""The sampled-ROI head on one detector (LightHeadDetector(head_rois=P), option "head_rois"): the proposal stage on
rpn_post_nms_top_n = 1800 ROIs per image, the head stage on the P = 64 the training step samples from them, the sampled set
handed over on the device.  S = 256, max_batch 2, rpn_pre_nms_top_n 5000, the TRAIN flags of
tests/test_gpu_entry_flow_backward.py (pool_index among them), f16x3.  One module fixture builds `det_one` (as above) and
`det_head` (the same flags, rpn_post_nms_top_n = 64, no head_rois: the head detector of the two-detector arrangement), runs
everything once, and the tests read what it recorded.

The chain on det_one is the training step's: the eval body, the three training flows, get_rpn on the training-mode `mid`,
rpn_decode, get_proposals(is_training=True) with an encode_fn that samples with keep_device=True (ground truth planted on two of
the net's own proposals per image, as tests/test_gpu_targets.py::test_get_proposals_training_branch does), the training
large-separable block, get_head with OHEM 32 on the device ROIs and a HeadLoss on the device labels and targets, and
head_backward(to_feat=True, weight_grads='device'); then the other backwards, so that one step of
MomentumOptimizer(det_one, reach='all') can follow.

Every comparison is for equal bits -- the head stage of det_one is the plan of det_head on the same values, and no op of it runs
a float atomic -- but the sampled targets, which keep the bar of tests/test_gpu_targets.py (logf may round differently from
NumPy's).  The batch-below-max_batch test feeds the head one image's `feat` rows of the two-image run: the training-mode batch
norm in front of `feat` makes that tensor depend on the batch, the head behind it is per image.  It runs image 0 as the issue
asks and image 1 as well: image 0's rows start at offset 0 whatever the strides are, image 1's do not.

Figures of the run on an MI355X that this file was written against are printed by the fixture (`-s`)."""
import ctypes
import time

import numpy as np
import pytest

import target_cases as C

from flow_train_cases import S, NC, A, MID, CO, bits, head_and_rpn_inputs
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_optimizer_heads import SECTIONS, weight_gradients
from test_gpu_targets import ROI, assert_targets

pytestmark = pytest.mark.gpu
f32 = np.float32
R, PRE, P, OHEM = 1800, 5000, 64, 32
NMS, MIN_SIZE = 0.7, 16. / 480
LR, MOMENTUM, WEIGHT_DECAY = 1e-3, 0.9, 2e-4             # tests/test_gpu_optimizer_heads.py's
HEAD_GRADS = ['final_head/%s/%s' % (l, k) for l in ('subnet_fc', 'fc_cls', 'fc_loc') for k in ('kernel', 'bias')]
LOSS_FIELDS = ('losses', 'per_roi', 'select', 'grad_cls', 'grad_reg')


def host(v):
    return v.numpy() if hasattr(v, 'numpy') else np.asarray(v)


def head_pass(det, feat, rois, labels, targets, n):
    """get_head(is_training=True, OHEM 32) and head_backward(to_feat=True, weight_grads='device') on the current detector
    -> the bits of everything they leave, and head_backward's dict with the loss_func under 'loss_func'"""
    from xdet import model as M, losses as L
    loss_func = L.HeadLoss(labels, targets, 0.25)
    M.get_head(feat, None, 7, 7, loss_func, rois, NC, True, True, OHEM, 'channels_first', 'final_head')
    r = {'cls_reg': bits(det.buffer('cls_reg', n).numpy()), 'fwd/pooled': bits(det.buffer('pooled', n).numpy()),
         'fwd/pool_index': bits(det.buffer('pool_index', n).numpy())}
    r.update({'loss/' + k: bits(np.asarray(getattr(loss_func.result, k)).astype(f32)) for k in LOSS_FIELDS})
    back = M.head_backward(loss_func, to_feat=True, weight_grads='device')
    r.update({k: bits(host(back[k])) for k in HEAD_GRADS + ['pooled', 'fc', 'feat']})
    back['loss_func'] = loss_func
    return r, back


def differing(a, b, keys=None):
    keys = sorted(set(a) | set(b)) if keys is None else keys
    return [k for k in keys if k not in a or k not in b or a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]


def refusal(call):
    import xdet
    try:
        call()
        return None
    except xdet.XdetError as e:
        return (type(e).__name__, e.code, str(e))


@pytest.fixture(scope='module')
def run(lh_weights):
    import xdet
    from xdet import model as M, losses as L, targets as T, train, weights as W
    from xdet._lib import lib, LightHeadConfig
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor, get_precision, set_precision, to_device, to_host
    t0 = time.time()
    r = {}
    images = W.synthetic_images(2, S, seed=3)
    _, _, _, a_l, a_t = head_and_rpn_inputs()
    anchors = C.anchors(S)
    glabels, gboxes = C.make_ground_truth(61, 2, anchors)
    enc = T.AnchorEncoder([anchors], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.)
    one = dict(TRAIN, image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R, head_rois=P)
    before = get_precision()
    set_precision('f16x3')
    try:
        # ---- refusals of the constructor and of the option itself (no net is built)
        r['ctor'] = {v: refusal(lambda: LightHeadDetector(lh_weights, **dict(one, head_rois=v))) for v in (0, R + 1, 'x')}
        cfg = LightHeadConfig(image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R)
        h = ctypes.c_void_p()
        assert lib().xdet_net_create(ctypes.byref(h), ctypes.byref(cfg)) == 0
        r['option'] = {}
        for v in (b'0', str(R + 1).encode(), b'x', b'', b'64x', b'-3', b'off', b'64', b'1', str(R).encode()):
            r['option'][v] = (lib().xdet_net_set_option(h, b'head_rois', v), lib().xdet_last_error().decode())
        lib().xdet_net_destroy(h)

        det_one = LightHeadDetector(lh_weights, **one)
        det_head = LightHeadDetector(lh_weights, **dict(TRAIN, image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=P))
        r['build_seconds'] = time.time() - t0
        r['head_R'] = (det_one.head_R, det_one.R, det_head.head_R, det_head.R, det_one.head_rois, det_head.head_rois)
        r['shapes'] = {name: (det_one.buffer(name, 2).shape, det_one.buffer(name, 2).ld, det_head.buffer(name, 2).shape, det_head.buffer(name, 2).ld)
                       for name in ('pooled', 'fc', 'cls_reg', 'pool_index')}
        r['one_shapes'] = {name: (det_one.buffer(name, 2).shape, det_one.buffer(name, 2).ld) for name in ('proposals', 'head_rois', 'head_boxes')}
        r['memory'] = (det_one.memory()['allocated_bytes'], det_head.memory()['allocated_bytes'])
        opt = train.MomentumOptimizer(det_one, MOMENTUM, WEIGHT_DECAY, reach='all')

        # ---- the real chain on the one detector
        seen = {}
        with det_one.scope():
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
            M.entry_flow_train()
            mid = M.middle_flow_train()
            out_t = M.exit_flow_train()
            cls, box = M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
            obj, rb = M.rpn_decode(cls, box)
            props = M.get_proposals(obj, rb, None, PRE, R, NMS, MIN_SIZE, False, 'channels_first')
            for n in range(2):                     # boxes the proposals can match: some of the forward's own
                gboxes[n][0] = props[n, 0]
                gboxes[n][-1] = props[n, 5]

            def encode_fn(rois):
                seen['rois'] = rois
                return enc.ext_encode_rois(rois, glabels, gboxes, P, 0.25, 0.1, seed=4, keep_device=True)

            def encode_host(rois):
                return enc.ext_encode_rois(rois, glabels, gboxes, P, 0.25, 0.1, seed=4)
            d_r, d_t, d_l, d_s = M.get_proposals(obj, rb, encode_fn, PRE, R, NMS, MIN_SIZE, True, 'channels_first')
            r['handed_over'] = [type(x).__name__ for x in (seen['rois'], d_r, d_t, d_l, d_s)]
            r['device_shapes'] = [(x.shape, x.ld) for x in (d_r, d_t, d_l, d_s)]
            feat = M.large_sep_kernel(out_t, MID, CO, True, 'channels_first', 'large_sep_feature')
            r['one'], head = head_pass(det_one, feat, d_r, d_l, d_t, 2)
            r['head_rois_buffer'] = bits(det_one.buffer('head_rois', 2).numpy())
            r['proposals_after'] = bits(det_one.flat('proposals', (2, R, 4)))
            det_one.stream.synchronize()
            sampled = (d_r.numpy().reshape(2, P, 4), d_t.numpy().reshape(2, P, 4), to_host(d_l.ptr, (2, P), np.int32),
                       d_s.numpy().reshape(2, P))
            r['props'], r['sampled'], r['gt'] = props, sampled, (glabels, gboxes)
            feat_host = r['feat_host'] = feat.numpy()
            # the ROIs as the buffer itself: no copy, the same bits
            r['one_in_place'], _ = head_pass(det_one, feat, det_one.buffer('head_rois', 2), d_l, d_t, 2)
            # ---- the host hand-over on the same detector
            h_r, h_t, h_l, h_s = M.get_proposals(obj, rb, encode_host, PRE, R, NMS, MIN_SIZE, True, 'channels_first')
            r['host_sampled'] = (h_r, h_t, h_l, h_s)
            r['one_host'], _ = head_pass(det_one, feat, h_r, h_l, h_t, 2)
            # ---- the other backwards of the step (the head's: the device pass above)
            lsep = M.large_sep_backward(head['feat'], weight_grads='device')
            res = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5, keep_device=True)
            rpn = M.rpn_backward(res, weight_grads='device')
            ef = M.exit_flow_backward(lsep['out'], rpn['mid'], weight_grads='device')
            mf = M.middle_flow_backward(ef['mid'], weight_grads='device')
            en = M.entry_flow_backward(mf['entry'], weight_grads='device')
        grads = weight_gradients(dict(zip(SECTIONS, (head, lsep, rpn, ef, mf, en))), opt.variables)
        r['grads_missing'] = [v for v in opt.variables if v not in grads]
        r['chain_seconds'] = time.time() - t0

        # ---- the two-detector arrangement: det_head fed the downloaded feat and the sampled set as host arrays
        with det_head.scope():
            r['head'], _ = head_pass(det_head, feat_host, sampled[0], sampled[2], sampled[1], 2)
            # the default detector's eval head on the same ROIs (the path this change leaves alone)
            c, g = M.get_head(feat_host, None, 7, 7, None, sampled[0], NC, False, False, 0, 'channels_first', 'final_head')
            r['head_eval'] = bits(np.concatenate([c, g], -1))
            r['refuse_buffer'] = refusal(lambda: det_head.buffer('head_rois', 1))

        # ---- a batch below max_batch: image k alone, its ROIs handed over on the device
        r['single'] = {}
        with det_one.scope():
            for k in (0, 1):
                buf = to_device(np.ascontiguousarray(sampled[0][k:k + 1]))
                rois_k = DeviceTensor(buf.ptr, (1, P, 1, 4), 4, owner=buf)
                loss_func = L.HeadLoss(sampled[2][k:k + 1], sampled[1][k:k + 1], 0.25)
                M.get_head(feat_host[k:k + 1], None, 7, 7, loss_func, rois_k, NC, True, True, OHEM, 'channels_first', 'final_head')
                r['single'][k] = {name: bits(det_one.buffer(name, 1).numpy()) for name in ('pooled', 'cls_reg', 'pool_index')}

            # ---- refusals on the built detectors
            loss63 = L.HeadLoss(sampled[2][:, :63], sampled[1][:, :63], 0.25)
            r['refuse_63'] = refusal(lambda: M.get_head(feat_host, None, 7, 7, loss63, sampled[0][:, :63], NC, True, True, OHEM, 'channels_first', 'final_head'))
            r['refuse_eval_head'] = refusal(lambda: M.get_head(feat_host, None, 7, 7, None, sampled[0], NC, False, False, 0, 'channels_first', 'final_head'))
            bad = DeviceTensor(d_t.ptr, (2, P, 1, 4), 8, owner=d_t)
            r['refuse_ld'] = refusal(lambda: M.get_head(feat_host, None, 7, 7, L.HeadLoss(sampled[2], sampled[1], 0.25), bad, NC, True, True, OHEM,
                                                        'channels_first', 'final_head'))
        s = det_one.stream.handle
        r['refuse_c'] = {}
        for what, call in (('head_decode', lambda: lib().xdet_net_head_decode(det_one.handle, 2, s)),
                           ('bboxes_eval', lambda: lib().xdet_net_bboxes_eval(det_one.handle, 2, None, None, det_one._det_scores.ptr, det_one._det_boxes.ptr, s)),
                           ('set_option', lambda: lib().xdet_net_set_option(det_one.handle, b'head_rois', b'32')),
                           ('calibrate', lambda: lib().xdet_net_calibrate(det_one.handle, det_one._images.ptr, 2, None, s)),
                           ('forward_graph', lambda: lib().xdet_net_forward(det_one.handle, det_one._images.ptr, 2, None, None, det_one._det_scores.ptr,
                                                                            det_one._det_boxes.ptr, 1, s))):
            rc = call()
            r['refuse_c'][what] = (rc, lib().xdet_last_error().decode())
        r['graphs'] = det_one.graph_count()

        # ---- one step on the one detector, then the head against a detector built from the exported weights
        r['info'] = opt.step(grads, LR)
        exported = opt.export_weights(lh_weights)
        r['moved'] = [v for v in train.HEAD_VARIABLES if not np.array_equal(exported[v], np.asarray(lh_weights[v], f32))]
        with det_one.scope():
            r['stale'] = refusal(lambda: M.head_backward(head['loss_func'], to_feat=True))
            r['one_stepped'], _ = head_pass(det_one, feat_host, sampled[0], sampled[2], sampled[1], 2)
        t1 = time.time()
        det_new = LightHeadDetector(exported, **one)
        with det_new.scope():
            r['new_stepped'], _ = head_pass(det_new, feat_host, sampled[0], sampled[2], sampled[1], 2)
        r['new_seconds'] = time.time() - t1
        del det_new

        # ---- the eval entries (each drops the training stages' saved state: last)
        r['refuse_forward'] = refusal(lambda: det_one.forward(images))
        r['refuse_calibrate'] = refusal(lambda: det_one.calibrate(images))
        u8 = (np.arange(S * S * 3) % 251).astype(np.uint8).reshape(S, S, 3)
        r['refuse_detect'] = refusal(lambda: det_one.detect_images([u8, u8]))
        r['refuse_detect_eager'] = refusal(lambda: det_one.detect_images([u8], use_graph=False))
        r['graphs_end'] = det_one.graph_count()
        r['det_one'], r['det_head'] = det_one, det_head
    finally:
        set_precision(before)
    a1, a2 = r['memory']
    print('fixture: %.1f s (two detectors built in %.1f s, the chain done at %.1f s, the detector from the exported weights %.1f s); '
          'allocated by the net: det_one %.1f MiB, det_head %.1f MiB' % (time.time() - t0, r['build_seconds'], r['chain_seconds'],
                                                                          r['new_seconds'], a1 / 2 ** 20, a2 / 2 ** 20))
    return r


def test_the_head_stage_is_planned_on_the_sampled_rows(run):
    assert run['head_R'] == (P, R, P, P, P, None)
    for name, (s1, ld1, s2, ld2) in run['shapes'].items():
        assert s1 == s2 and ld1 == ld2 and s1[:3] == (2, P, 1), (name, s1, s2)
    assert run['one_shapes'] == {'proposals': ((2, R, 1, 4), 4), 'head_rois': ((2, P, 1, 4), 4), 'head_boxes': ((2, R, 1, 4), 4)}


def test_sampled_set_equals_the_host_statement(run):
    from xdet import targets as T
    assert run['handed_over'] == ['DeviceTensor'] * 5
    assert run['device_shapes'] == [((2, P, 1, 4), 4), ((2, P, 1, 4), 4), ((2, P, 1, 1), 1), ((2, P, 1, 1), 1)]
    rois, targets, labels, scores = run['sampled']
    w = T.host_encode_rois(run['props'], *run['gt'], rois_per_image=P, seed=4, **ROI)
    assert np.array_equal(bits(rois), bits(w[0])) and np.array_equal(labels, w[2]) and np.array_equal(bits(scores), bits(w[3]))
    assert_targets(targets, w[1], 'sampled on the device')
    assert labels.dtype == np.int32 and (labels > 0).any()
    # the hand-over put exactly these ROIs into the head's buffer and left the proposal stage's alone
    assert np.array_equal(run['head_rois_buffer'].reshape(2, P, 4), bits(rois))
    assert np.array_equal(run['proposals_after'], bits(run['props']))


def test_the_chain_ran_and_selected(run):
    one = run['one']
    assert one['cls_reg'].shape == (2, P, 1, NC + 4) and one['loss/select'].shape == (2, OHEM)
    assert np.isfinite(one['loss/losses'].view(f32)).all() and one['loss/losses'].view(f32)[0] > 0
    for k in HEAD_GRADS + ['pooled', 'fc', 'feat']:
        assert one[k].view(f32).any(), k
    assert one['feat'].shape == run['feat_host'].shape
    assert run['grads_missing'] == []


def test_equal_bits_with_the_two_detector_arrangement(run):
    assert set(run['one']) == set(run['head'])
    assert differing(run['one'], run['head']) == []


def test_device_and_host_hand_over_agree(run):
    h_r, h_t, h_l, h_s = run['host_sampled']
    rois, targets, labels, scores = run['sampled']
    assert h_l.dtype == np.int64 and np.array_equal(h_l, labels)
    for a, b in ((h_r, rois), (h_t, targets), (h_s, scores)):
        assert np.array_equal(bits(a), bits(b))
    assert differing(run['one_host'], run['one']) == []
    assert differing(run['one_in_place'], run['one']) == []


@pytest.mark.parametrize('k', [0, 1])
def test_batch_below_max_batch(run, k):
    got = run['single'][k]
    for name, full in (('pooled', 'fwd/pooled'), ('cls_reg', 'cls_reg'), ('pool_index', 'fwd/pool_index')):
        assert got[name].shape[0] == 1 and np.array_equal(got[name][0], run['one'][full][k]), (name, k)
    assert not np.array_equal(run['one']['cls_reg'][0], run['one']['cls_reg'][1])


def test_step_on_the_one_detector(run):
    """the whole comparison of the issue: after one step at reach='all' the head of det_one -- forward, loss and backward on the
    kept `feat` and sampled set -- equals that of a detector built from opt.export_weights with the same options (the fixture
    prints what building it takes), the step moved every head variable and the logits, and a loss result from before it is
    refused"""
    from xdet import train
    assert run['info']['step'] == 1
    assert run['moved'] == list(train.HEAD_VARIABLES)
    assert run['stale'] and 'MomentumOptimizer.step has run since' in run['stale'][2]
    assert differing(run['one_stepped'], run['new_stepped']) == []
    assert not np.array_equal(run['one_stepped']['cls_reg'], run['one']['cls_reg'])


def test_default_detector_unchanged(run):
    """det_head has no head_rois: its training head and its eval head, the path this change leaves alone, give the same cls_reg"""
    assert np.array_equal(run['head_eval'].reshape(run['head']['cls_reg'].shape), run['head']['cls_reg'])


def test_refusals_of_the_option(run):
    for v, got in run['ctor'].items():
        assert got and got[0] == 'InvalidArgumentError' and 'head_rois must be None (off) or a whole number in 1..rpn_post_nms_top_n (1800), got' in got[2], (v, got)
    for v in (b'0', str(R + 1).encode(), b'x', b'', b'64x', b'-3'):
        rc, msg = run['option'][v]
        assert rc == -1 and 'head_rois must be off or a whole number in 1..rpn_post_nms_top_n (1800), got ' + v.decode() in msg, (v, rc, msg)
    for v in (b'off', b'64', b'1', str(R).encode()):
        assert run['option'][v][0] == 0, (v, run['option'][v])


def test_refusals_of_get_head(run):
    name, code, msg = run['refuse_63']
    assert name == 'InvalidArgumentError' and 'get_head: 63 ROIs per image but the detector was built with head_rois = 64' in msg
    name, code, msg = run['refuse_eval_head']
    assert name == 'InvalidArgumentError' and 'get_head: is_training=False on a detector built with head_rois=64' in msg
    name, code, msg = run['refuse_ld']
    assert name == 'InvalidArgumentError' and 'get_head: device ROIs must be dense corner boxes [N,64,(1,)4] (ld 4)' in msg


def test_refusals_of_the_eval_entries(run):
    sentence = 'this net was built with the option head_rois=64'
    for what, door in (('refuse_forward', 'net_forward:'), ('refuse_calibrate', 'net_calibrate:'), ('refuse_detect', 'net_forward_u8:'),
                       ('refuse_detect_eager', 'net_forward_u8:')):
        name, code, msg = run[what]
        assert name == 'XdetError' and code == -3 and door in msg and sentence in msg, (what, run[what])
    c = run['refuse_c']
    for what, door in (('head_decode', 'net_head_decode:'), ('bboxes_eval', 'net_bboxes_eval:'), ('calibrate', 'net_calibrate:'),
                       ('forward_graph', 'net_forward:')):
        assert c[what][0] == -3 and door in c[what][1] and sentence in c[what][1], (what, c[what])
    assert c['set_option'][0] == -1 and 'the net is already built' in c['set_option'][1]
    assert run['graphs'] == 0 and run['graphs_end'] == 0          # refused ahead of a capture


def test_the_default_net_refuses_the_buffer(run):
    name, code, msg = run['refuse_buffer']
    assert name == 'InvalidArgumentError' and 'net_buffer: head_rois needs a net built with the option head_rois=<P>' in msg
