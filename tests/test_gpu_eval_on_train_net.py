"""The detector that trains also evaluates: the eval forward of a net with 1800 proposals (bboxes_eval's wide form) and of a
training detector built with head_rois=64, eval_head=True (a second head stage on the shared dense layers).

One module fixture, sized as tests/test_gpu_sampled_head.py (S = 256, max_batch 2, rpn_pre_nms_top_n 5000, 1800 proposals, 64
sampled ROIs, the TRAIN flags, f16x3) with stem_train=True as tests/test_gpu_train_step_driver.py, and large_sep='direct' so
that MomentumOptimizer(reach='all').refresh_eval_net() reaches the large-separable block without further options.  It builds
  plain   no head_rois, no training flags: the reference point of every eval forward,
  det     the training detector with eval_head=True, its optimizer and its TrainStep,
  twin    the same without eval_head, stepped alongside,
  fresh   a plain detector from det's exported weights after one step,
runs everything once, and the tests read what it recorded.  Every comparison is for equal bits.

select_threshold is the default 0.01: with the synthetic weights a class has between 84 and 1768 of an image's 1800 ROIs above
it (printed by the fixture, `-s`; measured on an MI355X), several classes more than 1024 (asserted for the largest): the wide
kernel counts ranks, sorts 1024 slots and sorts 2048 slots in one forward."""
import ctypes
import time

import numpy as np
import pytest

import target_cases as C

from flow_train_cases import S, NC, bits
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_train_step_driver import R, PRE, P, LR, MOMENTUM, WEIGHT_DECAY, STEP_ARGS, SCALARS, differing, scalar_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = ('pooled_eval', 'fc_eval', 'cls_reg_eval')
TRAIN_HEAD = ('pooled', 'fc', 'cls_reg', 'pool_index', 'head_rois')


def refusal(call):
    import xdet
    try:
        call()
        return None
    except xdet.XdetError as e:
        return (type(e).__name__, e.code, str(e))


def dets_bits(dets):
    """forward()'s list of {class: (scores, boxes)} -> (scores bits [n, 20, topk], boxes bits [n, 20, topk, 4])"""
    return (bits(np.stack([np.stack([d[c][0] for c in sorted(d)]) for d in dets])),
            bits(np.stack([np.stack([d[c][1] for c in sorted(d)]) for d in dets])))


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope='module')
def run(lh_weights):
    from xdet import model as M, ops, targets as T, train, weights as W
    from xdet._lib import lib, LightHeadConfig
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision, to_host
    t0 = time.time()
    r = {}
    images = W.synthetic_images(2, S, seed=3)
    anchors = C.anchors(S)
    glabels, gboxes = C.make_ground_truth(61, 2, anchors)
    enc_a, enc_b = (T.AnchorEncoder([anchors], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.) for _ in range(2))
    sizes = dict(image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R, large_sep='direct')
    flags = dict(TRAIN, stem_train=True, head_rois=P, **sizes)
    before = get_precision()
    set_precision('f16x3')
    try:
        # ---- the plain 1800-proposal detector: eager, graph, and its tail through the op-level doors
        plain = LightHeadDetector(lh_weights, **sizes)
        r['plain'] = dets_bits(plain.forward(images))
        proposals = plain.flat('proposals', (2, R, 4))
        t = plain.buffer('cls_reg', 2)
        cls_reg = to_host(t.ptr, (2 * R, t.ld))
        r['plain_head_boxes'] = bits(plain.flat('head_boxes', (2 * R, 4)))
        r['plain_graph'] = dets_bits(plain.forward(images, use_graph=True))
        r['plain_graphs'] = plain.graph_count()
        boxes, probs, bad = ops.head_decode_probs(proposals, cls_reg, NC, R)
        r['op_boxes'], r['op_bad'] = bits(boxes), bad.tolist()
        r['op'] = dets_bits(ops.bboxes_eval_from_probs(probs, boxes, (S, S), train_image_size=S, bad=bad, wide=True))
        r['above'] = (probs[:, 1:] > f32(0.01)).sum(-1)                  # [2, 20] ROIs above select_threshold
        r['proposal_rows'] = [int((np.abs(proposals[i]).sum(-1) > 0).sum()) for i in range(2)]
        r['narrow_refuses'] = refusal(lambda: ops.bboxes_eval_from_probs(probs, boxes, (S, S), train_image_size=S, bad=bad))
        r['plain_buffer'] = {n: refusal(lambda: plain.buffer(n, 1)) for n in NAMES}
        r['memory_plain'] = plain.memory()

        # ---- the training detector with the eval head, and its twin without
        det, twin = LightHeadDetector(lh_weights, eval_head=True, **flags), LightHeadDetector(lh_weights, **flags)
        r['memory'] = (det.memory(), twin.memory())
        opt, opt_twin = (train.MomentumOptimizer(d, MOMENTUM, WEIGHT_DECAY, reach='all') for d in (det, twin))
        ts, ts_twin = train.TrainStep(det, opt, enc_a, **STEP_ARGS), train.TrainStep(twin, opt_twin, enc_b, **STEP_ARGS)
        r['build_seconds'] = time.time() - t0
        r['twin_buffer'] = {n: refusal(lambda: twin.buffer(n, 1)) for n in NAMES}
        r['twin_forward'] = refusal(lambda: twin.forward(images))
        r['eval'] = dets_bits(det.forward(images))
        r['eval_graph'] = dets_bits(det.forward(images, use_graph=True))
        r['eval_shapes'] = {n: (tuple(det.buffer(n, 2).shape), tuple(plain.buffer(n[:-5], 2).shape)) for n in NAMES}
        r['eval_cls_reg'] = (bits(det.buffer('cls_reg_eval', 2).numpy()), bits(plain.buffer('cls_reg', 2).numpy()))
        r['eval_one'] = dets_bits(det.forward(images[:1]))
        r['eval_one_graph'] = dets_bits(det.forward(images[:1], use_graph=True))

        # ---- refusals that stay, each by its sentence (C doors: return code and xdet_last_error)
        s = det.stream.handle
        r['refuse_c'] = {}
        for what, call in (('head_decode', lambda: lib().xdet_net_head_decode(det.handle, 2, s)),
                           ('bboxes_eval', lambda: lib().xdet_net_bboxes_eval(det.handle, 2, None, None, det._det_scores.ptr, det._det_boxes.ptr, s)),
                           ('calibrate', lambda: lib().xdet_net_calibrate(det.handle, det._images.ptr, 2, None, s))):
            rc = call()
            r['refuse_c'][what] = (rc, lib().xdet_last_error().decode())
        r['refuse_calibrate'] = refusal(lambda: det.calibrate(images))
        with det.scope():
            r['refuse_get_head'] = refusal(lambda: M.get_head(None, None, 7, 7, None, np.zeros((2, P, 4), f32), NC, False, False, 0,
                                                              'channels_first', 'final_head'))
        cfg = LightHeadConfig(image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R)
        h = ctypes.c_void_p()
        assert lib().xdet_net_create(ctypes.byref(h), ctypes.byref(cfg)) == 0
        r['option'] = {v: lib().xdet_net_set_option(h, b'eval_head', v) for v in (b'on', b'off', b'yes', b'')}
        assert lib().xdet_net_set_option(h, b'eval_head', b'on') == 0
        r['build_without_head_rois'] = (lib().xdet_net_build(h), lib().xdet_last_error().decode())
        assert lib().xdet_net_destroy(h) == 0

        # ---- saved state: a training forward, then an eval forward on the same detector
        with det.scope():
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
            M.stem_train()
            M.entry_flow_train()
            M.middle_flow_train()
            M.exit_flow_train()
        r['saved_before'] = sorted(det.exit_flow_saved())[:1]
        det.forward(images)
        r['saved_after'] = refusal(det.exit_flow_saved)
        with det.scope():
            r['backward_after'] = refusal(lambda: M.exit_flow_backward(None))

        # ---- one step on both: the option changes nothing in training; the eval forward left the sampled-row buffers alone
        r['start_equal'] = differing(opt.read(), opt_twin.read())
        got = ts.step(images, glabels, gboxes, None, LR, seed=7).read()
        want = ts_twin.step(images, glabels, gboxes, None, LR, seed=7).read()
        r['step'] = (got, want)
        r['state'] = differing(opt.read(), opt_twin.read())
        r['n_state'] = len(opt.read())
        r['variables'] = opt.variables
        head_before = {n: bits(det.buffer(n, 2).numpy()) for n in TRAIN_HEAD}
        r['head_vs_twin'] = [n for n in TRAIN_HEAD if not np.array_equal(head_before[n], bits(twin.buffer(n, 2).numpy()))]

        # ---- train, refresh, score: against a fresh plain detector from the exported weights
        r['stale'] = dets_bits(det.forward(images))                     # (the body still folded from the old weights)
        r['layers'] = opt.refresh_eval_net()
        r['refreshed'] = dets_bits(det.forward(images))
        r['refreshed_graph'] = dets_bits(det.forward(images, use_graph=True))
        r['head_untouched'] = [n for n in TRAIN_HEAD if not np.array_equal(head_before[n], bits(det.buffer(n, 2).numpy()))]
        exported = opt.export_weights(lh_weights)
        fresh = LightHeadDetector(exported, **sizes)
        r['fresh'] = dets_bits(fresh.forward(images))
        u8 = (np.arange(S * S * 3) % 251).astype(np.uint8).reshape(S, S, 3)
        gt = (np.array([1, 7]), np.array([[0.1, 0.1, 0.6, 0.6], [0.3, 0.2, 0.9, 0.8]], f32), np.array([0, 0]))
        r['detect'] = (dets_bits(det.detect_images([u8, u8[::-1].copy()])), dets_bits(fresh.detect_images([u8, u8[::-1].copy()])))
        acc = det.evaluate_images([u8, u8[::-1].copy()], [gt, gt])
        r['records'] = acc.records()
        r['graphs'] = det.graph_count()
    finally:
        set_precision(before)
    print('fixture: %.1f s (three detectors, two optimizers built in %.1f s); ROIs above select_threshold per class: %d .. %d; '
          'non-zero proposals per image %s; positive scores: plain %d, after the step %d'
          % (time.time() - t0, r['build_seconds'], r['above'].min(), r['above'].max(), r['proposal_rows'],
             int((r['plain'][0].view(f32) > 0).sum()), int((r['refreshed'][0].view(f32) > 0).sum())))
    print('xdet_net_memory: plain %.1f MiB; training detector with eval_head %.1f MiB, without %.1f MiB'
          % (r['memory_plain']['allocated_bytes'] / 2.0 ** 20, r['memory'][0]['allocated_bytes'] / 2.0 ** 20,
             r['memory'][1]['allocated_bytes'] / 2.0 ** 20))
    return r


def test_plain_1800_detector_runs_eager_and_captured(run):
    assert run['plain'][0].shape == (2, NC - 1, 200) and same(run['plain'], run['plain_graph']) and run['plain_graphs'] == 1
    scores = run['plain'][0].view(f32)
    assert np.isfinite(scores).all() and (scores > 0).sum() > 0


def test_plain_1800_detector_equals_the_entry_points(run):
    """its detections == ops.head_decode_probs + ops.bboxes_eval_from_probs(..., wide=True) on its own proposals and cls_reg,
    and at least one class has more than 1024 ROIs above select_threshold: the wide kernel, with more keys than the narrow
    one holds.  The narrow door refuses the same call."""
    assert run['op_bad'] == [0, 0] and np.array_equal(run['op_boxes'], run['plain_head_boxes'])
    assert same(run['op'], run['plain'])
    assert run['above'].max() > 1024, run['above']
    name, code, msg = run['narrow_refuses']
    assert name == 'InvalidArgumentError' and '1 <= rois per image <= 1024' in msg


def test_eval_head_forward_equals_the_plain_detector(run):
    assert same(run['eval'], run['plain']) and same(run['eval_graph'], run['plain'])
    for n, (got, want) in run['eval_shapes'].items():
        assert got == want and got[1] == R, (n, got, want)
    assert np.array_equal(*run['eval_cls_reg'])


def test_a_batch_of_one_equals_row_0_of_the_batch_of_two(run):
    for one in (run['eval_one'], run['eval_one_graph']):
        assert one[0].shape[0] == 1 and np.array_equal(one[0][0], run['eval'][0][0]) and np.array_equal(one[1][0], run['eval'][1][0])


def test_train_refresh_and_score_on_one_detector(run):
    """after one TrainStep.step and refresh_eval_net(): forward == a fresh plain detector built from export_weights; the step
    moved the detections; detect_images agrees too and evaluate_images runs"""
    assert run['layers'] == 76
    assert same(run['refreshed'], run['fresh']) and same(run['refreshed_graph'], run['fresh'])
    assert not same(run['refreshed'], run['plain']) and not same(run['stale'], run['refreshed'])
    assert same(*run['detect'])
    assert isinstance(run['records'], dict) and run['graphs'] >= 2


def test_eval_head_changes_nothing_in_training(run):
    """one TrainStep.step on the detector with the option == its twin without: the seven scalars and all 176 masters and
    momentum slots; and an eval forward leaves pooled, fc, cls_reg, pool_index and head_rois as the step left them"""
    got, want = run['step']
    assert run['start_equal'] == [] and got['skipped'] is False and want['skipped'] is False
    assert scalar_bits(got) == scalar_bits(want), {n: (got[n], want[n]) for n in SCALARS}
    assert all(np.isfinite(got[n]) for n in SCALARS) and got['head_ce_loss'] > 0
    assert run['state'] == [] and len(run['variables']) == 176 and run['n_state'] >= 2 * 176
    assert run['head_vs_twin'] == [] and run['head_untouched'] == []


def test_an_eval_forward_drops_the_saved_state(run):
    assert run['saved_before']
    for what, word in (('saved_after', 'exit_flow_saved'), ('backward_after', 'exit_flow_backward')):
        name, code, msg = run[what]
        assert name == 'InvalidArgumentError' and word in msg and 'exit_flow_train' in msg, run[what]


def test_refusals_that_stay(run):
    both = 'this net was built with the options head_rois=64 and eval_head=on'
    c = run['refuse_c']
    for what, door in (('head_decode', 'net_head_decode:'), ('bboxes_eval', 'net_bboxes_eval:'), ('calibrate', 'net_calibrate:')):
        assert c[what][0] == -3 and door in c[what][1] and both in c[what][1], (what, c[what])
    assert 'stage entry of the logits form' in c['head_decode'][1] and 'stage entry of the logits form' in c['bboxes_eval'][1]
    assert 'exponent 0' in c['calibrate'][1] and 'pre-scale' in c['calibrate'][1]
    name, code, msg = run['refuse_calibrate']
    assert name == 'XdetError' and code == -3 and 'net_calibrate:' in msg and both in msg
    name, code, msg = run['refuse_get_head']
    assert name == 'InvalidArgumentError' and 'get_head: is_training=False on a detector built with head_rois=64' in msg
    # the twin, built without eval_head, refuses as ever
    name, code, msg = run['twin_forward']
    assert name == 'XdetError' and code == -3 and 'this net was built with the option head_rois=64' in msg and 'no eval forward' in msg


def test_refusals_of_the_option_and_the_buffers(run):
    assert run['option'] == {b'on': 0, b'off': 0, b'yes': -1, b'': -1}
    rc, msg = run['build_without_head_rois']
    assert rc == -1 and 'eval_head=on needs the option head_rois=<P>' in msg
    for where in ('plain_buffer', 'twin_buffer'):
        for n in NAMES:
            name, code, msg = run[where][n]
            assert name == 'InvalidArgumentError' and 'net_buffer: %s needs a net built with the options head_rois=<P> and eval_head=on' % n in msg
