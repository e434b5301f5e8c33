"""train.TrainStep(..., clip_norm=c) on the GPU: the one-call step with the gradients clipped to a global norm inside the momentum
step.  One module fixture, sized as tests/test_gpu_train_step_driver.py (S = 256, max_batch 2, 176 variables), builds two
detectors from the same weights and runs two steps:
  1. `a` with clip_norm far above the norm, `b` with clip_norm=None, on the same batch: the same bits everywhere;
  2. `a` with clip_norm below the step's own norm; on `b` the chain made by hand, up to the gradients, which are downloaded and
     put through the NumPy statement (host_grad_sq, host_clip_scale, host_momentum_step(..., scale=)) from b's state -- equal
     to a's before the step -- : a's variables and momentum must hold the statement's bits."""
import time

import numpy as np
import pytest

import target_cases as C

from flow_train_cases import S, bits
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_train_step_driver import (hand_chain, differing, scalar_bits, STEP_ARGS, SCALARS, R, PRE, P, LR, MOMENTUM, WEIGHT_DECAY)

pytestmark = pytest.mark.gpu
f32 = np.float32
FAR = 1e9


def host_clipped_step(state, grads, variables, decayed, clip_norm, lr=LR):
    """the NumPy statement of a clipped step over `variables` -> (the state afterwards, the scale, grad_sq)"""
    from xdet import host_clip_scale, host_grad_sq, host_momentum_step
    sq = host_grad_sq([grads[v] for v in variables])
    scale = host_clip_scale(sq, clip_norm)
    out = {}
    for v in variables:
        out[v], out[v + '/Momentum'] = host_momentum_step(state[v], grads[v], state[v + '/Momentum'], lr, MOMENTUM, WEIGHT_DECAY,
                                                          decayed[v], scale=scale)
    return out, scale, sq


@pytest.fixture(scope='module')
def run(lh_weights):
    from xdet import targets as T, train, weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    t0 = time.time()
    r = {}
    anchors = C.anchors(S)
    enc_a, enc_b = (T.AnchorEncoder([anchors], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.) for _ in range(2))
    batches = []
    for k in range(2):
        gl, gb = C.make_ground_truth(71 + k, 2, anchors)
        batches.append([W.synthetic_images(2, S, seed=13 + k), gl, gb])
    flags = dict(TRAIN, stem_train=True, image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R, head_rois=P)
    before = get_precision()
    set_precision('f16x3')
    try:
        det_a, det_b = LightHeadDetector(lh_weights, **flags), LightHeadDetector(lh_weights, **flags)
        opt_a, opt_b = (train.MomentumOptimizer(d, MOMENTUM, WEIGHT_DECAY, reach='all') for d in (det_a, det_b))
        r['variables'] = opt_a.variables
        # ---- 1. far above the norm against clip_norm=None
        images, gl, gb = batches[0]
        r['far'] = train.TrainStep(det_a, opt_a, enc_a, clip_norm=FAR, **STEP_ARGS).step(images, gl, gb, None, LR, seed=21).read()
        r['none'] = train.TrainStep(det_b, opt_b, enc_b, **STEP_ARGS).step(images, gl, gb, None, LR, seed=21).read()
        state = opt_b.read()
        r['far_state'] = differing(opt_a.read(), state)
        r['far_moving'] = differing(opt_a.export_weights({}), opt_b.export_weights({}))
        # ---- 2. below the norm against the hand-made chain and the statement
        images, gl, gb = batches[1]
        r['clip'] = clip = 0.1 * r['none']['grad_norm']
        r['clipped'] = train.TrainStep(det_a, opt_a, enc_a, clip_norm=clip, **STEP_ARGS).step(images, gl, gb, None, LR, seed=22).read()
        scalars, grads, _ = hand_chain(det_b, enc_b, images, gl, gb, 22, opt_b.variables)
        host_grads = {v: grads[v].numpy() for v in opt_b.variables}
        want, r['scale'], r['grad_sq'] = host_clipped_step(state, host_grads, opt_b.variables, opt_b._decayed, clip)
        r['clipped_state'] = differing(opt_a.read(), want)
        r['unclipped_moved'] = len(differing(want, state))
        r['hand_scalars'] = scalars
        # ---- 3. the optimizer's own door: clip_norm without the guard, on the gradients b's chain left
        r['unguarded'] = opt_b.step(grads, LR, clip_norm=FAR)
    finally:
        set_precision(before)
    print('fixture: %.1f s; grad_norm %.6g then %.6g, clip %.6g, scale %.9g' % (time.time() - t0, r['none']['grad_norm'],
                                                                               r['clipped']['grad_norm'], clip, r['clipped']['clip_scale']))
    return r


def test_a_clip_far_above_the_norm_keeps_the_bits_of_no_clip(run):
    far, none = run['far'], run['none']
    assert scalar_bits(far) == scalar_bits(none) and bits(f32(far['l2']))[0] == bits(f32(none['l2']))[0]
    assert run['far_state'] == [] and run['far_moving'] == []
    assert far['clip_scale'] == 1.0 and far['grad_norm'] == none['grad_norm'] and 0 < far['grad_norm'] < FAR
    assert far['skipped'] is False and far['step'] == none['step'] == 1
    assert 'clip_scale' not in none and set(far) - set(none) == {'clip_scale'}


def test_a_clip_below_the_norm_equals_the_chain_and_the_statement(run):
    got = run['clipped']
    assert run['clip'] < got['grad_norm']                                         # below the step's own norm
    assert run['clipped_state'] == [], (run['clipped_state'][:5], len(run['clipped_state']))   # masters and momentum, 176 variables
    assert run['unclipped_moved'] >= 176                                          # (the statement moves the state: no vacuous equality)
    assert len(run['variables']) == 176
    for k in SCALARS[:6]:                                                         # the losses are the chain's: clipping touches none
        assert bits(f32(got[k]))[0] == bits(f32(run['hand_scalars'][k]))[0], k


def test_read_reports_the_scale_and_the_norm(run):
    got = run['clipped']
    assert bits(f32(got['clip_scale']))[0] == bits(run['scale'])[0] and 0 < got['clip_scale'] < 1
    assert got['grad_norm'] == float(np.sqrt(np.float64(run['grad_sq'])))
    assert abs(got['clip_scale'] - run['clip'] / got['grad_norm']) < 1e-6
    assert got['skipped'] is False and got['first_bad'] is None and got['step'] == 2
    u = run['unguarded']                                                          # no guard: no 'skipped', and grad_norm all the same
    assert set(u) == {'step', 'lr', 'l2', 'grad_norm', 'clip_scale'} and u['clip_scale'] == 1.0 and u['grad_norm'] > 0 and u['step'] == 2
