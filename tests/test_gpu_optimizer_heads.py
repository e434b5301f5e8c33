"""MomentumOptimizer(reach='all') on the detector of the flow tests (S = 256, P = 64, max_batch 2, the TRAIN flags of
tests/test_gpu_entry_flow_backward.py -- rpn_hidden and pool_index among them -- and large_sep='direct'): one full iteration
with weight_grads='device' in all six backwards, one step over the 170 variables, and then everything the step must have
brought in line, each against a detector built afresh from opt.export_weights(): the masters against the host statement, the
training forward, a second backward (a stale backward operand shows here), the eval net after refresh_eval_net(), and the
refusals.  Every comparison is for equal bits: no op of the chain runs a float atomic, and the table repack is the creation
path's own code.  One module fixture runs everything; the tests read what it recorded.

Figures of the run on an MI355X that this file was written against are printed by the fixture (`-s`)."""
import math
import time

import numpy as np
import pytest

from flow_train_cases import S, P, NC, A, MID, CO, bits, head_and_rpn_inputs
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_net_refresh import detections, equal

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
LR, MOMENTUM, WEIGHT_DECAY = 1e-3, 0.9, 2e-4             # (tests/test_gpu_net_refresh.py's rate: the eval net stays in the f16 range)
ALL = dict(TRAIN, large_sep='direct')
SECTIONS = ('head_backward', 'large_sep_backward', 'rpn_backward', 'exit_flow_backward', 'middle_flow_backward', 'entry_flow_backward')
HEADS = SECTIONS[:3]
FROZEN_BY_BN = ('large_sep_feature/Branch_0/conv2d_1/bias', 'large_sep_feature/Branch_1/conv2d_1/bias')


def host(v):
    return v.numpy() if hasattr(v, 'numpy') else np.asarray(v)


def iteration(det, inputs, weight_grads, images=None):
    """one training pass on the current weights (behind an eval body when images are given): the three training flows, the
    large-separable block, the head with OHEM 32 and its loss, the RPN and its loss (seed 5), and the six backwards
    -> what the forward left (bits), both loss results, the six backward dicts"""
    from xdet import model as M, losses as L
    rois, labels, targets, a_l, a_t = inputs
    n = rois.shape[0]
    r = {'fwd': {}}
    with det.scope():
        if images is not None:
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        M.entry_flow_train()
        mid = M.middle_flow_train()
        feat = M.large_sep_kernel(M.exit_flow_train(), MID, CO, True, 'channels_first', 'large_sep_feature')
        loss_func = L.HeadLoss(labels, targets, 0.25)
        M.get_head(feat, None, 7, 7, loss_func, rois, NC, True, True, 32, 'channels_first', 'final_head')
        r['fwd']['feat'], r['fwd']['cls_reg'] = bits(det.buffer('feat', n).numpy()), bits(det.buffer('cls_reg', n).numpy())
        head = M.head_backward(loss_func, to_feat=True, weight_grads=weight_grads)
        lsep = M.large_sep_backward(head['feat'], weight_grads=weight_grads)
        cls, box = M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
        r['fwd']['rpn_out'] = bits(det.buffer('rpn_out', n).numpy())
        res = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5, keep_device=True)
        rpn = M.rpn_backward(res, weight_grads=weight_grads)
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'], weight_grads=weight_grads)
        mf = M.middle_flow_backward(ef['mid'], weight_grads=weight_grads)
        en = M.entry_flow_backward(mf['entry'], weight_grads=weight_grads)
    r['fwd']['head_loss'], r['fwd']['rpn_loss'] = bits(loss_func.result.losses), bits(res.losses)
    r['loss_func'], r['rpn_result'] = loss_func, res
    r['sections'] = dict(zip(SECTIONS, (head, lsep, rpn, ef, mf, en)))
    return r


def weight_gradients(sections, variables):
    g = {}
    for name in SECTIONS:
        g.update({k: v for k, v in sections[name].items() if k in variables})
    return g


def differing(a, b, keys):
    """the keys whose two values do not have the same shape and bits"""
    out = []
    for k in keys:
        x, y = host(a[k]), host(b[k])
        if x.shape != y.shape or not np.array_equal(bits(x.astype(f32, copy=False)), bits(y.astype(f32, copy=False))):
            out.append(k)
    return out


@pytest.fixture(scope='module')
def run(lh_weights):
    import xdet
    from xdet import model as M, train, weights as W
    from xdet._lib import NetWeightDev, lib
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor, get_precision, set_precision
    t0 = time.time()
    r = {'weights': lh_weights}
    images, inputs = W.synthetic_images(2, S, seed=3), head_and_rpn_inputs()
    build = lambda w, **kw: LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **dict(ALL, **kw))
    before = get_precision()
    set_precision('f16x3')
    try:
        det = build(lh_weights)
        opt = train.MomentumOptimizer(det, MOMENTUM, WEIGHT_DECAY, reach='all')
        variables = r['variables'] = opt.variables
        r['read0'] = opt.read()
        # ---- iteration 1 with the weight gradients left on the device everywhere, and (2) the three backwards again at 'host'
        it1 = iteration(det, inputs, 'device', images)
        dev = weight_gradients(it1['sections'], variables)
        r['all_device'] = [v for v in variables if not (isinstance(dev.get(v), DeviceTensor) and dev[v].ld == dev[v].shape[-1])]
        r['grads1'] = {v: host(dev[v]) for v in variables}
        with det.scope():
            head_h = M.head_backward(it1['loss_func'], to_feat=True)
            hosts = {'head_backward': head_h, 'large_sep_backward': M.large_sep_backward(head_h['feat']),
                     'rpn_backward': M.rpn_backward(it1['rpn_result'])}
        r['host_keys'] = {n: (set(hosts[n]), set(it1['sections'][n])) for n in HEADS}
        r['host_types'] = [n + '/' + k for n in HEADS for k in hosts[n] if k in variables and not isinstance(hosts[n][k], np.ndarray)]
        r['host_diff'] = [n + '/' + k for n in HEADS for k in differing(hosts[n], it1['sections'][n], hosts[n])]
        r['host_shapes'] = [n + '/' + k for n in HEADS for k in hosts[n]
                            if k in variables and tuple(it1['sections'][n][k].shape) != np.shape(lh_weights[k])]
        # ---- (1) the step
        t1 = time.time()
        r['info'] = opt.step(dev, LR)
        r['step_seconds'] = time.time() - t1
        r['read1'] = opt.read()
        # ---- (6) a backward on a loss result from before the step; and a loss made again without its forward
        r['stale'] = {}
        with det.scope():
            from xdet import losses as L
            cls, box = det.buffer('rpn_out', 2).channels(0, 2 * A), det.buffer('rpn_out', 2).channels(2 * A, 6 * A)
            again = L.rpn_loss(cls, box, inputs[3], inputs[4], 256, 0.25, seed=5, keep_device=True)
            for what, call in (('head', lambda: M.head_backward(it1['loss_func'], to_feat=True)),
                               ('rpn', lambda: M.rpn_backward(it1['rpn_result'])),
                               ('rpn_loss_again', lambda: M.rpn_backward(again))):
                try:
                    call()
                    r['stale'][what] = None
                except xdet.InvalidArgumentError as e:
                    r['stale'][what] = str(e)
        # ---- (3), (4) the training forward and a second backward, against a detector built from the exported weights
        exported = opt.export_weights(lh_weights)
        r['exported_keys'] = (set(exported), set(lh_weights))
        r['exported_moved'] = [v for v in variables if not np.array_equal(exported[v], np.asarray(lh_weights[v], f32))]
        it2 = iteration(det, inputs, 'device')
        det2 = build(exported)
        ref = iteration(det2, inputs, 'host', images)
        r['fwd_diff'] = equal(it2['fwd'], ref['fwd'], sorted(ref['fwd']))
        r['fwd_moved'] = equal(it2['fwd'], it1['fwd'], sorted(ref['fwd']))
        g2, gref = weight_gradients(it2['sections'], variables), weight_gradients(ref['sections'], variables)
        r['grad_keys'] = (set(g2), set(gref))
        r['grad_diff'] = differing(g2, gref, variables)
        r['dx_diff'] = [n + '/' + k for n, k in (('large_sep_backward', 'out'), ('rpn_backward', 'mid'), ('exit_flow_backward', 'mid'),
                                                 ('head_backward', 'feat'), ('entry_flow_backward', 'stem'))
                        if differing(it2['sections'][n], ref['sections'][n], [k])]
        # ---- (5) the eval net
        r['eval_stale'] = detections(det, images)
        r['layers'] = opt.refresh_eval_net()
        # (iteration 2 moved the moving statistics once more: the fresh detector is built from what the optimizer exports now)
        r['eval'], r['eval_ref'] = detections(det, images), detections(build(opt.export_weights(lh_weights)), images)
        # ---- (6) the net door's refusals, each with the net's outputs unchanged
        heads = {v: opt._master[v][0] for v in train.RPN_HEAD_VARIABLES + train.HEAD_VARIABLES}
        flow = opt._master['conv2d_4/kernel'][0]
        r['door'] = {}
        for what, rows in (('partial', [n for n in heads if n != 'final_head/fc_loc/bias']),
                           ('duplicate', list(heads) + ['rpn_head/conv2d_1/kernel']),
                           ('flow', list(heads) + ['conv2d_4/kernel']),
                           ('null', None), ('empty', [])):
            if rows is None:
                table, n = (NetWeightDev * 1)(NetWeightDev(b'rpn_head/conv2d/kernel', None)), 1
            else:
                table = (NetWeightDev * max(len(rows), 1))(*[NetWeightDev(n.encode(), heads.get(n, flow).ptr) for n in rows])
                n = len(rows)
            rc = lib().xdet_net_refresh_heads(det.handle, table, n, det.stream.handle)
            r['door'][what] = (rc, lib().xdet_last_error().decode())
        try:
            det.refresh_heads(dict(heads, **{'rpn_head/conv2d/bias': np.zeros(512, f32)}))
            r['door']['host'] = None
        except xdet.InvalidArgumentError as e:
            r['door']['host'] = str(e)
        r['eval_after_refusals'] = detections(det, images)
        # ---- (6) reach='all' without rpn_hidden, and the rest of the constructor's requirements on stubs of the detector
        r['ctor'] = {}
        plain = build(lh_weights, rpn_hidden=False, middle_flow_train=False, entry_flow_train=False)
        for what, d in (('rpn_hidden', plain), ('reach', det)):
            try:
                train.MomentumOptimizer(d, reach='all' if what != 'reach' else 'heads')
                r['ctor'][what] = None
            except xdet.InvalidArgumentError as e:
                r['ctor'][what] = str(e)
        del plain
        # ---- (6) a spectral block: refresh_eval_net is refused by name ahead of any launch
        sp = build(lh_weights, large_sep='spectral')
        sp_opt = train.MomentumOptimizer(sp, MOMENTUM, WEIGHT_DECAY, reach='all')
        r['sp_before'] = detections(sp, images)
        try:
            sp_opt.refresh_eval_net()
            r['sp_error'] = None
        except xdet.InvalidArgumentError as e:
            r['sp_error'] = str(e)
        r['sp_after'] = detections(sp, images)
    finally:
        set_precision(before)
    print('fixture: %.1f s; the step at reach=\'all\' took %.1f ms (its first call allocates the net door\'s scratch)'
          % (time.time() - t0, 1e3 * r['step_seconds']))
    return r


def test_the_variables_and_their_start(run):
    from xdet import train
    v = run['variables']
    assert v == train.optimizer_variables((True,) * 4, 'all') and len(v) == 170 and len(set(v)) == 170
    for name in v:                                      # the masters start as the checkpoint's values, the slots at zero
        want = np.asarray(run['weights'][name], f32)
        assert run['read0'][name].shape == want.shape and np.array_equal(bits(run['read0'][name]), bits(want)), name
        assert not run['read0'][name + '/Momentum'].any(), name


def test_1_the_step_equals_the_host_statement(run):
    from xdet import host_momentum_step
    from xdet.train import decayed
    v = run['variables']
    assert run['all_device'] == []
    start = {name: np.asarray(run['weights'][name], f32) for name in v}
    moved = []
    for name in v:
        var, acc = host_momentum_step(start[name], run['grads1'][name], np.zeros_like(start[name]), LR, MOMENTUM, WEIGHT_DECAY, decayed(name))
        for key, want in ((name, var), (name + '/Momentum', acc)):
            got = run['read1'][key]
            assert got.shape == want.shape and got.dtype == f32, key
            assert np.array_equal(bits(got), bits(want)), (key, int((bits(got) != bits(want)).sum()), got.size)
        if not np.array_equal(run['read1'][name], start[name]):
            moved.append(name)
    # (the two conv2d_1 biases of the large-separable block sit in front of a training-mode batch norm: their gradient is the
    #  rounding of zero, and only the L2 term moves them)
    assert set(v) - set(moved) <= set(FROZEN_BY_BN), sorted(set(v) - set(moved))
    info = run['info']
    assert set(info) == {'step', 'lr', 'l2'} and info['step'] == 1 and info['lr'] == LR
    # include/xdet.h: a term passes through at most 1 + 2 + 2 + 8 + ceil(log2(C)) roundings, C the chunks of 4096 elements
    chunks = sum(-(-start[name].size // 4096) for name in v)
    k = (13 + math.ceil(math.log2(chunks))) * 2.0 ** -24
    l2 = sum(float((start[name].astype(f64) ** 2).sum()) for name in v if decayed(name)) / 2
    print('l2: got %.9g, float64 %.9g, relative error %.3g of the bound %.3g' % (info['l2'], l2, abs(info['l2'] - l2) / l2, k * (1 + k)))
    assert l2 > 0 and abs(info['l2'] - l2) <= k * (1 + k) * l2, (info['l2'], l2)


def test_2_device_gradients_equal_host_gradients(run):
    """the three backwards that gained weight_grads: the same keys, the same bits, only the variables change their type"""
    for n, (a, b) in run['host_keys'].items():
        assert a == b, (n, sorted(a ^ b))
    assert run['host_types'] == [] and run['host_shapes'] == []
    assert run['host_diff'] == [], run['host_diff']


def test_3_the_training_forward_equals_a_fresh_detector(run):
    assert run['exported_keys'][0] == run['exported_keys'][1] and set(run['variables']) - set(run['exported_moved']) <= set(FROZEN_BY_BN)
    assert run['fwd_diff'] == {}, run['fwd_diff']
    # and the step moved every one of them: rpn_out, feat, cls_reg and both losses
    assert set(run['fwd_moved']) == {'rpn_out', 'feat', 'cls_reg', 'head_loss', 'rpn_loss'}, run['fwd_moved']


def test_4_the_second_backward_equals_a_fresh_detector(run):
    """fails if step leaves a backward operand (K_a, K_b, the heads' concatenated kernels) at the old weights"""
    assert run['grad_keys'][0] == run['grad_keys'][1] == set(run['variables'])
    assert run['grad_diff'] == [], run['grad_diff'][:8]
    assert run['dx_diff'] == [], run['dx_diff']


def test_5_the_eval_net_equals_a_fresh_detector(run):
    assert run['layers'] == 74
    assert equal(run['eval'], run['eval_ref']) == {}
    # (before the refresh the eval net's body and large-separable block still held the checkpoint's weights)
    assert not np.array_equal(run['eval_stale']['feat'], run['eval']['feat'])


def test_6_a_backward_on_a_loss_from_before_the_step_is_refused(run):
    s = run['stale']
    assert s['head'] and 'head_backward: call get_head(..., is_training=True, ...) first' in s['head'], s
    assert s['rpn'] and 'rpn_backward: call get_rpn and losses.rpn_loss(..., keep_device=True) first' in s['rpn'], s
    assert s['rpn_loss_again'] and 'rpn_backward: call get_rpn' in s['rpn_loss_again'], s      # the loss again, but not the forward
    for msg in s.values():
        assert 'MomentumOptimizer.step has run since' in msg


def test_6_the_constructor_names_what_is_missing(run):
    c = run['ctor']
    assert c['rpn_hidden'] and "reach='all' needs a detector built with rpn_hidden=True" in c['rpn_hidden'], c
    assert c['reach'] and "reach must be 'flows' or 'all'" in c['reach'], c


def test_6_the_net_door_refuses_by_name_and_touches_nothing(run):
    d = run['door']
    assert d['partial'][0] == -1 and 'the group of final_head is given in part: final_head/fc_loc/bias is missing' in d['partial'][1]
    assert d['duplicate'][0] == -1 and 'rpn_head/conv2d_1/kernel is given twice' in d['duplicate'][1]
    assert d['flow'][0] == -1 and 'conv2d_4/kernel is outside the reach' in d['flow'][1]
    assert d['null'][0] == -1 and 'rpn_head/conv2d/kernel is a NULL pointer' in d['null'][1]
    assert d['empty'][0] == -1 and 'an empty table' in d['empty'][1]
    assert d['host'] and 'rpn_head/conv2d/bias' in d['host'] and 'device memory' in d['host']
    assert equal(run['eval_after_refusals'], run['eval']) == {}


def test_6_a_spectral_block_refuses_the_eval_refresh(run):
    assert run['sp_error'] and 'large_sep_feature' in run['sp_error'] and 'large_sep=direct' in run['sp_error'], run['sp_error']
    assert equal(run['sp_after'], run['sp_before']) == {}
