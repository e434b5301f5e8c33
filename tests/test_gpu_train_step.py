"""One and two optimizer steps on the detector of the flow tests (TRAIN, S = 256, P = 64, max_batch = 2): the masters the
stages hold, updated in place by xdet_momentum_step, against train_ops.host_momentum_step; the forward layers, refreshed on the
device, against a second detector built from export_weights(); the saved state dropped by the step; and weight_grads='device'
against 'host'.  Every comparison is for equal bits: every op of the chain gives the same bits for the same call.
The fixture builds the two detectors and runs everything once; the tests look at what it recorded."""
import time

import numpy as np
import pytest

from flow_train_cases import S, P, NC, bits, head_and_rpn_inputs, downstream
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_train_partial_batch import recorded_losses

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SAVED = ('entry_flow_saved', 'middle_flow_saved', 'exit_flow_saved', 'large_sep_saved')
LR = (1e-2, 3e-3)                                       # two steps, two rates
MOMENTUM, WEIGHT_DECAY = 0.9, 2e-4


def host(v):
    return v.numpy() if hasattr(v, 'numpy') else (None if v is None else np.asarray(v))


def same(a, b):
    a, b = host(a), host(b)
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def forwards_and_backwards(det, inputs, weight_grads, images=None):
    """the three training forwards (behind an eval body when images are given), the chain behind them and the three backwards
    -> (losses, {section: dict}) as the calls returned them"""
    from xdet import model as M
    losses = {}
    with det.scope():
        if images is not None:
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        M.entry_flow_train()
        mid = M.middle_flow_train()
        with recorded_losses(losses):
            lsep, rpn = downstream(M.exit_flow_train(), mid, inputs)
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'], weight_grads=weight_grads)
        mf = M.middle_flow_backward(ef['mid'], weight_grads=weight_grads)
        en = M.entry_flow_backward(mf['entry'], weight_grads=weight_grads)
    return losses, {'large_sep_backward': lsep, 'rpn_backward': rpn, 'exit_flow_backward': ef, 'middle_flow_backward': mf,
                    'entry_flow_backward': en}


def weight_gradients(sections, variables):
    g = {}
    for name in ('entry_flow_backward', 'middle_flow_backward', 'exit_flow_backward'):
        g.update({k: v for k, v in sections[name].items() if k in variables})
    return g


def host_step(before, grads, lr, variables):
    from xdet import host_momentum_step
    from xdet.train import decayed
    out = {}
    for v in variables:
        out[v], out[v + '/Momentum'] = host_momentum_step(before[v], grads[v], before[v + '/Momentum'], lr, MOMENTUM, WEIGHT_DECAY,
                                                          decayed(v))
    return out


@pytest.fixture(scope='module')
def run(lh_weights):
    from xdet import model as M, train, weights as W, InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor, get_precision, set_precision
    t0 = time.time()
    r = {}
    images, inputs = W.synthetic_images(2, S, seed=3), head_and_rpn_inputs()
    build = lambda w: LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
    before = get_precision()
    set_precision('f16x3')
    try:
        det = build(lh_weights)
        opt = train.MomentumOptimizer(det, MOMENTUM, WEIGHT_DECAY)
        variables = r['variables'] = opt.variables
        r['read0'] = opt.read()
        # ---- pass 1 and step 1
        _, sec = forwards_and_backwards(det, inputs, 'device', images)
        dev = weight_gradients(sec, variables)
        r['all_device'] = all(isinstance(dev[v], DeviceTensor) for v in variables)
        r['grads1'] = {v: host(dev[v]) for v in variables}
        r['info1'] = opt.step(dev, LR[0])
        r['read1'] = opt.read()
        # ---- (c) the saved state is gone
        r['refusals'] = {}
        with det.scope():
            for fn, call in (('exit_flow_backward', lambda: M.exit_flow_backward(sec['large_sep_backward']['out'])),
                             ('middle_flow_backward', lambda: M.middle_flow_backward(sec['exit_flow_backward']['mid'])),
                             ('entry_flow_backward', lambda: M.entry_flow_backward(sec['middle_flow_backward']['entry'])),
                             ('exit_flow_saved', det.exit_flow_saved)):
                try:
                    call()
                    r['refusals'][fn] = None
                except InvalidArgumentError as e:
                    r['refusals'][fn] = str(e)
        exported = opt.export_weights(lh_weights)
        r['exported_keys'] = (set(exported), set(lh_weights))
        # ---- (b) the training forwards again, without an eval body; a detector built from the exported weights, from the images
        losses1, sec1 = forwards_and_backwards(det, inputs, 'device')
        saved1 = {name: getattr(det, name)() for name in SAVED}
        det2 = build(exported)
        losses2, sec2 = forwards_and_backwards(det2, inputs, 'host', images)
        saved2 = {name: getattr(det2, name)() for name in SAVED}
        r['saved_keys'] = sum(len(saved1[n]) for n in SAVED)
        r['saved_diff'] = [n + '/' + k for n in SAVED for k in saved1[n] if k not in saved2[n] or not same(saved1[n][k], saved2[n][k])]
        r['saved_diff'] += [n + '/' + k for n in SAVED for k in saved2[n] if k not in saved1[n]]
        r['loss_diff'] = [n + '/' + k for n in ('head_loss', 'rpn_loss') for k in losses2[n] if not same(losses1[n][k], losses2[n][k])]
        r['loss_fields'] = sum(len(losses2[n]) for n in ('head_loss', 'rpn_loss'))
        r['head_loss'] = (float(losses1['head_loss']['losses'][0]), float(losses2['head_loss']['losses'][0]))
        r['grad_keys'] = {n: (set(sec1[n]), set(sec2[n])) for n in sec2}
        r['grad_diff'] = [n + '/' + k for n in sec2 for k in sec2[n] if k not in sec1[n] or not same(sec1[n][k], sec2[n][k])]
        # ---- (e) on det2's state: 'device' downloaded against 'host'
        with det2.scope():
            ef = M.exit_flow_backward(sec2['large_sep_backward']['out'], sec2['rpn_backward']['mid'], weight_grads='device')
            mf = M.middle_flow_backward(ef['mid'], weight_grads='device')
            en = M.entry_flow_backward(mf['entry'], weight_grads='device')
        again = {'exit_flow_backward': ef, 'middle_flow_backward': mf, 'entry_flow_backward': en}
        r['device_keys'] = {n: (set(again[n]), set(sec2[n])) for n in again}
        r['device_diff'] = [n + '/' + k for n in again for k in sec2[n] if not same(again[n].get(k), sec2[n][k])]
        r['device_types'] = [n + '/' + k for n in again for k in again[n] if k in variables and
                             not (isinstance(again[n][k], DeviceTensor) and again[n][k].shape == np.shape(sec2[n][k])
                                  and again[n][k].ld == again[n][k].shape[-1])]
        r['host_types'] = [n + '/' + k for n in again for k in sec2[n] if k in variables and not isinstance(sec2[n][k], np.ndarray)]
        # ---- (d) step 2 on det, from live momentum slots
        dev = weight_gradients(sec1, variables)
        r['grads2'] = {v: host(dev[v]) for v in variables}
        r['info2'] = opt.step(dev, LR[1])
        r['read2'] = opt.read()
        # a missing gradient and a host array are refused by name ahead of any launch: nothing moves
        bad = dict(dev)
        del bad['block7_sepconv2/pointwise_kernel']
        r['step_refusals'] = []
        for grads in (bad, dict(dev, **{'conv2d_4/kernel': r['grads2']['conv2d_4/kernel']})):
            try:
                opt.step(grads, 1.0)
                r['step_refusals'].append(None)
            except InvalidArgumentError as e:
                r['step_refusals'].append(str(e))
        r['read2_again'], r['steps'] = opt.read(), opt.steps
    finally:
        set_precision(before)
    r['weights'] = lh_weights
    print('fixture: %.1f s' % (time.time() - t0))
    return r


def assert_equal_tables(got, want, variables):
    assert set(got) == set(want) == set(variables) | set(v + '/Momentum' for v in variables)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == f32, k
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, int((bits(got[k]) != bits(want[k])).sum()), got[k].size)


def test_the_variables_are_the_three_flows(run):
    from xdet import train
    assert run['variables'] == train.ENTRY_FLOW_VARIABLES + train.MIDDLE_FLOW_VARIABLES + train.EXIT_FLOW_VARIABLES
    assert len(run['variables']) == 148 and run['all_device']
    for v in run['variables']:                          # the masters start as the checkpoint's values, the slots at zero
        want = np.asarray(run['weights'][v], f32)
        assert run['read0'][v].shape == want.shape and np.array_equal(bits(run['read0'][v]), bits(want)), v
        assert not run['read0'][v + '/Momentum'].any(), v


def test_step_one_equals_the_host_statement(run):
    """(a) the host inputs are the original weights and the downloaded gradients"""
    start = {v: np.asarray(run['weights'][v], f32) for v in run['variables']}
    start.update({v + '/Momentum': np.zeros_like(start[v]) for v in run['variables']})
    want = host_step(start, run['grads1'], LR[0], run['variables'])
    assert_equal_tables(run['read1'], want, run['variables'])
    moved = [v for v in run['variables'] if not np.array_equal(run['read1'][v], start[v])]
    assert len(moved) == 148, sorted(set(run['variables']) - set(moved))
    info = run['info1']
    assert set(info) == {'step', 'lr', 'l2'} and info['step'] == 1 and info['lr'] == LR[0]
    from xdet.train import decayed
    l2 = sum(float((start[v].astype(f64) ** 2).sum()) for v in run['variables'] if decayed(v)) / 2
    assert l2 > 0 and abs(info['l2'] - l2) <= 64 * 2.0 ** -24 * l2, (info['l2'], l2)


def test_refreshed_layers_equal_a_detector_built_from_the_exported_weights(run):
    """(b) every *_saved() tensor, the losses and every gradient of the next backward"""
    assert run['exported_keys'][0] == run['exported_keys'][1]
    # (275 tensors: 77 + 152 + 40 of the three flows and 6 of the large-separable block)
    assert run['saved_keys'] >= 270 and run['saved_diff'] == [], run['saved_diff'][:8]
    assert run['loss_fields'] >= 8 and run['loss_diff'] == [], run['loss_diff']
    assert run['head_loss'][0] == run['head_loss'][1] and np.isfinite(run['head_loss'][0])
    for n, (a, b) in run['grad_keys'].items():
        assert a == b, (n, sorted(a ^ b))
    assert run['grad_diff'] == [], run['grad_diff'][:8]


def test_the_step_drops_the_saved_state(run):
    """(c) each backward refuses with its own sentence (and ran again after the training forwards: the fixture went on)"""
    r = run['refusals']
    assert r['exit_flow_backward'] and 'exit_flow_backward: call exit_flow_train() first' in r['exit_flow_backward'], r
    assert r['middle_flow_backward'] and 'middle_flow_backward: call middle_flow_train() first' in r['middle_flow_backward'], r
    assert r['entry_flow_backward'] and 'entry_flow_backward: call entry_flow_train() first' in r['entry_flow_backward'], r
    assert r['exit_flow_saved'] and 'exit_flow_saved: no model.exit_flow_train() has run' in r['exit_flow_saved'], r


def test_step_two_equals_the_host_statement(run):
    """(d) from non-zero momentum slots"""
    assert any(run['read1'][v + '/Momentum'].any() for v in run['variables'])
    want = host_step(run['read1'], run['grads2'], LR[1], run['variables'])
    assert_equal_tables(run['read2'], want, run['variables'])
    assert run['info2']['step'] == 2 and run['info2']['lr'] == LR[1] and run['info2']['l2'] != run['info1']['l2']
    a, b = run['step_refusals']
    assert a and 'the gradients lack block7_sepconv2/pointwise_kernel' in a, a
    assert b and 'the gradient of conv2d_4/kernel must be a dense DeviceTensor' in b, b
    assert run['steps'] == 2
    assert_equal_tables(run['read2_again'], run['read2'], run['variables'])


def test_weight_grads_host_is_what_it_was(run):
    """(e) the same keys, and the same bits as a 'device' call downloaded; only the variables change their type"""
    for n, (a, b) in run['device_keys'].items():
        assert a == b, (n, sorted(a ^ b))
    assert run['device_diff'] == [] and run['device_types'] == [] and run['host_types'] == []
