"""The optimizer step over the whole network: MomentumOptimizer(reach='all') on a detector built with stem_train=True (the
detector of tests/test_gpu_optimizer_heads.py -- S = 256, P = 64, max_batch 2, its ALL flags -- plus the stem), one full
iteration with weight_grads='device' in all seven backwards, one step over the 176 variables, and then what the step and
refresh_eval_net() must have brought in line for the stem, each against a detector built afresh from opt.export_weights():
the six stem masters against the host statement, stem_train() on the stepped weights, the eval body after the refresh, a graph
captured before the refresh, and refresh_stem's refusals.  Every comparison is for equal bits.
A second, calibrated case: the checkpoint with block1_conv1_bn's gamma and beta x 2^K and block1_conv2's kernel x 2^-K (the
same function; the stem's first activation leaves the range the calibration keeps planes in), K the first of 10, 11, ... at
which calibrate gives the plane 'block1_conv1 [stem]' an exponent.  There the stem is stepped alone (reach='flows', drawn
gradients for the six stem variables, zeros for the flows: a cheap way to new weights) and the refreshed eval body is held
against a detector built from the exported weights and calibrated on the same batch, after both report the same
plane_scales().  One module fixture runs everything; the tests read what it recorded."""
import numpy as np
import pytest

from flow_train_cases import S, P, NC, bits, head_and_rpn_inputs
from test_gpu_net_refresh import detections, equal, graph_count
from test_gpu_optimizer_heads import ALL, LR, MOMENTUM, WEIGHT_DECAY, host, iteration, weight_gradients

pytestmark = pytest.mark.gpu
f32 = np.float32
STEM_ALL = dict(ALL, stem_train=True)
BODY = ('stem_out', 'entry_x', 'mid_x', 'out')
STEM_PLANE = 'block1_conv1 [stem]'


def eval_body(det, images):
    from xdet import model as M
    n = images.shape[0]
    with det.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        return {name: bits(det.buffer(name, n).numpy()) for name in BODY}


def stem_exponent(det):
    return [e for name, e in det.plane_scales().items() if STEM_PLANE in name]


@pytest.fixture(scope='module')
def run(lh_weights):
    import xdet
    from xdet import model as M, train, weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor, get_precision, set_precision, to_device
    r = {'weights': lh_weights}
    images, inputs = W.synthetic_images(2, S, seed=3), head_and_rpn_inputs()
    build = lambda w, **kw: LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **dict(STEM_ALL, **kw))
    before = get_precision()
    set_precision('f16x3')
    try:
        det = build(lh_weights)
        opt = train.MomentumOptimizer(det, MOMENTUM, WEIGHT_DECAY, reach='all')
        variables = r['variables'] = opt.variables
        r['read0'] = opt.read()
        r['captured'] = detections(det, images)          # the graph every later forward of `det` replays
        r['graphs0'] = graph_count(det)
        # ---- one iteration: the body, the stem, the six other sections, the stem's backward
        with det.scope():
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
            M.stem_train()
        it = iteration(det, inputs, 'device')
        with det.scope():
            stem = M.stem_backward(it['sections']['entry_flow_backward']['stem'], weight_grads='device')
        dev = weight_gradients(it['sections'], variables)
        dev.update(stem)
        r['all_device'] = [v for v in variables if not (isinstance(dev.get(v), DeviceTensor) and dev[v].ld == dev[v].shape[-1])]
        r['grads1'] = {v: host(dev[v]) for v in train.STEM_VARIABLES}
        r['info'] = opt.step(dev, LR)
        r['read1'] = opt.read()
        try:
            det.stem_saved()
            r['saved_after_step'] = None
        except xdet.InvalidArgumentError as e:
            r['saved_after_step'] = str(e)
        # ---- stem_train() on the stepped weights against a detector built from them
        with det.scope():
            r['stem2'] = bits(M.stem_train().numpy())
            r['moving2'] = {k: bits(v.numpy()) for k, v in det.stem_saved().items() if '/moving_' in k}
        exported = opt.export_weights(lh_weights)
        r['exported_keys'] = (set(exported), set(lh_weights))
        r['exported_moved'] = [v for v in train.STEM_VARIABLES + train.STEM_MOVING
                               if not np.array_equal(exported[v], np.asarray(lh_weights[v], f32))]
        r['exported_moving'] = {k: bits(exported[k].reshape(1, 1, 1, -1)) for k in train.STEM_MOVING}
        at_step = dict(exported, **{k: lh_weights[k] for k in train.STEM_MOVING})    # (the moving statistics as stem2's pass found them)
        det2 = build(at_step)
        with det2.scope():
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
            r['stem2_ref'] = bits(M.stem_train().numpy())
            r['moving2_ref'] = {k: bits(v.numpy()) for k, v in det2.stem_saved().items() if '/moving_' in k}
        del det2
        # ---- the eval net: stale, refreshed, and a detector built from what the optimizer exports now
        r['body_stale'] = eval_body(det, images)
        r['layers'] = opt.refresh_eval_net()
        r['graphs1'] = graph_count(det)
        fresh = build(exported)
        r['body'], r['body_ref'] = eval_body(det, images), eval_body(fresh, images)
        r['replayed'], r['replayed_ref'] = detections(det, images), detections(fresh, images)
        r['graphs2'] = graph_count(det)
        del fresh
        # ---- refresh_stem's refusals, each ahead of any GPU work, and the eval body unchanged behind them
        tensors = opt.eval_net_stem_tensors()
        r['stem_tensor_names'] = set(tensors)
        r['door'] = {}
        for what, t in (('host', dict(tensors, **{'block1_conv1_bn/gamma': np.ones(32, f32)})),
                        ('outside', dict(tensors, **{'conv2d_1/kernel': opt._master['conv2d_1/kernel'][0]})),
                        ('partial', {k: v for k, v in tensors.items() if k != 'block1_conv2_bn/moving_variance'}),
                        ('one group', {k: v for k, v in tensors.items() if k.startswith('block1_conv2')})):
            try:
                det.refresh_stem(t)
                r['door'][what] = None
            except xdet.InvalidArgumentError as e:
                r['door'][what] = str(e)
        r['body_after_door'] = eval_body(det, images)
        del det, opt

        # ---- the calibrated case
        k = 10
        while True:
            hot = dict(lh_weights)
            for name in ('block1_conv1_bn/gamma', 'block1_conv1_bn/beta'):
                hot[name] = (np.asarray(lh_weights[name], f32) * f32(2.0 ** k)).astype(f32)
            hot['block1_conv2/kernel'] = (np.asarray(lh_weights['block1_conv2/kernel'], f32) * f32(2.0 ** -k)).astype(f32)
            cal = build(hot)
            cal.calibrate(images)
            if any(stem_exponent(cal)) or k >= 14:
                break
            k += 1
            del cal
        r['c/k'], r['c/exponent'] = k, stem_exponent(cal)
        if any(r['c/exponent']):
            copt = train.MomentumOptimizer(cal, MOMENTUM, WEIGHT_DECAY)
            r['c/variables'] = len(copt.variables)
            with cal.scope():
                M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
                M.stem_train()                           # (moves the stem's moving statistics)
            # The scaled pair is the same function but badly conditioned for a gradient step (d K2 carries 2^K, K2 itself
            # 2^-K), and all that is asked for here is new weights: each stem variable gets a drawn gradient of ten times its
            # own mean magnitude, which the step at LR turns into a change of about one per cent; the flows get zeros.
            rng, grads = np.random.default_rng(9), {}
            for i, v in enumerate(copt.variables):
                shape = copt._master[v][1]
                g = np.zeros(shape, f32)
                if i < 6:
                    g = (rng.standard_normal(shape) * 10 * np.abs(hot[v]).mean()).astype(f32)
                buf = to_device(g)
                grads[v] = DeviceTensor(buf.ptr, shape, shape[-1], owner=buf)
            copt.step(grads, LR)
            r['c/scales_before'] = cal.plane_scales()
            r['c/body_stale'] = eval_body(cal, images)
            r['c/layers'] = copt.refresh_eval_net()
            r['c/scales'] = cal.plane_scales()
            cexp = copt.export_weights(hot)
            r['c/moved'] = [v for v in train.STEM_VARIABLES if not np.array_equal(cexp[v], hot[v])]
            ref = build(cexp)
            ref.calibrate(images)
            r['c/scales_ref'] = ref.plane_scales()
            r['c/body'], r['c/body_ref'] = eval_body(cal, images), eval_body(ref, images)
    finally:
        set_precision(before)
    return r


def test_the_variables(run):
    from xdet import train
    v = run['variables']
    assert v == train.optimizer_variables((True,) * 4, 'all', stem=True) and len(v) == 176 and len(set(v)) == 176
    assert v[:6] == train.STEM_VARIABLES and run['all_device'] == []
    for name in train.STEM_VARIABLES:                   # the masters start as the checkpoint's values, the slots at zero
        want = np.asarray(run['weights'][name], f32)
        assert run['read0'][name].shape == want.shape and np.array_equal(bits(run['read0'][name]), bits(want)), name
        assert not run['read0'][name + '/Momentum'].any(), name


def test_the_step_equals_the_host_statement_on_the_stem(run):
    from xdet import host_momentum_step
    from xdet.train import decayed, STEM_VARIABLES
    assert [decayed(v) for v in STEM_VARIABLES] == [True, False, False, True, False, False]
    for name in STEM_VARIABLES:
        start = np.asarray(run['weights'][name], f32)
        assert run['grads1'][name].any(), name
        var, acc = host_momentum_step(start, run['grads1'][name], np.zeros_like(start), LR, MOMENTUM, WEIGHT_DECAY, decayed(name))
        for key, want in ((name, var), (name + '/Momentum', acc)):
            got = run['read1'][key]
            assert got.shape == want.shape and got.dtype == f32, key
            assert np.array_equal(bits(got), bits(want)), (key, int((bits(got) != bits(want)).sum()), got.size)
        assert not np.array_equal(run['read1'][name], start), name
    assert run['info']['step'] == 1 and len(run['read1']) == 2 * 176


def test_the_step_drops_the_stems_saved_state(run):
    assert run['saved_after_step'] and 'stem_saved: no model.stem_train() has run on this detector' in run['saved_after_step']


def test_stem_train_after_the_step_equals_a_fresh_detector(run):
    from xdet.train import STEM_VARIABLES, STEM_MOVING
    assert run['exported_keys'][0] == run['exported_keys'][1]
    assert set(run['exported_moved']) == set(STEM_VARIABLES + STEM_MOVING)
    assert run['stem2'].any() and np.array_equal(run['stem2'], run['stem2_ref'])
    # the moving statistics: two updates from the checkpoint's on `det`, what export_weights carries ...
    for k in STEM_MOVING:
        assert np.array_equal(run['moving2'][k], run['exported_moving'][k]), k
        assert not np.array_equal(run['moving2'][k], run['moving2_ref'][k]), k       # ... and one on the fresh detector


def test_the_eval_net_equals_a_fresh_detector(run):
    assert run['layers'] == 76
    assert equal(run['body'], run['body_ref']) == {}
    # before the refresh the eval stem still held the checkpoint's weights
    assert set(equal(run['body'], run['body_stale'])) == set(BODY)


def test_a_graph_captured_before_the_refresh_computes_with_the_new_weights(run):
    assert run['graphs0'] == run['graphs1'] == run['graphs2'] == 1
    assert equal(run['replayed'], run['replayed_ref']) == {}
    assert equal(run['replayed'], run['captured']) != {}


def test_refresh_stem_refuses_by_name_and_touches_nothing(run):
    from xdet.train import STEM_VARIABLES, STEM_MOVING
    assert run['stem_tensor_names'] == set(STEM_VARIABLES + STEM_MOVING)
    d = run['door']
    assert d['host'] and 'refresh_stem: block1_conv1_bn/gamma must be a DeviceTensor or a DeviceBuffer (device memory)' in d['host'], d
    assert d['outside'] and 'refresh_stem: conv2d_1/kernel is outside the reach' in d['outside'], d
    assert d['partial'] and 'the group of block1_conv2 is given in part: block1_conv2_bn/moving_variance is missing' in d['partial'], d
    assert d['one group'] is None                      # a whole group alone is a whole table
    assert equal(run['body_after_door'], run['body']) == {}


def test_the_calibrated_eval_net_equals_a_fresh_detector(run):
    print('k = %d, exponent of %r: %s' % (run['c/k'], STEM_PLANE, run['c/exponent']))
    assert any(run['c/exponent']), 'no K up to 14 gives the stem plane an exponent at this size'
    assert run['c/variables'] == 154 and run['c/layers'] == 74
    assert len(run['c/moved']) == 6
    assert run['c/scales'] == run['c/scales_before'] == run['c/scales_ref']
    assert equal(run['c/body'], run['c/body_ref']) == {}
    assert 'stem_out' in equal(run['c/body'], run['c/body_stale'])
