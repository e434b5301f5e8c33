"""The Xception middle flow in training mode through the net (LightHeadDetector(middle_flow_train=True), model.middle_flow_train,
model.middle_flow_backward), on the path of tests/test_gpu_exit_flow_backward.py and at its sizes: one pass -- eval body, the
middle flow with batch statistics and the refresh of what the net derived from `mid_x`, the RPN, the training exit flow and
large-separable block, head loss and backward, large_sep_backward, RPN loss and backward, exit_flow_backward,
middle_flow_backward -- on a detector built in split precision (f16x3, where `mid_x` also lives as the ReLU planes the RPN
conv reads), and every stage judged against its float64 statement fed the tensors the GPU left upstream, so one check measures
one step.  The bars are those of tests/test_gpu_exit_flow_backward.py: depthwise forwards 1e-6 of the output scale, pointwise
forwards 3e-5, the batch norms batch_norm_cases.bar() at eps 1e-4 / momentum 0.99, pointwise backwards
conv_backward_cases.bar(), depthwise backwards the dx equality and depthwise_backward_cases.bar() for dw; the sixteen joins
are bit-equal to numpy's f32 adds of the GPU's own addends.  A block's third batch norm output is overwritten by the join
(y3 + x, in place): its addend is had again from xdet_batch_norm_forward on the kept z3, whose bits depend on its inputs and
M alone -- the batch statistics of that second call are compared with the kept ones bit for bit.
Measured on an MI355X, worst fraction of each bar over the 24 units (every test prints its own with -s): depthwise forwards
0.13, pointwise forwards 0.017, batch norm forward 0.0076, backward 0.0035; pointwise backwards 0.28; depthwise backwards: dx
equal everywhere, dw 0.072; the eval middle flow from the GPU's entry_x 0.035 of the stage bar, rpn_out behind the refresh
0.012; conditions: positive share 0.50-0.87, smallest batch variance 5.53e-4, |z| <= 0.73, |mid_x| <= 15.3."""
import numpy as np
import pytest

import batch_norm_cases as BC
import conv_backward_cases as CC
import depthwise_backward_cases as DC

from flow_train_cases import S, P, NC, A, bits, rel_err, close, depthwise_forward64, bn_forward_distances, head_and_rpn_inputs, \
    downstream

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DEPTHWISE_FORWARD_TOL = 1e-6     # tests/test_gpu_layers.py::test_depthwise_matches_oracle
CONV_FORWARD_TOL = 3e-5          # tests/test_gpu_layers.py::test_conv_matches_oracle, f16x3
STAGE_TOL = 1e-4                 # tests/test_gpu_e2e.py::test_dense_stages
EPS, MOMENTUM = 1e-4, 0.99       # the Xception layers' batch norm (model.MIDDLE_FLOW_EPS / _MOMENTUM)
BLOCKS = tuple(range(5, 13))
TRAIN = dict(pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True, middle_flow_train=True)


def refresh_and_rpn(det, M, mid, n):
    """rpn_out and mid as they are, then again behind xdet_net_mid_refresh -> ((rpn_out, mid), (rpn_out, mid))"""
    from xdet._lib import lib, check
    M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
    before = (det.buffer('rpn_out', n).numpy(), mid.numpy())
    check(lib().xdet_net_mid_refresh(det.handle, n, det.stream.handle))
    M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
    return before, (det.buffer('rpn_out', n).numpy(), mid.numpy())


@pytest.fixture(scope='module')
def run(lh_weights):
    """one pass over the whole path; the tests below look at what it left"""
    from xdet import model as M, weights as W, ops, InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor, get_precision, set_precision
    r = {}
    w = lh_weights
    images = W.synthetic_images(2, S, seed=3)
    inputs = head_and_rpn_inputs()

    before = get_precision()
    set_precision('f16x3')
    try:
        plain = LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P)
        det = LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
        small = LightHeadDetector(w, image_size=S, max_batch=1, rpn_post_nms_top_n=P)
    finally:
        set_precision(before)
    with plain.scope():
        _, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['plain_out'], r['plain_mid_x'] = out.numpy(), plain.buffer('mid_x', 2).numpy()
    with small.scope():                              # the refresh on a calibrated net
        r['small_scaled'] = small.calibrate(images[:1])
        mid, _ = M.XceptionBody(images[:1], NC, is_training=False, data_format='channels_first')
        r['small_refresh'] = refresh_and_rpn(small, M, mid, 1)
    r['plain'], r['det'] = plain, det
    with det.scope():
        mid, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['eval_out'], r['eval_mid_x'] = out.numpy(), det.buffer('mid_x', 2).numpy()
        r['entry_x'] = det.buffer('entry_x', 2).numpy()
        r['entry_shape_ld'] = (det.buffer('entry_x', 2).shape, det.buffer('entry_x', 2).ld)
        r['refresh'] = refresh_and_rpn(det, M, mid, 2)
        M.exit_flow_train()                          # (on the eval-mode mid_x: the state middle_flow_train has to drop)
        mid_t = M.middle_flow_train()
        mid_x = det.buffer('mid_x', 2)
        r['mid_is_the_buffer'] = mid_t.ptr == mid.ptr and mid_t.ld == mid.ld and mid_t.shape == mid.shape
        r['mid'], r['mid_x'] = mid_t.numpy(), mid_x.numpy()
        r['mid_shape_ld'] = (mid_x.shape, mid_x.ld)
        sv = det.middle_flow_saved()
        r['x12_out_is_mid_x'] = 'x13' not in sv
        r['saved'] = {k: v.numpy() for k, v in sv.items()}
        # a block's y3 again, by the op the chain ran, from the kept z3 (see the module's docstring)
        for b in BLOCKS:
            u = 'block%d_sepconv3' % b
            r['saved']['block%d/y3' % b], m2, i2, _, _ = ops.batch_norm_forward(r['saved'][u + '/z'], w[u + '_bn/gamma'], w[u + '_bn/beta'],
                                                                               EPS, True, MOMENTUM, stream=det.stream)
            assert np.array_equal(bits(m2), bits(r['saved'][u + '_bn/save_mean'].reshape(-1)))
            assert np.array_equal(bits(i2), bits(r['saved'][u + '_bn/save_invstd'].reshape(-1)))
        d_out0 = DeviceTensor.empty(out.shape, ld=out.ld)
        with pytest.raises(InvalidArgumentError):    # what exit_flow_train saved belongs to the eval-mode mid_x
            M.exit_flow_backward(d_out0)
        lsep, rpn = downstream(M.exit_flow_train(), mid_t, inputs)
        r['rpn_out'] = det.buffer('rpn_out', 2).numpy()
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'])
        r['d_mid_t'], r['d_mid'] = ef['mid'], ef['mid'].numpy()
        host = lambda g: {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in g.items()}
        grads = M.middle_flow_backward(ef['mid'], intermediates=True)
        r['entry_grad_shape_ld'] = (grads['entry'].shape, grads['entry'].ld)
        r['grads'] = host(grads)
        r['again'] = host(M.middle_flow_backward(ef['mid'], intermediates=True))
        r['lean'] = host(M.middle_flow_backward(ef['mid']))
        r['entry_x_after'] = det.buffer('entry_x', 2).numpy()
        r['mid_x_after'] = det.buffer('mid_x', 2).numpy()
    return r


def units(run):
    """per unit: (name, block, index, the unit's input and output as the GPU left them)"""
    sv = run['saved']
    out = []
    for b in BLOCKS:
        ins = (sv['x%d' % b], sv['block%d/y1' % b], sv['block%d/y2' % b])
        outs = (sv['block%d/y1' % b], sv['block%d/y2' % b], sv['block%d/y3' % b])
        out += [('block%d_sepconv%d' % (b, i + 1), b, i + 1, ins[i], outs[i]) for i in range(3)]
    return out


def block_output(run, b):
    return run['saved']['x%d' % (b + 1)] if b != BLOCKS[-1] else run['mid_x']


def test_default_path_unchanged(run):
    """the options change nothing in the eval body: `out` and `mid_x` have the plain detector's bits, which refuses the name"""
    from xdet import InvalidArgumentError
    assert run['plain_out'].shape == (2, 16, 16, 2048) and run['plain_out'].any()
    assert np.array_equal(bits(run['eval_out']), bits(run['plain_out']))
    assert np.array_equal(bits(run['eval_mid_x']), bits(run['plain_mid_x']))
    with pytest.raises(InvalidArgumentError, match='entry_x=keep'):
        run['plain'].buffer('entry_x', 2)


def test_entry_x_survives_the_pass(run):
    assert run['entry_shape_ld'] == ((2, 16, 16, 728), 736) and run['entry_x'].any()
    assert np.array_equal(bits(run['entry_x_after']), bits(run['entry_x']))


def test_entry_x_is_the_middle_flows_input(run, oracle, lh_weights):
    """the eval middle flow in NumPy (the oracle's _sep_bn loop) from the GPU's entry_x against the GPU's eval mid_x"""
    x = run['entry_x']
    for b in BLOCKS:
        res = x
        for s in (1, 2, 3):
            x = oracle._sep_bn(x, lh_weights, 'block%d_sepconv%d' % (b, s))
        x = x + res
    e = rel_err(run['eval_mid_x'], x)
    print('eval mid_x from the GPU\'s entry_x: rel_err / bar = %.4f' % (e / STAGE_TOL))
    assert e < STAGE_TOL


def test_refresh_is_neutral_on_the_eval_tensor(run):
    """the planes the refresh writes are the planes block12_sepconv3's epilogue wrote (tests/test_gpu_conv_planes_out.py,
    item c): rpn_out and mid keep their bits -- on the detector of the pass and on a small one after calibrate()"""
    for name in ('refresh', 'small_refresh'):
        (rpn0, mid0), (rpn1, mid1) = run[name]
        assert rpn0.any() and np.array_equal(bits(rpn0), bits(rpn1)), name
        assert np.array_equal(bits(mid0), bits(mid1)), name
    print('exponents chosen by calibrate() on the small detector: %r' % (run['small_scaled'],))


def test_the_refresh_took(run, oracle, lh_weights):
    """after middle_flow_train the RPN reads the training-mode tensor"""
    assert run['mid_is_the_buffer']
    assert np.array_equal(bits(run['mid']), bits(np.maximum(run['mid_x'], f32(0))))
    assert not np.array_equal(run['mid_x'], run['eval_mid_x'])
    cls, box = oracle.get_rpn(np.maximum(run['mid_x'], f32(0)), lh_weights)
    e = rel_err(run['rpn_out'], np.concatenate([cls, box], -1))
    print('rpn_out on the training mid_x: rel_err / bar = %.4f' % (e / STAGE_TOL))
    assert e < STAGE_TOL
    assert not np.array_equal(run['rpn_out'], run['refresh'][0][0])
    # ... and by a margin the bar resolves: the eval-mode rpn_out is not within it
    assert rel_err(run['refresh'][0][0], np.concatenate([cls, box], -1)) > 10 * STAGE_TOL


def test_conditions_from_the_float64_statements(run, lh_weights):
    """what the masks of the chain rely on, from float64 statements of each unit fed the GPU's upstream tensors: both sides
    of every ReLU are populated and every batch variance is well above zero.  A float64 training-mode middle flow from the
    oracle's entry_x on these inputs gave a positive share of 0.50-0.87, a smallest batch variance of 5.5e-4, |z| <= 0.74 and
    |mid_x| <= 15.3; the envelope asserted here is a little wider, for the GPU's tensors are not the oracle's to the last bit."""
    from xdet.ops import host_batch_norm_forward
    w = lh_weights
    share, var_min, z_max = [], np.inf, 0.
    for name, b, i, x, _ in units(run):
        share.append(float((x > 0).mean()))
        t = depthwise_forward64(x, w[name + '/depthwise_kernel'])
        z = CC.conv_forward64(t, w[name + '/pointwise_kernel'], False)
        _, _, invstd, _, _ = host_batch_norm_forward(z, w[name + '_bn/gamma'], w[name + '_bn/beta'], EPS, True, MOMENTUM, None, None,
                                                     False, f64)
        var_min, z_max = min(var_min, float((1. / invstd ** 2 - EPS).min())), max(z_max, float(np.abs(z).max()))
    share.append(float((run['mid_x'] > 0).mean()))
    print('positive share %.2f-%.2f, smallest batch variance %.2e, |z| <= %.2f, |mid_x| <= %.1f'
          % (min(share), max(share), var_min, z_max, np.abs(run['mid_x']).max()))
    assert 0.45 <= min(share) and max(share) <= 0.90
    assert var_min >= 4e-4 and z_max <= 0.85 and np.abs(run['mid_x']).max() <= 17.


def test_training_forward(run, lh_weights):
    w, sv = lh_weights, run['saved']
    worst = {'depthwise': 0., 'pointwise': 0., 'bn': 0.}
    for name, b, i, x, y in units(run):
        assert sv[name + '/dw'].shape == sv[name + '/z'].shape == y.shape == (2, 16, 16, 728)
        worst['depthwise'] = max(worst['depthwise'], close(name + ' depthwise', sv[name + '/dw'],
                                                           depthwise_forward64(x, w[name + '/depthwise_kernel']), DEPTHWISE_FORWARD_TOL))
        worst['pointwise'] = max(worst['pointwise'], close(name + ' pointwise', sv[name + '/z'],
                                                           CC.conv_forward64(sv[name + '/dw'], w[name + '/pointwise_kernel'], False),
                                                           CONV_FORWARD_TOL))
        bn = name + '_bn/'
        d = bn_forward_distances(sv[name + '/z'], w[bn + 'gamma'], w[bn + 'beta'], w[bn + 'moving_mean'], w[bn + 'moving_variance'],
                                 (y, sv[bn + 'save_mean'], sv[bn + 'save_invstd'], sv[bn + 'moving_mean'], sv[bn + 'moving_variance']),
                                 eps=EPS, momentum=MOMENTUM)
        assert max(d.values()) <= BC.bar(), (name, d)
        worst['bn'] = max(worst['bn'], max(d.values()) / BC.bar())
        assert not np.array_equal(sv[bn + 'moving_mean'].reshape(-1), w[bn + 'moving_mean'])
        assert not np.array_equal(sv[bn + 'moving_variance'].reshape(-1), w[bn + 'moving_variance'])
    print('training forward, worst fraction of the bar: %s' % ', '.join('%s %.4f' % kv for kv in sorted(worst.items())))
    # the eight joins: numpy's f32 add of the GPU's own addends; the last one is the net's mid_x
    assert run['x12_out_is_mid_x'] and run['mid_shape_ld'] == ((2, 16, 16, 728), 736)
    assert np.array_equal(bits(sv['x5']), bits(run['entry_x']))
    for b in BLOCKS:
        assert np.array_equal(bits(block_output(run, b)), bits(sv['block%d/y3' % b] + sv['x%d' % b])), b
    assert np.array_equal(bits(run['mid_x_after']), bits(run['mid_x']))


def test_the_chain(run, lh_weights):
    """every backward step against its statement fed the gradient the GPU left upstream"""
    from xdet.ops import host_depthwise_backward
    w, sv, g = lh_weights, run['saved'], run['grads']
    assert run['d_mid'].any()
    worst = {'bn': 0., 'pointwise': 0., 'depthwise dw': 0.}
    for name, b, i, x, _ in reversed(units(run)):
        g_out = g['x%d' % (b + 1)] if b != BLOCKS[-1] else run['d_mid']
        dy = {3: g_out, 2: g.get('d3/block%d' % b), 1: g.get('d2/block%d' % b)}[i]
        dx = g['d%d/block%d' % (i, b)]
        bn = name + '_bn'
        d = BC.backward_distances(dict(x=sv[name + '/z'], dy=dy, gamma=w[bn + '/gamma'], relu=False), True, None,
                                  sv[bn + '/save_mean'].reshape(-1), sv[bn + '/save_invstd'].reshape(-1),
                                  (g['z/' + name], g[bn + '/gamma'], g[bn + '/beta']))
        assert max(d.values()) <= BC.bar(), (name, d)
        worst['bn'] = max(worst['bn'], max(d.values()) / BC.bar())
        ref, den = CC.reference64(sv[name + '/dw'], w[name + '/pointwise_kernel'], g['z/' + name], None, False)
        d = CC.distances((g['dw/' + name], g[name + '/pointwise_kernel'], None), ref, den)
        assert max(d) <= CC.bar(), (name, d)
        worst['pointwise'] = max(worst['pointwise'], max(d) / CC.bar())
        kd = w[name + '/depthwise_kernel']
        assert np.array_equal(dx, host_depthwise_backward(x, kd, g['dw/' + name], 1, True)[0]), name
        (_, ref_dw), den = DC.reference64(x, kd, g['dw/' + name], 1, True)
        d = DC.dw_distance(g[name + '/depthwise_kernel'], ref_dw, den)
        assert d <= DC.bar(), (name, d / DC.bar())
        worst['depthwise dw'] = max(worst['depthwise dw'], d / DC.bar())
        if i == 1:                                   # the join, in its order: d1 + g
            got = g['x%d' % b] if b != BLOCKS[0] else g['entry']
            assert np.array_equal(bits(got), bits(dx + g_out)), b
            # d1 vanishes where the block's input is not positive; the residual share does not
            assert not dx[~(x > 0)].any() and got[~(x > 0)].any(), b
    print('the chain, worst fraction of the bar: %s' % ', '.join('%s %.4f' % kv for kv in sorted(worst.items())))


def test_gradients(run, lh_weights):
    from xdet.model import MIDDLE_FLOW_VARIABLES, MIDDLE_FLOW_UNITS
    g = run['grads']
    names = {u + v for b in BLOCKS for u in ['block%d_sepconv%d' % (b, i) for i in (1, 2, 3)]
             for v in ('/depthwise_kernel', '/pointwise_kernel', '_bn/gamma', '_bn/beta')}
    assert len(names) == 96 and set(MIDDLE_FLOW_VARIABLES) == names and len(MIDDLE_FLOW_UNITS) == 24
    lean = run['lean']
    assert set(lean) == names | {'entry'} | {'x%d' % b for b in BLOCKS[1:]}
    assert set(g) >= set(lean) | {'dw/' + u for u in MIDDLE_FLOW_UNITS} | {'z/' + u for u in MIDDLE_FLOW_UNITS} | \
        {'d%d/block%d' % (i, b) for b in BLOCKS for i in (1, 2, 3)}
    for k in names:
        assert g[k].shape == lh_weights[k].shape and g[k].dtype == f32 and np.isfinite(g[k]).all() and g[k].any(), k
    assert run['entry_grad_shape_ld'] == run['entry_shape_ld']
    for k in g:
        assert np.array_equal(bits(g[k]), bits(run['again'][k])), k
    for k in lean:
        assert np.array_equal(bits(g[k]), bits(lean[k])), k


def test_refusals(run, lh_weights):
    from xdet import model as M, InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor
    plain, det = run['plain'], run['det']
    kw = dict(image_size=S, max_batch=1, rpn_post_nms_top_n=P)
    with pytest.raises(InvalidArgumentError, match='exit_flow_train'):
        LightHeadDetector(lh_weights, large_sep_train=True, middle_flow_train=True, **kw)
    with pytest.raises(InvalidArgumentError, match='block7_sepconv2_bn/moving_variance'):
        LightHeadDetector({k: v for k, v in lh_weights.items() if k != 'block7_sepconv2_bn/moving_variance'},
                          large_sep_train=True, exit_flow_train=True, middle_flow_train=True, **kw)
    with plain.scope():
        with pytest.raises(InvalidArgumentError):
            M.middle_flow_train()
        with pytest.raises(InvalidArgumentError):
            M.middle_flow_backward(run['d_mid_t'])
        with pytest.raises(InvalidArgumentError):
            plain.middle_flow_saved()
    fresh = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, large_sep_train=True, exit_flow_train=True,
                              middle_flow_train=True)
    with fresh.scope():
        with pytest.raises(InvalidArgumentError):
            M.middle_flow_train()                                                     # no body has run
        with pytest.raises(InvalidArgumentError):
            M.middle_flow_backward(run['d_mid_t'])                                    # no training forward has run
        with pytest.raises(InvalidArgumentError):
            fresh.middle_flow_saved()
    with det.scope():
        with pytest.raises(InvalidArgumentError):
            M.middle_flow_backward(DeviceTensor.empty((2, 8, 8, 728)))
        with pytest.raises(InvalidArgumentError):
            M.middle_flow_backward(DeviceTensor.empty((2, 16, 16, 728), ld=728))       # another ld
        with pytest.raises(InvalidArgumentError):
            M.middle_flow_backward(run['d_mid'])                                      # not on the device
        # (the fixture has shown exit_flow_backward refusing between middle_flow_train and a new exit_flow_train)
