"""The Xception exit flow in training mode through the net (LightHeadDetector(exit_flow_train=True), model.exit_flow_train,
model.exit_flow_backward), on the path of tests/test_gpu_large_sep_backward.py: one pass -- eval body, the exit flow with
batch statistics, the training large-separable block, head loss and backward, large_sep_backward, RPN loss and backward,
exit_flow_backward -- and every stage judged against its float64 statement fed the tensors the GPU left upstream, so one
check measures one step.  Depthwise forwards keep the bar of tests/test_gpu_layers.py (1e-6 of the output scale), pointwise
forwards its f16x3 bar (3e-5), the batch norms the metric and bar of tests/batch_norm_cases.py evaluated at this flow's
constants (eps 1e-4, momentum 0.99), pointwise backwards conv_backward_cases.bar(), depthwise backwards the dx equality and
the dw bar of tests/depthwise_backward_cases.py; the two joins are bit-equal to numpy's f32 adds of the GPU's own addends.
Measured on an MI355X, worst fraction of each bar: depthwise forwards 0.15, pointwise forwards 0.02,
batch norm forward 0.007 (var), backward 0.002 (dx); pointwise backwards 0.27 (dx of block14_sepconv2) and 0.13 (dW); depthwise
backwards: dx equal everywhere, dw 0.04."""
import numpy as np
import pytest

import batch_norm_cases as BC
import conv_backward_cases as CC
import depthwise_backward_cases as DC

from flow_train_cases import S, P, NC, bits, close, depthwise_forward64, bn_forward_distances, head_and_rpn_inputs, downstream

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DEPTHWISE_FORWARD_TOL = 1e-6     # tests/test_gpu_layers.py::test_depthwise_matches_oracle
CONV_FORWARD_TOL = 3e-5          # tests/test_gpu_layers.py::test_conv_matches_oracle, f16x3
EPS, MOMENTUM = 1e-4, 0.99       # the Xception layers' batch norm (model.EXIT_FLOW_EPS / _MOMENTUM)


@pytest.fixture(scope='module')
def run(lh_weights):
    """one pass over the whole path; the tests below look at what it left"""
    from xdet import model as M, weights as W
    from xdet.model import LightHeadDetector
    r = {}
    images = W.synthetic_images(2, S, seed=3)
    inputs = head_and_rpn_inputs()

    plain = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P)
    with plain.scope():
        _, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['plain_out'] = out.numpy()
    r['plain'] = plain
    det = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, pool_index=True, rpn_hidden=True,
                            large_sep_train=True, exit_flow_train=True)
    r['det'] = det
    with det.scope():
        mid, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['eval_out'] = out.numpy()
        r['mid_x'] = det.buffer('mid_x', 2).numpy()
        r['mid_shape_ld'] = (det.buffer('mid_x', 2).shape, det.buffer('mid_x', 2).ld)
        out_t = M.exit_flow_train()
        assert out_t.ptr == out.ptr and out_t.ld == out.ld
        r['out'] = out_t.numpy()
        r['saved'] = {k: v.numpy() for k, v in det.exit_flow_saved().items()}
        lsep, rpn = downstream(out_t, mid, inputs)
        r['d_out_t'] = lsep['out']
        r['d_out'] = lsep['out'].numpy()
        r['d_mid'] = rpn['mid'].numpy()
        host = lambda g: {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in g.items()}
        grads = M.exit_flow_backward(lsep['out'], rpn['mid'])
        r['grads'] = host(grads)
        r['mid_grad_shape_ld'] = (grads['mid'].shape, grads['mid'].ld)
        r['no_mid'] = host(M.exit_flow_backward(lsep['out']))
        r['again'] = host(M.exit_flow_backward(lsep['out'], rpn['mid']))
        r['mid_x_after'] = det.buffer('mid_x', 2).numpy()
        r['out_after'] = det.buffer('out', 2).numpy()
    return r


def units(run, w):
    """per separable unit: (name, dilation, relu_in, relu_out, the unit's input and output as the GPU left them)"""
    sv = run['saved']
    ins = (run['mid_x'], sv['a'], sv['b2'], sv['c3'])
    outs = (sv['a'], sv['y2'], sv['c3'], run['out'])
    from xdet.model import EXIT_FLOW_UNITS
    return [(n, d, ri, ro, x, y) for (n, d, ri, ro), x, y in zip(EXIT_FLOW_UNITS, ins, outs)]


def test_default_path_unchanged(run):
    """the option changes nothing until exit_flow_train() is called; afterwards `out` holds the training-mode tensor and
    `mid_x` what the eval body wrote"""
    assert run['plain_out'].shape == (2, 16, 16, 2048) and run['plain_out'].any()
    assert np.array_equal(bits(run['eval_out']), bits(run['plain_out']))
    assert not np.array_equal(run['out'], run['eval_out'])
    assert np.array_equal(bits(run['mid_x_after']), bits(run['mid_x']))
    assert np.array_equal(bits(run['out_after']), bits(run['out']))


def test_refusals(run, lh_weights):
    from xdet import model as M, InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor
    plain, det = run['plain'], run['det']
    with pytest.raises(InvalidArgumentError):
        LightHeadDetector(lh_weights, image_size=S, max_batch=1, rpn_post_nms_top_n=P, exit_flow_train=True)
    with pytest.raises(InvalidArgumentError):
        LightHeadDetector({k: v for k, v in lh_weights.items() if k != 'block14_sepconv1_bn/moving_variance'}, image_size=S,
                          max_batch=1, rpn_post_nms_top_n=P, large_sep_train=True, exit_flow_train=True)
    with plain.scope():
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_train()
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_backward(run['d_out_t'])
        with pytest.raises(InvalidArgumentError):
            plain.exit_flow_saved()
    fresh = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, large_sep_train=True, exit_flow_train=True)
    with fresh.scope():
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_backward(run['d_out_t'])                                  # no training forward has run
        with pytest.raises(InvalidArgumentError):
            fresh.exit_flow_saved()
    with det.scope():
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_backward(DeviceTensor.empty((2, 8, 8, 2048)))
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_backward(DeviceTensor.empty((2, 16, 16, 2048), ld=2048 + 32))     # another ld
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_backward(run['d_out'])                                        # not on the device
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_backward(run['d_out_t'], run['d_mid'])                        # d_mid not on the device
        with pytest.raises(InvalidArgumentError):
            M.exit_flow_backward(run['d_out_t'], DeviceTensor.empty((2, 16, 16, 728), ld=728))


def test_conditions_from_the_float64_statements(run, lh_weights):
    """what the masks of the chain rely on, from float64 statements of each stage fed the GPU's upstream tensors: both sides
    of every ReLU are populated and every batch variance is positive"""
    from xdet.ops import host_batch_norm_forward
    w = lh_weights
    assert (run['mid_x'] > 0).any() and (run['mid_x'] <= 0).any()
    for name, dil, relu_in, relu_out, x, _ in units(run, w):
        t = depthwise_forward64(x, w[name + '/depthwise_kernel'], dil, relu_in)
        z = CC.conv_forward64(t, w[name + '/pointwise_kernel'], False)
        y, _, invstd, _, _ = host_batch_norm_forward(z, w[name + '_bn/gamma'], w[name + '_bn/beta'], EPS, True, MOMENTUM, None, None,
                                                     relu_out, f64)
        assert (1. / invstd ** 2 - EPS > 0).all(), name
        if relu_out:
            assert (y == 0).any() and (y > 0).any(), name
        else:
            assert (y <= 0).any() and (y > 0).any(), name
    z = CC.conv_forward64(run['mid_x'], w['conv2d_4/kernel'], False)
    assert (z.reshape(-1, z.shape[-1]).var(axis=0) > 0).all()


def test_training_forward(run, lh_weights):
    w, sv = lh_weights, run['saved']
    worst = {}
    for name, dil, relu_in, relu_out, x, y in units(run, w):
        C, J = w[name + '/pointwise_kernel'].shape[2:]
        assert sv[name + '/dw'].shape == (2, 16, 16, C) and sv[name + '/z'].shape == (2, 16, 16, J) and y.shape == (2, 16, 16, J)
        close(name + ' depthwise', sv[name + '/dw'], depthwise_forward64(x, w[name + '/depthwise_kernel'], dil, relu_in),
              DEPTHWISE_FORWARD_TOL, show=True)
        close(name + ' pointwise', sv[name + '/z'], CC.conv_forward64(sv[name + '/dw'], w[name + '/pointwise_kernel'], False),
              CONV_FORWARD_TOL, show=True)
        bn = name + '_bn/'
        d = bn_forward_distances(sv[name + '/z'], w[bn + 'gamma'], w[bn + 'beta'], w[bn + 'moving_mean'], w[bn + 'moving_variance'],
                                 (y, sv[bn + 'save_mean'], sv[bn + 'save_invstd'], sv[bn + 'moving_mean'], sv[bn + 'moving_variance']),
                                 relu=relu_out, eps=EPS, momentum=MOMENTUM)
        print('%s batch norm forward: distance / bar = %s' % (name, ', '.join('%s %.4f' % (k, v / BC.bar()) for k, v in sorted(d.items()))))
        assert max(d.values()) <= BC.bar(), (name, d)
        worst[name] = max(d.values()) / BC.bar()
        assert not np.array_equal(sv[bn + 'moving_mean'].reshape(-1), w[bn + 'moving_mean'])
        if relu_out:
            assert (y == 0).any() and (y > 0).any()
    close('conv2d_4', sv['conv2d_4/z'], CC.conv_forward64(run['mid_x'], w['conv2d_4/kernel'], False), CONV_FORWARD_TOL, show=True)
    bn = 'batch_normalization_4/'
    d = bn_forward_distances(sv['conv2d_4/z'], w[bn + 'gamma'], w[bn + 'beta'], w[bn + 'moving_mean'], w[bn + 'moving_variance'],
                             (sv['r'], sv[bn + 'save_mean'], sv[bn + 'save_invstd'], sv[bn + 'moving_mean'], sv[bn + 'moving_variance']),
                             eps=EPS, momentum=MOMENTUM)
    print('batch_normalization_4 forward: distance / bar = %s' % ', '.join('%s %.4f' % (k, v / BC.bar()) for k, v in sorted(d.items())))
    assert max(d.values()) <= BC.bar(), d
    print('batch norm forward, worst distance / bar: %.4f' % max(list(worst.values()) + [max(d.values()) / BC.bar()]))
    # the join: numpy's f32 add of the GPU's own addends
    assert np.array_equal(bits(sv['b2']), bits(sv['y2'] + sv['r']))


def test_the_chain(run, lh_weights):
    """every backward step against its statement fed the gradient the GPU left upstream"""
    from xdet.ops import host_depthwise_backward
    w, sv, g = lh_weights, run['saved'], run['grads']
    assert run['d_out'].any() and run['d_mid'].any()
    dys = {'block14_sepconv2': run['d_out'], 'block14_sepconv1': g['c3'], 'block13_sepconv2': g['b2'], 'block13_sepconv1': g['a']}
    dxs = {'block14_sepconv2': g['c3'], 'block14_sepconv1': g['b2'], 'block13_sepconv2': g['a'], 'block13_sepconv1': g['mid_B']}
    worst = {'bn': 0., 'pointwise': 0., 'depthwise dw': 0.}

    def bn_backward(name, z_name, mask, dy, got):
        c = dict(x=sv[z_name], dy=dy, gamma=w[name + '/gamma'], relu=mask is not None)
        d = BC.backward_distances(c, True, mask, sv[name + '/save_mean'].reshape(-1), sv[name + '/save_invstd'].reshape(-1), got)
        print('%s backward: distance / bar = %s' % (name, ', '.join('%s %.4f' % (k, v / BC.bar()) for k, v in sorted(d.items()))))
        assert max(d.values()) <= BC.bar(), (name, d)
        worst['bn'] = max(worst['bn'], max(d.values()) / BC.bar())

    def pointwise_backward(name, x, k, dy, got_dx, got_dw):
        ref, den = CC.reference64(x, k, dy, None, False)
        d = CC.distances((got_dx, got_dw, None), ref, den)
        print('%s backward: distance / bar = %s' % (name, ', '.join('%.4f' % (v / CC.bar()) for v in d)))
        assert max(d) <= CC.bar(), (name, d)
        worst['pointwise'] = max(worst['pointwise'], max(d) / CC.bar())

    for name, dil, relu_in, relu_out, x, y in units(run, w):
        bn_backward(name + '_bn', name + '/z', y if relu_out else None, dys[name],
                    (g['z/' + name], g[name + '_bn/gamma'], g[name + '_bn/beta']))
        pointwise_backward(name + '/pointwise', sv[name + '/dw'], w[name + '/pointwise_kernel'], g['z/' + name], g['dw/' + name],
                           g[name + '/pointwise_kernel'])
        kd = w[name + '/depthwise_kernel']
        want_dx = host_depthwise_backward(x, kd, g['dw/' + name], dil, relu_in)[0]
        assert np.array_equal(dxs[name], want_dx), name
        (_, ref_dw), den = DC.reference64(x, kd, g['dw/' + name], dil, relu_in)
        d = DC.dw_distance(g[name + '/depthwise_kernel'], ref_dw, den)
        print('%s/depthwise backward: dx equal, dw distance / bar = %.4f' % (name, d / DC.bar()))
        assert d <= DC.bar(), (name, d / DC.bar())
        worst['depthwise dw'] = max(worst['depthwise dw'], d / DC.bar())
    # d loss / d b2 also goes through the projection branch: share A
    bn_backward('batch_normalization_4', 'conv2d_4/z', None, g['b2'],
                (g['z/conv2d_4'], g['batch_normalization_4/gamma'], g['batch_normalization_4/beta']))
    pointwise_backward('conv2d_4', run['mid_x'], w['conv2d_4/kernel'], g['z/conv2d_4'], g['mid_A'], g['conv2d_4/kernel'])
    assert np.array_equal(bits(g['r']), bits(g['b2']))
    print('worst distance / bar: %s' % ', '.join('%s %.4f' % kv for kv in sorted(worst.items())))
    # the join, in its order: numpy's f32 adds of the GPU's own addends
    assert np.array_equal(bits(g['mid']), bits((g['mid_B'] + g['mid_A']) + run['d_mid']))
    assert np.array_equal(bits(run['no_mid']['mid']), bits(g['mid_B'] + g['mid_A']))
    assert not g['mid_B'][~(run['mid_x'] > 0)].any() and g['mid_A'][~(run['mid_x'] > 0)].any()


def test_gradients(run, lh_weights):
    from xdet.model import EXIT_FLOW_VARIABLES
    g = run['grads']
    names = {'%s/%s' % (u, v) for u in ('block13_sepconv1', 'block13_sepconv2', 'block14_sepconv1', 'block14_sepconv2')
             for v in ('depthwise_kernel', 'pointwise_kernel')}
    names |= {'%s_bn/%s' % (u, v) for u in ('block13_sepconv1', 'block13_sepconv2', 'block14_sepconv1', 'block14_sepconv2')
              for v in ('gamma', 'beta')}
    names |= {'conv2d_4/kernel', 'batch_normalization_4/gamma', 'batch_normalization_4/beta'}
    assert set(EXIT_FLOW_VARIABLES) == names and names <= set(g) and {'mid', 'b2', 'c3', 'a', 'r'} <= set(g)
    for k in names:
        assert g[k].shape == lh_weights[k].shape and g[k].dtype == f32 and np.isfinite(g[k]).all() and g[k].any(), k
    shape, ld = run['mid_grad_shape_ld']
    assert (shape, ld) == run['mid_shape_ld'] and shape == (2, 16, 16, 728)
    assert g['b2'].shape == (2, 16, 16, 1024) and g['c3'].shape == (2, 16, 16, 1536) and g['a'].shape == (2, 16, 16, 728)
    for k in g:
        assert np.array_equal(bits(g[k]), bits(run['again'][k])), k
    for k in g:
        if k not in ('mid',):
            assert np.array_equal(bits(g[k]), bits(run['no_mid'][k])), k
