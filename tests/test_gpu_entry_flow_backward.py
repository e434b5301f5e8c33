"""Blocks 2-4 of the Xception entry flow in training mode through the net (LightHeadDetector(entry_flow_train=True),
model.entry_flow_train, model.entry_flow_backward), on the path of tests/test_gpu_middle_flow_backward.py and at its sizes:
S = 256, two images, a detector built in split precision (f16x3), one pass -- eval body, entry_flow_train, middle_flow_train,
the RPN, the training exit flow and large-separable block, head loss and backward, large_sep_backward, RPN loss and backward,
exit_flow_backward, middle_flow_backward, entry_flow_backward -- and every step judged against its float64 statement fed the
tensors the GPU left upstream, so one check measures one step.  At S = 256 the maps are 125 -> 63 -> 32 -> 16: odd, odd, even,
the parities of the 480-pixel net (237 -> 119 -> 60 -> 30).
Bars, all the project's own: depthwise forwards 1e-6 of the output scale, pointwise and projection forwards 3e-5, the batch
norms batch_norm_cases.bar() at eps 1e-4 / momentum 0.99, pointwise and projection backwards conv_backward_cases.bar(),
depthwise backwards the dx equality and depthwise_backward_cases.bar() for dw.  The subsampled inputs, the three pool + add
steps, the three pool backwards and the three joins are bit-equal to NumPy on the GPU's own tensors: a max pool chooses, and
across precisions a choice between two nearly equal values may fall either way (the share of such windows is printed by the
conditions test), so that step is judged on the very tensor the GPU pooled.
Measured on an MI355X, worst fraction of each bar per op class (every test prints its own with -s): depthwise forwards 0.13,
pointwise forwards 0.010, projection forwards 0.012, batch norm forward 0.018, backward 0.0035; pointwise backwards 0.31,
projection backwards 0.21; depthwise backwards: dx equal everywhere, dw 0.046; the eval entry flow from the GPU's stem_out
0.016 of the stage bar; conditions: positive share 0.50-0.89, smallest batch variance 6.87e-4, |entry_x| <= 7.3, pool windows
with a near tie 2.0e-6 of block 2's, none of block 3's and 4's."""
import numpy as np
import pytest

import batch_norm_cases as BC
import conv_backward_cases as CC
import depthwise_backward_cases as DC

from flow_train_cases import S, P, NC, bits, rel_err, close, depthwise_forward64, bn_forward_distances, head_and_rpn_inputs, downstream

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DEPTHWISE_FORWARD_TOL = 1e-6     # tests/test_gpu_layers.py::test_depthwise_matches_oracle
CONV_FORWARD_TOL = 3e-5          # tests/test_gpu_layers.py::test_conv_matches_oracle, f16x3
STAGE_TOL = 1e-4                 # tests/test_gpu_e2e.py::test_dense_stages
EPS, MOMENTUM = 1e-4, 0.99       # the Xception layers' batch norm (model.ENTRY_FLOW_EPS / _MOMENTUM)
BLOCKS = (2, 3, 4)
MAPS = {2: (125, 64, 128), 3: (63, 128, 256), 4: (32, 256, 728)}      # block: (input extent, input channels, width)
UPPER = dict(pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True, middle_flow_train=True)
TRAIN = dict(UPPER, entry_flow_train=True)


def relu_in(b, i):
    return not (b == 2 and i == 1)


@pytest.fixture(scope='module')
def run(lh_weights):
    """one pass over the whole path; the tests below look at what it left"""
    from xdet import model as M, weights as W, InvalidArgumentError
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
        upper = LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **UPPER)     # keeps entry_x, not stem_out
        det = LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
    finally:
        set_precision(before)
    with plain.scope():
        _, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['plain_out'], r['plain_mid_x'] = out.numpy(), plain.buffer('mid_x', 2).numpy()
    with upper.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['upper_entry_x'] = upper.buffer('entry_x', 2).numpy()
    r['plain'], r['upper'], r['det'] = plain, upper, det
    with det.scope():
        mid, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['eval_out'], r['eval_mid_x'], r['eval_entry_x'] = out.numpy(), det.buffer('mid_x', 2).numpy(), det.buffer('entry_x', 2).numpy()
        stem = det.buffer('stem_out', 2)
        r['stem_out'], r['stem_shape_ld'] = stem.numpy(), (stem.shape, stem.ld)
        M.middle_flow_train()                        # (on the eval-mode entry_x: the state entry_flow_train has to drop)
        entry_t = M.entry_flow_train()
        entry = det.buffer('entry_x', 2)
        r['entry_is_the_buffer'] = entry_t.ptr == entry.ptr and entry_t.ld == entry.ld and entry_t.shape == entry.shape
        r['entry_x'], r['entry_shape_ld'] = entry.numpy(), (entry.shape, entry.ld)
        r['saved'] = {k: v.numpy() for k, v in det.entry_flow_saved().items()}
        mid_x = det.buffer('mid_x', 2)
        with pytest.raises(InvalidArgumentError):    # what middle_flow_train saved belongs to the eval-mode entry_x
            M.middle_flow_backward(DeviceTensor.empty(mid_x.shape, ld=mid_x.ld))
        mid_t = M.middle_flow_train()
        lsep, rpn = downstream(M.exit_flow_train(), mid_t, inputs)
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'])
        mf = M.middle_flow_backward(ef['mid'])
        r['d_entry_t'], r['d_entry'] = mf['entry'], mf['entry'].numpy()
        host = lambda g: {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in g.items()}
        grads = M.entry_flow_backward(mf['entry'], intermediates=True)
        r['stem_grad_shape_ld'] = (grads['stem'].shape, grads['stem'].ld)
        r['grads'] = host(grads)
        r['again'] = host(M.entry_flow_backward(mf['entry'], intermediates=True))
        r['lean'] = host(M.entry_flow_backward(mf['entry']))
        r['stem_out_after'] = det.buffer('stem_out', 2).numpy()
        r['entry_x_after'] = det.buffer('entry_x', 2).numpy()
    return r


def units(run):
    """per unit: (name, block, index, the unit's input and output as the GPU left them)"""
    sv = run['saved']
    out = []
    for b in BLOCKS:
        ins = (sv['x%d' % b], sv['block%d/y1' % b])
        outs = (sv['block%d/y1' % b], sv['block%d/y2' % b])
        out += [('block%d_sepconv%d' % (b, i + 1), b, i + 1, ins[i], outs[i]) for i in range(2)]
    return out


def test_default_path_unchanged(run):
    """the options change nothing in the eval body: `out`, `mid_x` and `entry_x` keep their bits; the plain nets refuse the name"""
    from xdet import InvalidArgumentError
    assert run['plain_out'].shape == (2, 16, 16, 2048) and run['plain_out'].any()
    assert np.array_equal(bits(run['eval_out']), bits(run['plain_out']))
    assert np.array_equal(bits(run['eval_mid_x']), bits(run['plain_mid_x']))
    assert run['upper_entry_x'].any() and np.array_equal(bits(run['eval_entry_x']), bits(run['upper_entry_x']))
    for d in (run['plain'], run['upper']):
        with pytest.raises(InvalidArgumentError, match='stem_out=keep'):
            d.buffer('stem_out', 2)


def test_stem_out_survives_and_is_the_entry_flows_input(run, oracle, lh_weights):
    """the eval entry flow in NumPy (the oracle's layers) from the GPU's stem_out against the GPU's eval entry_x"""
    assert run['stem_shape_ld'] == ((2, 125, 125, 64), 64) and run['stem_out'].any() and (run['stem_out'] >= 0).all()
    assert np.array_equal(bits(run['stem_out_after']), bits(run['stem_out']))
    O, w, x = oracle, lh_weights, run['stem_out']
    for b in BLOCKS:
        res = O.batch_norm(O.conv2d(x, w['conv2d_%d/kernel' % (b - 1)], 2, 'SAME'), w, 'batch_normalization_%d' % (b - 1), EPS)
        x = O._sep_bn(x, w, 'block%d_sepconv1' % b, pre_relu=relu_in(b, 1))
        x = O._sep_bn(x, w, 'block%d_sepconv2' % b)
        x = O.max_pool_3x3_s2_same(x) + res
    e = rel_err(run['eval_entry_x'], x)
    print('eval entry_x from the GPU\'s stem_out: rel_err / bar = %.4f' % (e / STAGE_TOL))
    assert e < STAGE_TOL


def test_conditions_from_the_float64_statements(run, lh_weights):
    """what the masks and the pool's choices rely on, from float64 statements of each unit fed the GPU's upstream tensors: both
    sides of every ReLU are populated, every batch variance is well above zero; and, recorded only, the share of pool windows
    whose two largest values lie within 2^-20 of the maximum's magnitude -- windows where another precision may choose another
    pixel, which is why the pool steps are judged on the GPU's own tensor"""
    from xdet.ops import host_batch_norm_forward
    w, sv = lh_weights, run['saved']
    share, var_min, near = [], np.inf, {}
    for name, b, i, x, _ in units(run):
        if relu_in(b, i):
            share.append(float((x > 0).mean()))
        t = depthwise_forward64(x, w[name + '/depthwise_kernel'], relu_in=relu_in(b, i))
        z = CC.conv_forward64(t, w[name + '/pointwise_kernel'], False)
        y, _, invstd, _, _ = host_batch_norm_forward(z, w[name + '_bn/gamma'], w[name + '_bn/beta'], EPS, True, MOMENTUM, None, None,
                                                     False, f64)
        var_min = min(var_min, float((1. / invstd ** 2 - EPS).min()))
        if i == 2:
            y = np.asarray(y, f64).reshape(x.shape[:3] + (-1,))
            N, H, W, C = y.shape
            Ho, Wo, pt, pl = (H + 1) // 2, (W + 1) // 2, H % 2, W % 2
            yp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf)
            yp[:, pt:pt + H, pl:pl + W] = y
            top = np.sort(np.stack([yp[:, a:a + 2 * Ho:2, c:c + 2 * Wo:2] for a in range(3) for c in range(3)], -1), -1)[..., -2:]
            near[b] = float((top[..., 1] - top[..., 0] <= 2.0 ** -20 * np.abs(top[..., 1])).mean())
    for b in BLOCKS:
        z = CC.conv_forward64(sv['block%d/xs' % b], w['conv2d_%d/kernel' % (b - 1)], False)
        bn = 'batch_normalization_%d/' % (b - 1)
        _, _, invstd, _, _ = host_batch_norm_forward(z, w[bn + 'gamma'], w[bn + 'beta'], EPS, True, MOMENTUM, None, None, False, f64)
        var_min = min(var_min, float((1. / invstd ** 2 - EPS).min()))
    print('positive share %.2f-%.2f, smallest batch variance %.2e, |entry_x| <= %.1f, windows with a near tie: %s'
          % (min(share), max(share), var_min, np.abs(run['entry_x']).max(), ', '.join('block %d %.2e' % kv for kv in sorted(near.items()))))
    # both sides of a mask must be a real share of the tensor for the test to see a wrong mask, and a batch variance must stay
    # far above the rounding of the f32 sums it is made of (2^-24 of values of order 1)
    assert 0.05 <= min(share) and max(share) <= 0.95
    assert var_min >= 1e-6


def test_training_forward(run, oracle, lh_weights):
    w, sv = lh_weights, run['saved']
    worst = {'depthwise': 0., 'pointwise': 0., 'projection': 0., 'bn': 0.}

    def judge_bn(what, z, bn, y):
        d = bn_forward_distances(z, w[bn + 'gamma'], w[bn + 'beta'], w[bn + 'moving_mean'], w[bn + 'moving_variance'],
                                 (y, sv[bn + 'save_mean'], sv[bn + 'save_invstd'], sv[bn + 'moving_mean'], sv[bn + 'moving_variance']),
                                 eps=EPS, momentum=MOMENTUM)
        assert max(d.values()) <= BC.bar(), (what, d)
        worst['bn'] = max(worst['bn'], max(d.values()) / BC.bar())
        assert not np.array_equal(sv[bn + 'moving_mean'].reshape(-1), w[bn + 'moving_mean'])
        assert not np.array_equal(sv[bn + 'moving_variance'].reshape(-1), w[bn + 'moving_variance'])
    assert np.array_equal(bits(sv['x2']), bits(run['stem_out']))
    for b in BLOCKS:
        ext, cin, c = MAPS[b]
        half = (ext + 1) // 2
        x, proj = sv['x%d' % b], 'conv2d_%d' % (b - 1)
        assert x.shape == (2, ext, ext, cin) and sv['block%d/y2' % b].shape == (2, ext, ext, c)
        assert sv['block%d/xs' % b].shape == (2, half, half, cin) and sv['block%d/r' % b].shape == (2, half, half, c)
        assert np.array_equal(bits(sv['block%d/xs' % b]), bits(x[:, ::2, ::2])), b
        worst['projection'] = max(worst['projection'], close(proj, sv[proj + '/z'],
                                                             CC.conv_forward64(sv['block%d/xs' % b], w[proj + '/kernel'], False), CONV_FORWARD_TOL))
        judge_bn(proj, sv[proj + '/z'], 'batch_normalization_%d/' % (b - 1), sv['block%d/r' % b])
        # pool + add: NumPy's f32 max and add of the GPU's own y2 and r
        want = oracle.max_pool_3x3_s2_same(sv['block%d/y2' % b]) + sv['block%d/r' % b]
        assert want.dtype == f32 and np.array_equal(bits(sv['x%d' % (b + 1)]), bits(want)), b
    for name, b, i, x, y in units(run):
        worst['depthwise'] = max(worst['depthwise'], close(name + ' depthwise', sv[name + '/dw'],
                                                           depthwise_forward64(x, w[name + '/depthwise_kernel'], relu_in=relu_in(b, i)),
                                                           DEPTHWISE_FORWARD_TOL))
        worst['pointwise'] = max(worst['pointwise'], close(name + ' pointwise', sv[name + '/z'],
                                                           CC.conv_forward64(sv[name + '/dw'], w[name + '/pointwise_kernel'], False),
                                                           CONV_FORWARD_TOL))
        judge_bn(name, sv[name + '/z'], name + '_bn/', y)
    print('training forward, worst fraction of the bar: %s' % ', '.join('%s %.4f' % kv for kv in sorted(worst.items())))
    # block 4's output is the net's entry_x, and it is not the eval-mode tensor any more
    assert run['entry_is_the_buffer'] and run['entry_shape_ld'] == ((2, 16, 16, 728), 736)
    assert np.array_equal(bits(sv['x5']), bits(run['entry_x'])) and not np.array_equal(run['entry_x'], run['eval_entry_x'])
    assert np.array_equal(bits(run['entry_x_after']), bits(run['entry_x']))


def test_the_chain(run, lh_weights):
    """every backward step against its statement fed the gradient the GPU left upstream"""
    from xdet.ops import host_depthwise_backward, host_max_pool_backward, host_add_upsample2
    w, sv, g = lh_weights, run['saved'], run['grads']
    assert run['d_entry'].any()
    worst = {'bn': 0., 'pointwise': 0., 'projection': 0., 'depthwise dw': 0.}

    def judge_bn(what, z, dy, bn, dz):
        d = BC.backward_distances(dict(x=z, dy=dy, gamma=w[bn + '/gamma'], relu=False), True, None,
                                  sv[bn + '/save_mean'].reshape(-1), sv[bn + '/save_invstd'].reshape(-1),
                                  (dz, g[bn + '/gamma'], g[bn + '/beta']))
        assert max(d.values()) <= BC.bar(), (what, d)
        worst['bn'] = max(worst['bn'], max(d.values()) / BC.bar())

    def judge_conv(what, key, x, kname, dz, dx):
        ref, den = CC.reference64(x, w[kname], dz, None, False)
        d = CC.distances((dx, g[kname], None), ref, den)
        assert max(d) <= CC.bar(), (what, d)
        worst[key] = max(worst[key], max(d) / CC.bar())
    for b in reversed(BLOCKS):
        g_out = g['x%d' % (b + 1)] if b != BLOCKS[-1] else run['d_entry']
        proj, x = 'conv2d_%d' % (b - 1), sv['x%d' % b]
        judge_bn(proj, sv[proj + '/z'], g_out, 'batch_normalization_%d' % (b - 1), g['z/' + proj])
        judge_conv(proj, 'projection', sv['block%d/xs' % b], proj + '/kernel', g['z/' + proj], g['dxs/block%d' % b])
        dy2 = g['dy2/block%d' % b]
        assert dy2.any() and np.array_equal(bits(dy2), bits(host_max_pool_backward(sv['block%d/y2' % b], g_out))), b
        for i, xin, dy in ((2, sv['block%d/y1' % b], dy2), (1, x, g['d2/block%d' % b])):
            name = 'block%d_sepconv%d' % (b, i)
            judge_bn(name, sv[name + '/z'], dy, name + '_bn', g['z/' + name])
            judge_conv(name, 'pointwise', sv[name + '/dw'], name + '/pointwise_kernel', g['z/' + name], g['dw/' + name])
            kd, dx = w[name + '/depthwise_kernel'], g['d%d/block%d' % (i, b)]
            assert np.array_equal(dx, host_depthwise_backward(xin, kd, g['dw/' + name], 1, relu_in(b, i))[0]), name
            (_, ref_dw), den = DC.reference64(xin, kd, g['dw/' + name], 1, relu_in(b, i))
            d = DC.dw_distance(g[name + '/depthwise_kernel'], ref_dw, den)
            assert d <= DC.bar(), (name, d / DC.bar())
            worst['depthwise dw'] = max(worst['depthwise dw'], d / DC.bar())
        # the join: the units' share everywhere, the shortcut's on the even pixels
        got, d1, dxs = g['stem' if b == BLOCKS[0] else 'x%d' % b], g['d1/block%d' % b], g['dxs/block%d' % b]
        assert dxs.any() and np.array_equal(bits(got), bits(host_add_upsample2(d1, dxs))), b
        assert not np.array_equal(got[:, ::2, ::2], d1[:, ::2, ::2])
    print('the chain, worst fraction of the bar: %s' % ', '.join('%s %.4f' % kv for kv in sorted(worst.items())))


def test_gradients(run, lh_weights):
    from xdet.model import ENTRY_FLOW_VARIABLES, ENTRY_FLOW_UNITS
    g, lean = run['grads'], run['lean']
    names = set(ENTRY_FLOW_VARIABLES)
    assert len(names) == 33 and len(ENTRY_FLOW_UNITS) == 6
    assert names == {'conv2d_%d/kernel' % k for k in (1, 2, 3)} | \
        {'batch_normalization_%d/%s' % (k, v) for k in (1, 2, 3) for v in ('gamma', 'beta')} | \
        {u + v for u in ENTRY_FLOW_UNITS for v in ('/depthwise_kernel', '/pointwise_kernel', '_bn/gamma', '_bn/beta')}
    assert set(lean) == names | {'stem', 'x3', 'x4'}
    assert set(g) >= set(lean) | {'dw/' + u for u in ENTRY_FLOW_UNITS} | {'z/' + u for u in ENTRY_FLOW_UNITS} | \
        {'%s/block%d' % (k, b) for b in BLOCKS for k in ('dxs', 'dy2', 'd2', 'd1')} | {'z/conv2d_%d' % k for k in (1, 2, 3)}
    for k in names:
        assert g[k].shape == lh_weights[k].shape and g[k].dtype == f32 and np.isfinite(g[k]).all() and g[k].any(), k
    assert run['stem_grad_shape_ld'] == run['stem_shape_ld'] and g['stem'].any()
    assert g['x3'].shape == (2, 63, 63, 128) and g['x4'].shape == (2, 32, 32, 256)
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
    with pytest.raises(InvalidArgumentError, match='middle_flow_train'):
        LightHeadDetector(lh_weights, large_sep_train=True, exit_flow_train=True, entry_flow_train=True, **kw)
    with pytest.raises(InvalidArgumentError, match='batch_normalization_2/moving_variance'):
        LightHeadDetector({k: v for k, v in lh_weights.items() if k != 'batch_normalization_2/moving_variance'},
                          large_sep_train=True, exit_flow_train=True, middle_flow_train=True, entry_flow_train=True, **kw)
    for d in (plain, run['upper']):
        with d.scope():
            with pytest.raises(InvalidArgumentError):
                M.entry_flow_train()
            with pytest.raises(InvalidArgumentError):
                M.entry_flow_backward(run['d_entry_t'])
            with pytest.raises(InvalidArgumentError):
                d.entry_flow_saved()
    fresh = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
    with fresh.scope():
        with pytest.raises(InvalidArgumentError):
            M.entry_flow_train()                                                      # no body has run
        with pytest.raises(InvalidArgumentError):
            M.entry_flow_backward(run['d_entry_t'])                                   # no training forward has run
        with pytest.raises(InvalidArgumentError):
            fresh.entry_flow_saved()
    with det.scope():
        with pytest.raises(InvalidArgumentError):
            M.entry_flow_backward(DeviceTensor.empty((2, 8, 8, 728)))
        with pytest.raises(InvalidArgumentError):
            M.entry_flow_backward(DeviceTensor.empty((2, 16, 16, 728), ld=728))        # another ld
        with pytest.raises(InvalidArgumentError):
            M.entry_flow_backward(run['d_entry'])                                     # not on the device
        # (the fixture has shown middle_flow_backward refusing between entry_flow_train and a new middle_flow_train)
