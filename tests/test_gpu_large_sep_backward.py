"""The large-separable block in training mode through the net (LightHeadDetector(large_sep_train=True),
model.large_sep_kernel(..., is_training=True), model.large_sep_backward), on the path of
tests/test_gpu_conv_backward.py::test_rpn_backward_through_the_net: every stage is judged against its float64 statement fed
the tensors the GPU left upstream.  The forward convs keep the f16x3 bar of tests/test_gpu_layers.py (3e-5 of the output
scale), the batch norm the bar of tests/batch_norm_cases.py, the two conv backwards conv_backward_cases.bar().
Measured on an MI355X, worst fraction of each bar: forward convs 0.14 (t) and 0.09 (z); batch norm forward 0.005 (var),
backward 0.003 (dgamma); conv2d_1's backward 0.47 (dx), conv2d's 0.35 (dW)."""
import numpy as np
import pytest

import batch_norm_cases as BC
import conv_backward_cases as CC

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
S, P, NC, MID, CO = 256, 64, 21, 256, 490
CONV_FORWARD_TOL = 3e-5          # tests/test_gpu_layers.py::test_conv_matches_oracle, f16x3


def bits(a):
    return np.asarray(a).view(np.uint32)


def close(what, a, b, tol):
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    print('%s: error / (tol * scale) = %.4f' % (what, err / (tol * scale)))
    assert err <= tol * scale, (what, err, scale)


@pytest.fixture(scope='module')
def run(lh_weights):
    """one pass over the whole path; the tests below look at what it left"""
    from xdet import model as M, losses as L, weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import to_host
    r = {}
    images = W.synthetic_images(2, S, seed=3)
    rng = np.random.default_rng(11)
    ctr, hw = rng.uniform(0.25, 0.75, (2, P, 2)), rng.uniform(0.1, 0.4, (2, P, 2))
    rois = np.concatenate([ctr - hw / 2, ctr + hw / 2], -1).astype(f32)
    labels = rng.integers(-1, NC, (2, P)).astype(np.int32)
    targets = (rng.standard_normal((2, P, 4)) * 0.2).astype(f32)

    plain = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, pool_index=True)
    with plain.scope():
        _, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['plain_feat'] = M.large_sep_kernel(out, MID, CO, False, 'channels_first', 'large_sep_feature').numpy()
    r['plain'] = plain
    det = LightHeadDetector(lh_weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, pool_index=True, large_sep_train=True)
    r['det'] = det
    with det.scope():
        _, out = M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        r['out'] = out.numpy()
        r['out_ld'] = out.ld
        r['eval_feat'] = M.large_sep_kernel(out, MID, CO, False, 'channels_first', 'large_sep_feature').numpy()
        feat = M.large_sep_kernel(out, MID, CO, True, 'channels_first', 'large_sep_feature')
        r['feat'], r['feat_ld'] = feat.numpy(), feat.ld
        r['saved'] = {k: v.numpy() for k, v in det.large_sep_saved().items()}
        loss_func = L.HeadLoss(labels, targets, 0.25)
        M.get_head(feat, None, 7, 7, loss_func, rois, NC, True, True, 32, 'channels_first', 'final_head')
        head = M.head_backward(loss_func, to_feat=True)
        r['d_feat_t'] = head['feat']
        r['d_feat'] = head['feat'].numpy()
        grads = M.large_sep_backward(head['feat'])
        r['grads'] = {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in grads.items()}
        r['d_out_raw'] = to_host(grads['out'].ptr, (2, 16, 16, grads['out'].ld))
        r['d_out_shape_ld'] = (grads['out'].shape, grads['out'].ld)
        again = M.large_sep_backward(head['feat'])
        # what the backward read is what the forward read: the head did not recycle the block's input or output
        assert np.array_equal(bits(det.buffer('out', 2).numpy()), bits(r['out']))
        assert np.array_equal(bits(det.buffer('feat', 2).numpy()), bits(r['feat']))
        r['again'] = {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in again.items()}
    return r


def test_default_path_unchanged(run):
    assert run['plain_feat'].shape == (2, 16, 16, CO) and run['plain_feat'].any()
    assert np.array_equal(bits(run['eval_feat']), bits(run['plain_feat']))


def test_refusals(run, lh_weights):
    from xdet import model as M, InvalidArgumentError
    from xdet.runtime import DeviceTensor
    plain, det = run['plain'], run['det']
    with plain.scope():
        with pytest.raises(InvalidArgumentError):
            M.large_sep_kernel(plain.buffer('out', 2), MID, CO, True, 'channels_first', 'large_sep_feature')
        with pytest.raises(InvalidArgumentError):
            M.large_sep_backward(run['d_feat_t'])
        with pytest.raises(InvalidArgumentError):
            plain.large_sep_saved()
    with det.scope():
        with pytest.raises(InvalidArgumentError):
            M.large_sep_backward(DeviceTensor.empty((2, 8, 8, CO)))
        with pytest.raises(InvalidArgumentError):
            M.large_sep_backward(DeviceTensor.empty((2, 16, 16, CO), ld=CO))       # another ld
        with pytest.raises(InvalidArgumentError):
            M.large_sep_backward(run['d_feat'])                                    # not on the device


@pytest.fixture(scope='module')
def merged(lh_weights):
    from xdet.model import merge_large_sep
    return merge_large_sep(lh_weights)


def test_training_forward(run, merged, lh_weights):
    ka, ba, kb, bb = merged
    sv = run['saved']
    assert sv['t'].shape == (2, 16, 16, 2 * MID) and sv['z'].shape == (2, 16, 16, CO)
    close('t', sv['t'], CC.conv_forward64(run['out'], ka, False) + ba, CONV_FORWARD_TOL)
    close('z', sv['z'], CC.conv_forward64(sv['t'], kb, False) + bb, CONV_FORWARD_TOL)
    bn = 'large_sep_feature/batch_normalization/'
    c = dict(x=sv['z'], gamma=lh_weights[bn + 'gamma'], beta=lh_weights[bn + 'beta'], moving_mean=lh_weights[bn + 'moving_mean'],
             moving_var=lh_weights[bn + 'moving_variance'], relu=True)
    feat = run['feat']
    assert feat.shape == (2, 16, 16, CO) and (feat == 0).any() and (feat > 0).any()
    d = BC.forward_distances(c, True, (feat, sv['save_mean'].reshape(-1), sv['save_invstd'].reshape(-1),
                                       sv['moving_mean'].reshape(-1), sv['moving_variance'].reshape(-1)))
    print('batch norm forward: distance / bar = %s' % ', '.join('%s %.4f' % (k, v / BC.bar()) for k, v in sorted(d.items())))
    assert max(d.values()) <= BC.bar(), d
    assert not np.array_equal(sv['moving_mean'].reshape(-1), lh_weights[bn + 'moving_mean'])


def test_the_chain(run, merged, lh_weights):
    ka, ba, kb, bb = merged
    sv, g = run['saved'], run['grads']
    d_feat = run['d_feat']
    assert d_feat.any() and g['z'].shape == (2, 16, 16, CO) and g['t'].shape == (2, 16, 16, 2 * MID)
    bn = 'large_sep_feature/batch_normalization/'
    # the batch norm and its ReLU, masked by the net's own feat
    c = dict(x=sv['z'], dy=d_feat, gamma=lh_weights[bn + 'gamma'], relu=True)
    d = BC.backward_distances(c, True, run['feat'], sv['save_mean'].reshape(-1), sv['save_invstd'].reshape(-1),
                              (g['z'], g[bn + 'gamma'], g[bn + 'beta']))
    print('batch norm backward: distance / bar = %s' % ', '.join('%s %.4f' % (k, v / BC.bar()) for k, v in sorted(d.items())))
    assert max(d.values()) <= BC.bar(), d
    # the merged (1,15) conv: its dy is d loss / d z as the GPU left it
    p0, p1 = 'large_sep_feature/Branch_0/', 'large_sep_feature/Branch_1/'
    dkb = np.concatenate([g[p0 + 'conv2d_1/kernel'], g[p1 + 'conv2d_1/kernel']], axis=2)
    ref, den = CC.reference64(sv['t'], kb, g['z'], None, False)
    d = CC.distances((g['t'], dkb, g[p0 + 'conv2d_1/bias']), ref, den)
    print('conv2d_1: distance / bar = %s' % ', '.join('%.4f' % (v / CC.bar()) for v in d))
    assert max(d) <= CC.bar(), d
    # the merged (15,1) conv: its dy is d loss / d t as the GPU left it
    dka = np.concatenate([g[p0 + 'conv2d/kernel'], g[p1 + 'conv2d/kernel']], axis=3)
    dba = np.concatenate([g[p0 + 'conv2d/bias'], g[p1 + 'conv2d/bias']])
    ref, den = CC.reference64(run['out'], ka, g['t'], None, False)
    d = CC.distances((g['out'], dka, dba), ref, den)
    print('conv2d: distance / bar = %s' % ', '.join('%.4f' % (v / CC.bar()) for v in d))
    assert max(d) <= CC.bar(), d


def test_gradients(run, lh_weights):
    from xdet.model import LARGE_SEP_VARIABLES
    g = run['grads']
    assert len(LARGE_SEP_VARIABLES) == 10 and set(g) == set(LARGE_SEP_VARIABLES) | {'out', 'z', 't'}
    for k in LARGE_SEP_VARIABLES:
        assert g[k].shape == lh_weights[k].shape and g[k].dtype == f32 and np.isfinite(g[k]).all() and g[k].any(), k
    assert np.array_equal(bits(g['large_sep_feature/Branch_0/conv2d_1/bias']), bits(g['large_sep_feature/Branch_1/conv2d_1/bias']))
    shape, ld = run['d_out_shape_ld']
    assert shape == run['out'].shape == (2, 16, 16, 2048) and ld == run['out_ld']
    assert not run['d_out_raw'][..., 2048:].any() and run['d_out_raw'][..., :2048].any()
    for k in g:
        assert np.array_equal(bits(g[k]), bits(run['again'][k])), k
