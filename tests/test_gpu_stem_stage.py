"""The stem in training mode through the net (LightHeadDetector(stem_train=True), model.stem_train, model.stem_backward), on the
path of tests/test_gpu_entry_flow_backward.py and at its sizes: S = 256, two images, a detector built in split precision
(f16x3) with that file's TRAIN flags plus stem_train, one pass -- eval body, stem_train, entry_flow_train, middle_flow_train, the
chain behind the exit flow (flow_train_cases.downstream), exit_flow_backward, middle_flow_backward, entry_flow_backward,
stem_backward -- and every step judged against its float64 statement fed the tensors the GPU left upstream, so one check
measures one step.  At S = 256 the stem's maps are 127 -> 125, odd and odd: the parities of the 480-pixel net (239 -> 237).
Bars: z1 the derived bound of tests/test_gpu_stem_train_op.py (27 * 2^-24 * sum |x| |w| per element); the batch norms
batch_norm_cases.bar() through flow_train_cases.bn_forward_distances (eps 1e-4, momentum 0.99) and
batch_norm_cases.backward_distances; z2 3e-5 of the output's scale (tests/test_gpu_layers.py's f16x3 conv bar); dK2, da1 and
dK1 conv_strided_backward_cases.bar().
A second, small case runs the stage's own code (StemState, stem_train, stem_backward) on a stand-in for the detector at
tests/test_gpu_stem_chain.py's size and tensors (make_chain: two images of 21 x 21, which no net can be built for): the six
gradients of loss = sum(r * stem_out) against host_stem_* in float64, in that test's metric (chain_distances), at 4 x the
distance of the f32 host chain recorded in tests/golden/stem_train_f32_distance.npz -- the GPU result is never its own
yardstick.  And one image on the max_batch = 2 detector gives the bits of the same pass on a max_batch = 1 detector.
Every test prints the fraction of its bar it used (-s); the figures of an MI355X run are in DESIGN.md 4.46."""
import numpy as np
import pytest

import batch_norm_cases as BC
import conv_strided_backward_cases as CS

from flow_train_cases import S, P, NC, bits, close, bn_forward_distances, head_and_rpn_inputs, downstream
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_stem_train_op import conv64

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
CONV_FORWARD_TOL = 3e-5          # tests/test_gpu_layers.py::test_conv_matches_oracle, f16x3
EPS, MOMENTUM = 1e-4, 0.99
STEM_TRAIN = dict(TRAIN, stem_train=True)
H1, H2 = 127, 125


def host(g):
    return {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in g.items()}


def one_image_pass(det, image, d_stem):
    """eval body, stem_train and stem_backward on one image -> the bits of stem_out and of the six gradients"""
    from xdet import model as M
    from xdet.runtime import DeviceTensor
    with det.scope():
        M.XceptionBody(image, NC, is_training=False, data_format='channels_first')
        out = M.stem_train()
        r = {'stem_out': bits(out.numpy())}
        g = M.stem_backward(DeviceTensor.from_numpy(d_stem))
    r.update({k: bits(g[k]) for k in M.STEM_VARIABLES})
    return r


@pytest.fixture(scope='module')
def run(lh_weights):
    """one pass over the whole path; the tests below look at what it left"""
    from xdet import model as M, weights as W, InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor, get_precision, set_precision
    r = {}
    w = lh_weights
    images = r['images'] = W.synthetic_images(2, S, seed=3)
    inputs = head_and_rpn_inputs()
    before = get_precision()
    set_precision('f16x3')
    try:
        det = LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **STEM_TRAIN)
        det1 = LightHeadDetector(w, image_size=S, max_batch=1, rpn_post_nms_top_n=P, **STEM_TRAIN)
    finally:
        set_precision(before)
    r['det'] = det
    with det.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        buf = det.buffer('stem_out', 2)
        r['eval_stem_out'] = buf.numpy()
        M.entry_flow_train()                           # (on the eval-mode stem_out: the state stem_train has to drop)
        stem_t = M.stem_train()
        r['stem_is_the_buffer'] = stem_t.ptr == buf.ptr and stem_t.ld == buf.ld and stem_t.shape == buf.shape
        r['stem_out'], r['stem_shape_ld'] = buf.numpy(), (buf.shape, buf.ld)
        r['saved'] = {k: v.numpy() for k, v in det.stem_saved().items()}
        entry_x = det.buffer('entry_x', 2)
        with pytest.raises(InvalidArgumentError):      # what entry_flow_train saved belongs to the eval-mode stem_out
            M.entry_flow_backward(DeviceTensor.empty(entry_x.shape, ld=entry_x.ld))
        M.entry_flow_train()
        r['entry_x2'] = det.entry_flow_saved()['x2'].numpy()
        mid_t = M.middle_flow_train()
        lsep, rpn = downstream(M.exit_flow_train(), mid_t, inputs)
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'])
        mf = M.middle_flow_backward(ef['mid'])
        en = M.entry_flow_backward(mf['entry'])
        r['d_stem_t'], r['d_stem'] = en['stem'], en['stem'].numpy()
        r['saved_after'] = {k: v.numpy() for k, v in det.stem_saved().items()}     # no other stage's forward dropped it
        r['grads'] = host(M.stem_backward(en['stem'], intermediates=True))
        r['again'] = host(M.stem_backward(en['stem'], intermediates=True))
        r['lean'] = host(M.stem_backward(en['stem']))
        dev = M.stem_backward(en['stem'], weight_grads='device')
        r['device_types'] = {k: (type(v).__name__, tuple(v.shape), v.ld) for k, v in dev.items()}
        r['device'] = host(dev)
        r['stem_out_after'] = det.buffer('stem_out', 2).numpy()
    # one image, on both detectors
    d1 = np.random.default_rng(5).standard_normal((1, H2, H2, 64)).astype(f32)
    r['one_of_two'], r['one_of_one'] = one_image_pass(det, images[:1], d1), one_image_pass(det1, images[:1], d1)
    r['det1'] = det1
    return r


def judge_bn_forward(w, sv, conv, z, y):
    bn = conv + '_bn/'
    d = bn_forward_distances(z, w[bn + 'gamma'], w[bn + 'beta'], w[bn + 'moving_mean'], w[bn + 'moving_variance'],
                             (y, sv[bn + 'save_mean'], sv[bn + 'save_invstd'], sv[bn + 'moving_mean'], sv[bn + 'moving_variance']),
                             relu=True, eps=EPS, momentum=MOMENTUM)
    assert max(d.values()) <= BC.bar(), (conv, d)
    assert not np.array_equal(sv[bn + 'moving_mean'].reshape(-1), w[bn + 'moving_mean'])
    assert not np.array_equal(sv[bn + 'moving_variance'].reshape(-1), w[bn + 'moving_variance'])
    return max(d.values()) / BC.bar()


def test_training_forward(run, lh_weights):
    w, sv = lh_weights, run['saved']
    images = run['images']
    # x1: the image as NHWC rows; z1: the new kernel against float64 under the derived bound
    assert sv['x1'].shape == (2, S, S, 3) and np.array_equal(bits(sv['x1']), bits(np.transpose(images, (0, 2, 3, 1))))
    ref, mag = conv64(images, w['block1_conv1/kernel'])
    z1 = sv['block1_conv1/z']
    assert z1.shape == (2, H1, H1, 32)
    used = {'z1': float((np.abs(z1.astype(f64) - ref) / (27 * 2.0 ** -24 * mag)).max())}
    assert used['z1'] <= 1
    used['bn1'] = judge_bn_forward(w, sv, 'block1_conv1', z1, sv['a1'])
    z2 = sv['block1_conv2/z']
    assert sv['a1'].shape == (2, H1, H1, 32) and z2.shape == (2, H2, H2, 64)
    used['z2'] = close('block1_conv2', z2, CS.conv_forward64(sv['a1'], w['block1_conv2/kernel'], False, 1, 'VALID'), CONV_FORWARD_TOL)
    used['bn2'] = judge_bn_forward(w, sv, 'block1_conv2', z2, sv['x2'])
    print('training forward, fraction of each bar: %s' % ', '.join('%s %.4f' % kv for kv in used.items()))
    for a in (sv['a1'], sv['x2']):                     # both sides of both ReLUs are a real share of the tensor
        assert 0.05 <= float((a > 0).mean()) <= 0.95


def test_stem_out_holds_the_training_tensor(run):
    sv = run['saved']
    assert run['stem_is_the_buffer'] and run['stem_shape_ld'] == ((2, H2, H2, 64), 64)
    assert np.array_equal(bits(sv['x2']), bits(run['stem_out'])) and (run['stem_out'] >= 0).all() and run['stem_out'].any()
    assert np.array_equal(bits(run['entry_x2']), bits(run['stem_out']))          # the entry flow consumed it
    assert not np.array_equal(bits(run['stem_out']), bits(run['eval_stem_out']))   # batch, not moving, statistics
    assert np.array_equal(bits(run['stem_out_after']), bits(run['stem_out']))
    for k, v in sv.items():                            # nothing behind stem_train touched what it saved
        assert np.array_equal(bits(v), bits(run['saved_after'][k])), k


def test_the_chain(run, lh_weights):
    """every backward step against its statement fed the gradient the GPU left upstream"""
    w, sv, g = lh_weights, run['saved'], run['grads']
    assert run['d_stem'].any() and run['d_stem'].shape == (2, H2, H2, 64)
    used = {}

    def judge_bn(conv, z, y, dy, dz):
        bn = conv + '_bn'
        d = BC.backward_distances(dict(x=z, dy=dy, gamma=w[bn + '/gamma'], relu=True), True, y,
                                  sv[bn + '/save_mean'].reshape(-1), sv[bn + '/save_invstd'].reshape(-1),
                                  (dz, g[bn + '/gamma'], g[bn + '/beta']))
        assert max(d.values()) <= BC.bar(), (conv, d)
        return max(d.values()) / BC.bar()

    def judge_conv(x, kname, dz, dx, stride):
        ref, den = CS.reference64(x, w[kname], dz, None, False, stride, 'VALID')
        d = CS.distances((dx, g[kname], None), ref, den)
        assert max(d) <= CS.bar(), (kname, d)
        return max(d) / CS.bar()
    used['bn2 backward'] = judge_bn('block1_conv2', sv['block1_conv2/z'], sv['x2'], run['d_stem'], g['z/block1_conv2'])
    used['dK2, da1'] = judge_conv(sv['a1'], 'block1_conv2/kernel', g['z/block1_conv2'], g['a/block1_conv1'], 1)
    used['bn1 backward'] = judge_bn('block1_conv1', sv['block1_conv1/z'], sv['a1'], g['a/block1_conv1'], g['z/block1_conv1'])
    used['dK1'] = judge_conv(sv['x1'], 'block1_conv1/kernel', g['z/block1_conv1'], None, 2)
    print('the chain, fraction of each bar: %s' % ', '.join('%s %.4f' % kv for kv in used.items()))


def test_gradients(run, lh_weights):
    from xdet.model import STEM_VARIABLES
    g, lean, dev = run['grads'], run['lean'], run['device']
    names = set(STEM_VARIABLES)
    assert set(lean) == names == set(dev)              # six gradients, no image gradient
    assert set(g) == names | {'z/block1_conv2', 'a/block1_conv1', 'z/block1_conv1'}
    for k in names:
        assert isinstance(g[k], np.ndarray) and g[k].shape == lh_weights[k].shape and g[k].dtype == f32, k
        assert np.isfinite(g[k]).all() and g[k].any(), k
        assert run['device_types'][k] == ('DeviceTensor', lh_weights[k].shape, lh_weights[k].shape[-1]), run['device_types'][k]
    assert g['z/block1_conv2'].shape == (2, H2, H2, 64) and g['a/block1_conv1'].shape == g['z/block1_conv1'].shape == (2, H1, H1, 32)
    for k in g:
        assert np.array_equal(bits(g[k]), bits(run['again'][k])), k
    for k in names:
        assert np.array_equal(bits(g[k]), bits(lean[k])) and np.array_equal(bits(g[k]), bits(dev[k])), k


def test_one_image_does_not_depend_on_max_batch(run):
    a, b = run['one_of_two'], run['one_of_one']
    assert set(a) == set(b) and len(a) == 7
    for k in a:
        assert a[k].any() and np.array_equal(a[k], b[k]), k
    # and it is not the two-image pass's first image: the batch statistics are the batch's
    assert not np.array_equal(a['stem_out'][0], bits(run['stem_out'])[0])


class StandIn(object):
    """what StemState, stem_train and stem_backward read of a detector, at a size no net can be built for"""
    large_sep_train = exit_flow_train = middle_flow_train = entry_flow_train = False
    stem_train = True

    def __init__(self, S, B, weights, images):
        from xdet import train
        from xdet.runtime import DeviceTensor, Stream, to_device
        H2 = (S - 3) // 2 - 1
        self.image_size, self.max_batch, self._N = S, B, images.shape[0]
        self.stream = Stream()
        self._stem_out = DeviceTensor.empty((B, H2, H2, 64))
        self._images = to_device(np.ascontiguousarray(images, f32))
        self._stem = train.StemState(self, weights)

    def buffer(self, name, n=None):
        from xdet.runtime import DeviceTensor
        assert name == 'stem_out'
        t = self._stem_out
        return DeviceTensor(t.ptr, (n or self._N,) + t.shape[1:], t.ld, owner=self)


def test_the_six_gradients_against_the_float64_chain():
    """S = 21, tests/test_gpu_stem_chain.py's tensors and metric; the bar comes from the f32 host chain, recorded on the CPU"""
    import test_gpu_stem_chain as SC
    import test_stem_math as SM
    from xdet import model as M
    from xdet.runtime import DeviceTensor, _current
    p = SC.make_chain()
    w = SM.chain_weights(p)
    ref = SM.host_stem_chain(p, f64)
    _, den = SC.host_chain(p, f64)
    d = StandIn(21, 2, w, SM.chain_images(p))
    _current.append(d)
    try:
        out = M.stem_train()
        grads = M.stem_backward(DeviceTensor.from_numpy(p['r']))
    finally:
        _current.pop()
    assert tuple(out.shape) == (2, 8, 8, 64) and d._stem.n == 2
    a2 = out.numpy()
    assert (a2 == 0).any() and (a2 > 0).any()
    got = SM.as_chain(grads)
    bar = SM.chain_bar()
    dist = SC.chain_distances(got, ref, den)
    print('stem stage at S = 21: distance / bar = %s' % ', '.join('%s %.4f' % (n, dist[n] / bar) for n in SC.NAMES))
    for n in SC.NAMES:
        assert got[n].any() and dist[n] <= bar, (n, dist[n] / bar)


def test_refusals(run, lh_weights):
    from xdet import model as M, InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor
    det, det1 = run['det'], run['det1']
    plain = LightHeadDetector(lh_weights, image_size=S, max_batch=1, rpn_post_nms_top_n=P, **TRAIN)
    assert plain.stem_train is False and not hasattr(plain, '_stem')
    with plain.scope():
        M.XceptionBody(run['images'][:1], NC, is_training=False, data_format='channels_first')
        with pytest.raises(InvalidArgumentError, match='stem_train: needs a detector built with stem_train=True'):
            M.stem_train()
        with pytest.raises(InvalidArgumentError, match='stem_backward: needs a detector built with stem_train=True'):
            M.stem_backward(run['d_stem_t'])
        with pytest.raises(InvalidArgumentError, match='stem_saved'):
            plain.stem_saved()
    with det1.scope():
        det1.set_images(run['images'][:1])             # a new body: what the one-image pass saved is dropped
        with pytest.raises(InvalidArgumentError, match=r'stem_backward: call stem_train\(\) first'):
            M.stem_backward(DeviceTensor.empty((1, H2, H2, 64)))
        with pytest.raises(InvalidArgumentError, match='stem_saved'):
            det1.stem_saved()
    with det.scope():
        M.XceptionBody(run['images'], NC, is_training=False, data_format='channels_first')
        M.stem_train()
        with pytest.raises(InvalidArgumentError):
            M.stem_backward(DeviceTensor.empty((2, 8, 8, 64)))
        with pytest.raises(InvalidArgumentError):
            M.stem_backward(DeviceTensor.empty((2, H2, H2, 64), ld=96))          # another ld
        with pytest.raises(InvalidArgumentError):
            M.stem_backward(run['d_stem'])                                       # not on the device
        with pytest.raises(InvalidArgumentError, match='weight_grads'):
            M.stem_backward(run['d_stem_t'], weight_grads='both')
        with pytest.raises(InvalidArgumentError, match='stem_train: images must be a dense f32 DeviceTensor'):
            M.stem_train(images=run['images'])                                   # a host array
        # images=: the caller's own NCHW tensor gives the bits of the detector's buffer
        own = DeviceTensor(det._images.ptr, (2, 3, S, S), S, owner=det._images)
        again = M.stem_train(images=own).numpy()
        assert np.array_equal(bits(again), bits(run['stem_out']))
