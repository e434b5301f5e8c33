"""The refresh of a spectral conv from a kernel in device memory (xdet_spectral_conv_set_kernel_device, csrc/conv_repack.hip:
the two repack passes fed by spectral_weight_element of csrc/spectral_weights.h) and the net door that uses it
(xdet_net_refresh_heads on a spectral net built with the option spectral_refresh=on; MomentumOptimizer.refresh_eval_net), in
f16x3.  Every comparison is for equal bits: the device evaluates the block matrices by the host's own function from the host's
own table (tests/test_spectral_weights_host.py is the host side of that claim), and the passes behind the fetch are the
creation path's.

Layer: a layer created from w0 (a magnitude apart from w1's, so that a stale operand would show) and refreshed to
(w1, scale1, shift1) computes what a layer created from those computes; NULL scale / shift are kept; a second refresh restores
the first bits.  Net: one training iteration, one step and refresh_eval_net() on the detector of tests/test_gpu_optimizer_heads.py
with large_sep='spectral', against a spectral detector built afresh from the exported weights; a calibrated net (the two (15,1)
kernels x 2^K, as tests/test_gpu_proposals.py's overflow test scales them) keeps its exponents and bits through a refresh, and a
cold net refreshed with those weights calibrates like a net built from them.  Without the option the refusal stands."""
import numpy as np
import pytest

from flow_train_cases import S, P, bits, head_and_rpn_inputs
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_net_refresh import detections, equal, graph_count
from test_gpu_optimizer_heads import iteration, weight_gradients, LR, MOMENTUM, WEIGHT_DECAY

pytestmark = pytest.mark.gpu
f32 = np.float32

# (T, cin, cout, axis, F): G.cout = 2 round_up(cout, 32) = 64 -> the 64-wide GEMM tile; 128 -> the 128-wide one (and padding
# channels on both sides); 3 taps; 19 and 29 bins
SHAPES = {'15x32x32_y_F16': (15, 32, 32, 0, 16), '15x24x40_x_F16': (15, 24, 40, 1, 16), '3x32x32_x_F16': (3, 32, 32, 1, 16),
          '15x32x32_y_F30': (15, 32, 32, 0, 30), '15x32x32_x_F50': (15, 32, 32, 1, 50)}
# every shape at N = 1 and N = 3; rows per bin are N F in groups of 128 up to 128 rows and of 256 above: N = 3 reaches the
# 256-row groups at F = 50, the two N = 9 cases reach them with both tile widths at F = 16.  The variants are dealt over them.
CASES = [('15x32x32_y_F16', 1, 'plain'), ('15x32x32_y_F16', 3, 'relu'), ('15x24x40_x_F16', 1, 'zero_channel'),
         ('15x24x40_x_F16', 3, 'keep_affine'), ('3x32x32_x_F16', 1, 'zero_kernel'), ('3x32x32_x_F16', 3, 'plain'),
         ('15x32x32_y_F30', 1, 'plain'), ('15x32x32_y_F30', 3, 'plain'), ('15x32x32_x_F50', 1, 'plain'),
         ('15x32x32_x_F50', 3, 'plain'), ('15x32x32_y_F16', 9, 'plain'), ('15x24x40_x_F16', 9, 'plain')]


def dense(a):
    from xdet.runtime import DeviceTensor, to_device
    b = to_device(a)
    return DeviceTensor(b.ptr, a.shape, a.shape[-1], owner=b)


def make_layer(w, axis, F, scale, shift, relu=False):
    from xdet import ops
    from xdet.runtime import get_precision, set_precision
    before = get_precision()
    set_precision('f16x3')
    try:
        return ops.SpectralConv(w, axis, F, scale, shift, relu=relu)
    finally:
        set_precision(before)


def forward_bits(layer, x):
    from xdet.runtime import DeviceTensor
    return bits(layer(DeviceTensor.from_numpy(x)).numpy())


def values(name, N, variant):
    T, cin, cout, axis, F = SHAPES[name]
    rng = np.random.default_rng(sum(name.encode()) * 31 + N)
    w0 = (rng.standard_normal((T, cin, cout)) * 8).astype(f32)
    w1 = (rng.standard_normal((T, cin, cout)) / np.sqrt(T * cin)).astype(f32)
    if variant == 'zero_channel':
        w1[:, :, cout // 2] = 0
    if variant == 'zero_kernel':
        w1[:] = 0
    affine = lambda: (rng.uniform(0.5, 1.5, cout).astype(f32), rng.standard_normal(cout).astype(f32))
    x = rng.standard_normal((N, F, F, cin)).astype(f32)
    return w0, affine(), w1, affine(), x


@pytest.mark.parametrize('name,N,variant', CASES, ids=['%s_n%d_%s' % c for c in CASES])
def test_a_refreshed_layer_equals_a_created_one(name, N, variant):
    from xdet.runtime import synchronize, to_device
    T, cin, cout, axis, F = SHAPES[name]
    w0, (sc0, sh0), w1, (sc1, sh1), x = values(name, N, variant)
    relu = variant == 'relu'
    layer = make_layer(w0, axis, F, sc0, sh0, relu)
    first = forward_bits(layer, x)
    if variant == 'keep_affine':                         # NULL scale and shift: what the layer has stays
        layer.set_kernel_device(dense(w1))
        fresh = make_layer(w1, axis, F, sc0, sh0, relu)
    else:
        layer.set_kernel_device(dense(w1), scale=to_device(sc1), shift=to_device(sh1))
        fresh = make_layer(w1, axis, F, sc1, sh1, relu)
    synchronize()
    got, want = forward_bits(layer, x), forward_bits(fresh, x)
    assert got.shape == want.shape == (N, F, F, cout)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got, first)
    # back to w0 (and the first scale and shift): nothing of w1 is left in any buffer
    layer.set_kernel_device(dense(w0), scale=to_device(sc0), shift=to_device(sh0))
    synchronize()
    assert np.array_equal(forward_bits(layer, x), first)


def test_refusals_leave_the_layer_as_it_was_and_the_old_doors_still_refuse():
    import xdet
    from xdet import ops
    from xdet._lib import lib
    from xdet.ops import refresh_layers_device
    from xdet.runtime import DeviceBuffer, synchronize, to_device
    T, cin, cout, axis, F = SHAPES['3x32x32_x_F16']
    w0, (sc0, sh0), w1, (sc1, sh1), x = values('3x32x32_x_F16', 1, 'plain')
    layer = make_layer(w0, axis, F, sc0, sh0)
    was = forward_bits(layer, x)
    k1 = dense(w1)
    # a NULL layer, a NULL kernel, a handle that is not a spectral layer: the library, by name
    assert lib().xdet_spectral_conv_set_kernel_device(None, k1.ptr, None, None, None) == -1
    assert b'not a spectral conv layer' in lib().xdet_last_error()
    assert lib().xdet_spectral_conv_set_kernel_device(layer.handle, None, None, None, None) == -1
    assert b'kernel is NULL' in lib().xdet_last_error()
    conv = ops.Conv2D(np.zeros((1, 1, 32, 32), f32))
    assert lib().xdet_spectral_conv_set_kernel_device(conv.handle, k1.ptr, None, None, None) == -1
    assert b'not a spectral conv layer' in lib().xdet_last_error()
    # a host array, a wrong shape, a host scale: the Python door, by name
    with pytest.raises(xdet.InvalidArgumentError, match=r'SpectralConv.set_kernel_device: kernel must be a dense DeviceTensor.*device memory.*ndarray'):
        layer.set_kernel_device(w1)
    with pytest.raises(xdet.InvalidArgumentError, match='SpectralConv.set_kernel_device: kernel must be a dense DeviceTensor of shape'):
        layer.set_kernel_device(dense(w1.transpose(0, 2, 1)[:, :, :16].copy()))
    with pytest.raises(xdet.InvalidArgumentError, match='scale must be a device array of 32 floats'):
        layer.set_kernel_device(k1, scale=sc1)
    synchronize()
    assert np.array_equal(forward_bits(layer, x), was)
    # refreshed through the new door, the layer is still a spectral handle to the two old ones
    layer.set_kernel_device(k1, scale=to_device(sc1), shift=to_device(sh1))
    synchronize()
    now = forward_bits(layer, x)
    assert not np.array_equal(now, was)
    assert lib().xdet_conv_set_kernel_device(layer.handle, k1.ptr, None, None) == -1
    assert b'a spectral layer keeps its kernel as DFT-domain block matrices' in lib().xdet_last_error()
    with pytest.raises(xdet.InvalidArgumentError, match='a spectral layer keeps its kernel as DFT-domain block matrices'):
        refresh_layers_device([(layer, to_device(w1.ravel()))], workspace=DeviceBuffer(1 << 20))
    synchronize()
    assert np.array_equal(forward_bits(layer, x), now)


# ---- the net door ------------------------------------------------------------------------------------------------------------

def eager(det, images):
    """detections()'s buffers from a forward without a graph"""
    from xdet.runtime import to_host
    n, nc, k = det.set_images(images), det.num_classes - 1, det.nms_topk
    det.forward_device(n, use_graph=False)
    det.stream.synchronize()
    r = {name: bits(det.buffer(name, n).numpy()) for name in ('feat', 'rpn_out', 'cls_reg')}
    r['scores'] = bits(to_host(det._det_scores.ptr, (n, nc, k)))
    r['boxes'] = bits(to_host(det._det_boxes.ptr, (n, nc, k, 4)))
    return r


def block_matrix_bytes(F=S // 16, cin=2048, mid2=512):
    """the smaller of the net's two sets of block matrices would be this large as one f32 array -- the first conv's"""
    return ((F + 8) // 2 * 2 // 2) * (2 * cin) * (2 * mid2) * 4


@pytest.fixture(scope='module')
def trained(lh_weights):
    """one iteration, one step at reach='all' and refresh_eval_net() on a spectral detector built with spectral_refresh=True"""
    from xdet import train, weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    images, inputs = W.synthetic_images(2, S, seed=3), head_and_rpn_inputs()
    build = lambda w, **kw: LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **dict(TRAIN, large_sep='spectral', **kw))
    r = {}
    before = get_precision()
    set_precision('f16x3')
    try:
        det = build(lh_weights, spectral_refresh=True)
        opt = train.MomentumOptimizer(det, MOMENTUM, WEIGHT_DECAY, reach='all')
        r['before'] = detections(det, images)                      # (captures the graph)
        it = iteration(det, inputs, 'device', images)
        opt.step(weight_gradients(it['sections'], opt.variables), LR)
        r['stale'] = detections(det, images)
        r['graphs_before'], r['memory_before'] = graph_count(det), det.memory()['allocated_bytes']
        r['layers'] = opt.refresh_eval_net()
        r['graphs_after'], r['memory_after'] = graph_count(det), det.memory()['allocated_bytes']
        r['after'] = detections(det, images)                       # (replays it)
        r['graphs_replayed'] = graph_count(det)
        r['eager'] = eager(det, images)
        r['ref'] = detections(build(opt.export_weights(lh_weights)), images)
    finally:
        set_precision(before)
    return r


def test_net_refresh_eval_net_goes_through_and_equals_a_fresh_spectral_detector(trained):
    r = trained
    assert r['layers'] == 74
    assert equal(r['after'], r['ref']) == {}
    # (the step refreshes the two heads' layers, which the eval net shares: `feat` is what only this refresh can move)
    assert not np.array_equal(r['after']['feat'], r['stale']['feat'])
    assert not np.array_equal(r['after']['scores'], r['before']['scores'])


def test_net_graphs_stay_and_replay_the_new_weights(trained):
    r = trained
    assert r['graphs_before'] == r['graphs_after'] == r['graphs_replayed'] == 1
    assert equal(r['after'], r['eager']) == {}


def test_net_scratch_shows_in_memory_and_is_no_block_matrix(trained):
    """the first call allocates the merges' scratch (the two merged kernels, 15 x 2048 x 512 and 15 x 512 x 490 floats, and the
    small block) and nothing of the size of a layer's block matrices"""
    grown = trained['memory_after'] - trained['memory_before']
    merged = (15 * 2048 * 512 + 15 * 512 * 490) * 4
    print('refresh scratch: %d bytes; merged kernels %d; the first conv\'s block matrices %d' % (grown, merged, block_matrix_bytes()))
    assert merged <= grown < merged + (8 << 20)
    assert grown < block_matrix_bytes()


LSEP_A = ['large_sep_feature/%s/conv2d/kernel' % br for br in ('Branch_0', 'Branch_1')]


def on_device(w):
    from xdet import train
    from xdet.runtime import to_device
    return {n: to_device(np.ascontiguousarray(w[n], f32)) for n in train.LARGE_SEP_VARIABLES + train.LARGE_SEP_MOVING}


@pytest.fixture(scope='module')
def calibrated(lh_weights):
    """K: the first of 10, 11, ... at which calibrate() gives a DFT-domain plane an exponent (the fixture records it: 10 on an
    MI355X, where conv2d_1/dft_x gets exponent 4 and the head's first dense input 1); `hot` is built from Wh and calibrated,
    `cold` from the checkpoint"""
    import xdet
    from xdet import weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    images = W.synthetic_images(2, S, seed=3)
    build = lambda w, **kw: LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=P, large_sep='spectral', check_range=True,
                                              **kw)
    dft = lambda scaled: {n: e for n, e in scaled.items() if 'DFT-domain planes' in n}
    r = {}
    before = get_precision()
    set_precision('f16x3')
    try:
        k = 10
        while True:
            wh = dict(lh_weights)
            for n in LSEP_A:
                wh[n] = np.ldexp(np.asarray(lh_weights[n], f32), k).astype(f32)
            hot = build(wh, spectral_refresh=True)
            scaled = hot.calibrate(images)
            if dft(scaled) or k >= 24:
                break
            k += 1
        r['k'], r['scaled'], r['dft'] = k, scaled, dft(scaled)
        try:
            hot.forward(images)
            r['clean'] = None
        except xdet.XdetError as e:
            r['clean'] = str(e)
        d_hot, d_cold = on_device(wh), on_device(lh_weights)
        # (i) the calibrated net refreshed with its own weights; by way of the checkpoint's and back
        r['scales0'], r['bits0'] = hot.plane_scales(), detections(hot, images)
        hot.refresh_heads(d_hot)
        r['scales1'], r['bits1'] = hot.plane_scales(), detections(hot, images)
        hot.refresh_heads(d_cold)
        r['scales2'], r['bits_cold'] = hot.plane_scales(), detections(hot, images)
        hot.refresh_heads(d_hot)
        r['scales3'], r['bits3'] = hot.plane_scales(), detections(hot, images)
        # (ii) calibrate after refresh
        cold = build(lh_weights, spectral_refresh=True)
        r['cold_before'] = detections(cold, images)
        cold.refresh_heads(d_hot)
        r['cold_scaled'] = cold.calibrate(images)
        r['cold_scales'], r['cold'] = cold.plane_scales(), detections(cold, images)
        # the option off: the refusal, and the net as it was
        off = build(lh_weights)
        r['off_before'] = detections(off, images)
        try:
            off.refresh_heads(d_hot)
            r['off_error'] = None
        except xdet.InvalidArgumentError as e:
            r['off_error'] = str(e)
        r['off_after'] = detections(off, images)
    finally:
        set_precision(before)
    print('K = %d: %r' % (r['k'], r['scaled']))
    return r


def test_calibrated_fixture_reaches_the_dft_planes_and_runs_clean(calibrated):
    r = calibrated
    assert r['dft'] and any(e != 0 for e in r['dft'].values()), (r['k'], r['scaled'])
    assert r['clean'] is None, r['clean']
    assert np.isfinite(r['bits0']['feat'].view(f32)).all()


def test_calibrated_net_keeps_exponents_and_bits_through_a_refresh(calibrated):
    r = calibrated
    assert equal(r['bits1'], r['bits0']) == {}
    assert equal(r['bits3'], r['bits0']) == {}
    assert not np.array_equal(r['bits_cold']['feat'], r['bits0']['feat'])
    assert r['scales0'] == r['scales1'] == r['scales2'] == r['scales3']


def test_calibrate_after_refresh_equals_a_net_built_from_the_weights(calibrated):
    r = calibrated
    assert r['cold_scaled'] == r['scaled'] and r['cold_scales'] == r['scales0']
    assert equal(r['cold'], r['bits0']) == {}
    assert not np.array_equal(r['cold']['feat'], r['cold_before']['feat'])


def test_option_off_still_refuses_with_the_old_words(calibrated):
    r = calibrated
    assert r['off_error'] and 'large_sep_feature' in r['off_error'] and 'large_sep=direct' in r['off_error'], r['off_error']
    assert 'which keeps the kernels as DFT-domain block matrices' in r['off_error']
    assert equal(r['off_after'], r['off_before']) == {}
