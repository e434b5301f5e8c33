"""The NumPy statements of the clipped momentum step (xdet.ops): host_clip_scale, host_momentum_step(..., scale=) and
host_grad_sq, the record's f32 sum of squares in the device's order.  No GPU."""
import math

import numpy as np
import pytest

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_scale_is_exactly_one_at_or_below_the_clip():
    from xdet import host_clip_scale
    rng = np.random.default_rng(3)
    assert bits(host_clip_scale(f32(25), 5))[0] == 0x3f800000            # norm == clip: the gradient [3, 4] under a clip of 5
    for clip in (f32(5), f32(0.1), f32(1e-3), f32(3e4), f32(1.7)):
        sq = rng.uniform(0, float(clip) ** 2, 2000).astype(f32)
        sq = sq[np.sqrt(sq) <= clip]                       # (the statement's own norm, an f32)
        assert sq.size > 1000
        ends = [f32(0), np.nextafter(f32(clip * clip), f32(0)), f32(clip * clip)]
        hit = [s for s in ends if np.sqrt(s) == clip]      # a grad_sq whose f32 root IS the clip
        assert hit
        for s in list(sq[:300]) + [s for s in ends if np.sqrt(s) <= clip]:
            got = host_clip_scale(s, clip)
            assert got.dtype == f32 and bits(got)[0] == 0x3f800000, (s, clip, got)


def test_scale_is_the_float64_value_rounded_twice():
    """norm = the f32 nearest sqrt(grad_sq), scale = the f32 nearest clip / max(norm, clip): float64 holds the exact square
    root of an f32 to 53 bits and the exact quotient of two f32 to 53 bits, and a double rounding through 53 bits to 24 is the
    single rounding for both operations (2p + 2 <= 53), so the float64 route is the yardstick bit for bit"""
    from xdet import host_clip_scale
    rng = np.random.default_rng(4)
    sq = np.concatenate([rng.uniform(0, 100, 3000), 10.0 ** rng.uniform(-30, 30, 3000)]).astype(f32)
    for clip in (0.5, 5.0, 1e-4, 123.456):
        c = f32(clip)
        for s in sq[::7]:
            norm = f32(math.sqrt(f64(s)))
            want = f32(f64(c) / f64(max(norm, c)))
            got = host_clip_scale(s, clip)
            assert bits(got)[0] == bits(want)[0], (s, clip, got, want)
            assert 0 <= got <= 1


def test_scale_of_a_record_that_is_not_finite():
    from xdet import host_clip_scale
    assert np.isnan(host_clip_scale(f32(np.nan), 1.0))     # the maximum keeps a NaN norm
    assert host_clip_scale(f32(np.inf), 1.0) == 0


@pytest.mark.parametrize('clip', [0, -1.0, np.nan, np.inf])
def test_scale_refuses_a_clip_that_is_not_finite_and_positive(clip):
    import xdet
    with pytest.raises(xdet.InvalidArgumentError) as e:
        xdet.host_clip_scale(f32(1), clip)
    assert 'clip_scale: clip_norm must be finite and positive' in str(e.value)


@pytest.mark.parametrize('decay', [True, False])
@pytest.mark.parametrize('dtype', [f32, f64])
def test_scale_one_keeps_the_bits_of_the_plain_statement(decay, dtype):
    from xdet import host_momentum_step
    rng = np.random.default_rng(5)
    var, grad, accum = (rng.standard_normal(5000).astype(f32) * s for s in (0.1, 0.01, 0.02))
    grad[7], grad[8], var[9] = -0.0, 1e-42, 0.0            # a signed zero and a denormal keep their bits through x * 1
    plain = host_momentum_step(var, grad, accum, 0.1, 0.9, 2e-4, decay, dtype)
    for one in (f32(1), 1, 1.0):
        got = host_momentum_step(var, grad, accum, 0.1, 0.9, 2e-4, decay, dtype, scale=one)
        for a, b in zip(got, plain):
            assert a.dtype == b.dtype == dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_scale_is_one_more_rounding():
    from xdet import host_momentum_step
    rng = np.random.default_rng(6)
    var, grad, accum = (rng.standard_normal(3000).astype(f32) * s for s in (0.1, 0.01, 0.02))
    s = f32(0.3712)
    v, a = host_momentum_step(var, grad, accum, 0.1, 0.9, 2e-4, True, scale=s)
    g = (grad * s).astype(f32)
    wv, wa = host_momentum_step(var, g, accum, 0.1, 0.9, 2e-4, True)
    assert np.array_equal(bits(v), bits(wv)) and np.array_equal(bits(a), bits(wa))
    assert not np.array_equal(bits(v), bits(host_momentum_step(var, grad, accum, 0.1, 0.9, 2e-4, True)[0]))


def test_grad_sq_follows_the_float64_sum():
    """the ordered f32 sum against host_grad_stats: every term is non-negative and passes 1 + 2 + 2 + 8 + ceil(log2(chunks))
    roundings (include/xdet.h)"""
    from xdet import host_grad_sq, host_grad_stats
    rng = np.random.default_rng(7)
    sizes = [1, 5, 4095, 4096, 4097, 9000]
    grads = [(rng.standard_normal(n) * 0.01).astype(f32) for n in sizes]
    chunks = sum(-(-n // 4096) for n in sizes)
    k = 1 + 2 + 2 + 8 + math.ceil(math.log2(chunks))
    got, want = host_grad_sq(grads), host_grad_stats(grads)[0]
    assert got.dtype == f32 and abs(float(got) - want) / want <= k * U / (1 - k * U)
    assert host_grad_sq([np.array([3, 4], f32)]) == 25
    bad = [g.copy() for g in grads]
    bad[3][17] = np.nan
    assert np.isnan(host_grad_sq(bad))


class Fake(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_train_step_refuses_a_bad_clip_norm_or_communicator():
    """ahead of any device work: the constructor needs no GPU for its refusals"""
    import xdet
    from xdet import model
    det = Fake(head_rois=64, pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True, middle_flow_train=True,
               entry_flow_train=True, cfg=Fake(rpn_nms_thres=0.7, rpn_min_size=16. / 480))
    opt = Fake(det=det, reach='all', variables=())
    args = dict(rpn_anchors_per_image=256, rpn_fg_ratio=0.25, roi_one_image=64, fg_ratio=0.25, ohem_roi_one_image=32, nms_threshold=0.7,
                rpn_min_size=16. / 480)
    for bad in (0, -1.0, float('nan'), float('inf'), 'ten', True):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            model.TrainStep(det, opt, Fake(_anchors=[None]), clip_norm=bad, **args)
        assert 'TrainStep: clip_norm must be None or a finite positive number' in str(e.value)
    with pytest.raises(xdet.InvalidArgumentError) as e:
        model.TrainStep(det, opt, Fake(_anchors=[None]), comm=object(), **args)
    assert 'TrainStep: comm must be an xdet.dist.Communicator, got object' in str(e.value)
    ts = model.TrainStep(det, opt, Fake(_anchors=[None]), clip_norm=10, comm=Fake(average_gradients=None, world=2), **args)
    assert ts.clip_norm == 10 and ts.comm.world == 2
    plain = model.TrainStep(det, opt, Fake(_anchors=[None]), **args)
    assert plain.clip_norm is None and plain.comm is None
