"""The host statements of the eval-net refresh, without a GPU: xdet.ops.host_bn_fold (the NumPy statement of xdet_bn_fold) against
the float64 formula and at the documented bit patterns, and the pure-Python grouping MomentumOptimizer.refresh_eval_net and
LightHeadDetector.refresh_weights check their table with (train.eval_net_groups).
The float32 fold's bar: sc = g / sqrt(v + eps) passes three roundings (the sum, the root, the quotient: 3 x 2^-24 relative, the
root halving the sum's), shift = (b - m sc) + bias sc five more on terms bounded by |b| + |m sc| + |bias sc|."""
import numpy as np
import pytest

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def arrays(C, seed, with_bias):
    rng = np.random.default_rng(seed)
    g, b, m = (rng.standard_normal(C).astype(f32) for _ in range(3))
    v = rng.uniform(1e-6, 4.0, C).astype(f32)
    return g, b, m, v, (rng.standard_normal(C).astype(f32) if with_bias else None)


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('eps', [1e-4, 1e-5])
def test_host_bn_fold_against_float64(with_bias, eps):
    from xdet.ops import host_bn_fold
    g, b, m, v, bias = arrays(2048, 5, with_bias)
    sc, sh = host_bn_fold(g, b, m, v, eps, bias)
    assert sc.dtype == f32 and sh.dtype == f32
    g64, b64, m64, v64 = (np.asarray(a, f64) for a in (g, b, m, v))
    rsc = g64 / np.sqrt(v64 + f64(f32(eps)))
    rsh = b64 - m64 * rsc + (np.asarray(bias, f64) * rsc if with_bias else 0.0)
    assert (np.abs(sc - rsc) <= 3 * U * np.abs(rsc)).all()
    scale = np.abs(b64) + np.abs(m64 * rsc) + (np.abs(np.asarray(bias, f64) * rsc) if with_bias else 0.0)
    assert (np.abs(sh - rsh) <= 8 * U * scale).all()
    # the float64 door is the formula itself
    sc64, sh64 = host_bn_fold(g, b, m, v, f64(f32(eps)), bias, dtype=f64)
    assert np.array_equal(sc64, rsc) and np.array_equal(sh64, rsh)


def test_host_bn_fold_documented_bits():
    from xdet.ops import host_bn_fold
    one = np.ones(1, f32)
    # beta = -0, mean = 0: (-0 - 0 * sc) = -0, and the + 0.f of a fold without bias makes it +0
    sc, sh = host_bn_fold(one, f32([-0.0]), f32([0.0]), one, 0.0)
    assert bits(sc)[0] == 0x3f800000 and bits(sh)[0] == 0x00000000
    # with a bias the sum is -0 + (-0 * 1) = -0: kept
    _, sh = host_bn_fold(one, f32([-0.0]), f32([0.0]), one, 0.0, bias=f32([-0.0]))
    assert bits(sh)[0] == 0x80000000
    # gamma = -0: the scale is -0, mean * -0 = -0 for a positive mean, beta - (-0) = beta
    sc, sh = host_bn_fold(f32([-0.0]), f32([0.5]), f32([2.0]), one, 0.0)
    assert bits(sc)[0] == 0x80000000 and bits(sh)[0] == bits(f32([0.5]))[0]
    # denormals pass: the smallest one as gamma over sqrt(1) stays itself, and as beta it is the shift
    tiny = np.array([1], np.uint32).view(f32)
    sc, sh = host_bn_fold(tiny, tiny, f32([0.0]), one, 0.0)
    assert bits(sc)[0] == 1 and bits(sh)[0] == 1
    # a denormal variance plus eps is eps: 1 / sqrt(2^-20) = 2^10
    sc, _ = host_bn_fold(one, one, one, tiny, 2.0 ** -20)
    assert bits(sc)[0] == bits(f32([1024.0]))[0]


def reach():
    from xdet import train as T
    return (T.ENTRY_FLOW_VARIABLES + T.MIDDLE_FLOW_VARIABLES + T.EXIT_FLOW_VARIABLES +
            T.ENTRY_FLOW_MOVING + T.MIDDLE_FLOW_MOVING + T.EXIT_FLOW_MOVING)


def test_grouping_names_every_name_once():
    from xdet import train as T
    names = reach()
    assert len(names) == 148 + 76 == len(set(names))
    groups = T.eval_net_groups(names)
    assert len(groups) == 38                       # 34 units and 4 projections: 34 x 2 + 4 = 72 layers
    assert sum(2 if not g.startswith('conv2d_') else 1 for g in groups) == 72
    flat = [n for have in groups.values() for n in have]
    assert sorted(flat) == sorted(names)
    assert all(len(v) == (5 if g.startswith('conv2d_') else 6) for g, v in groups.items())
    # any set of whole groups: the exit flow alone
    exit_only = T.eval_net_groups(T.EXIT_FLOW_VARIABLES + T.EXIT_FLOW_MOVING)
    assert sorted(exit_only) == ['block13_sepconv1', 'block13_sepconv2', 'block14_sepconv1', 'block14_sepconv2', 'conv2d_4']


def test_grouping_refusals_are_by_name():
    import xdet
    from xdet import train as T
    names = list(reach())
    for gone in ('block7_sepconv2_bn/moving_variance', 'conv2d_2/kernel', 'block13_sepconv1/depthwise_kernel'):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            T.eval_net_groups([n for n in names if n != gone])
        assert gone in str(e.value) and 'in part' in str(e.value)
    for outside in ('rpn_head/conv2d/kernel', 'block1_conv2/kernel', 'large_sep_feature/batch_normalization/gamma',
                    'final_head/fc_cls/kernel', 'nonsense'):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            T.eval_net_groups(names + [outside])
        assert outside in str(e.value) and 'outside the reach' in str(e.value)
    with pytest.raises(xdet.InvalidArgumentError) as e:
        T.eval_net_groups(names + ['conv2d_4/kernel'])
    assert 'conv2d_4' in str(e.value)
