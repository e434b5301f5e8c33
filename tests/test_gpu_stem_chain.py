"""xdet_conv_backward_strided closes the stem: the two stem convs of the Xception entry flow with their training-mode batch
norms, forward and backward on the GPU on one stream with no host round trip, against the same chain in float64 NumPy.

    image [2,21,21,3] -> Conv2D(k1, stride 2, 'VALID') (f16x3, f32 out) -> batch norm (training, ReLU) -> [2,10,10,32]
                      -> Conv2D(k2, 'VALID') -> batch norm (training, ReLU) -> stem_out [2,8,8,64];   loss = sum(r * stem_out)
    backward: batch_norm_backward -> conv_backward_strided_device(stride 1, 'VALID') -> batch_norm_backward ->
              conv_backward_strided_device(stride 2, 'VALID', with_dx=False)

The gradients of both kernels, gammas and betas are judged by tests/conv_strided_backward_cases.py's metric -- max |got - ref|
over the largest entry of the same sum taken over the float64 chain's operand magnitudes -- at 4 x the distance of the f32 HOST
chain from the float64 one, recorded in tests/golden/conv_strided_backward_f32_distance.npz under stem_chain_f32_distance
(`python tests/test_conv_strided_backward_math.py --write`, on the CPU): the GPU result is never its own yardstick.
Measured on an MI355X: 0.05 (beta2) to 0.22 (gamma1) of that bar, 4 x 1.39e-07."""
import numpy as np
import pytest

import conv_strided_backward_cases as CS

f32, f64 = np.float32, np.float64
EPS = 1e-4
NAMES = ('k1', 'gamma1', 'beta1', 'k2', 'gamma2', 'beta2')


def make_chain():
    rng = np.random.default_rng(2117)
    p = {'image': rng.standard_normal((2, 21, 21, 3)).astype(f32),
         'k1': (rng.standard_normal((3, 3, 3, 32)) / np.sqrt(27)).astype(f32),
         'k2': (rng.standard_normal((3, 3, 32, 64)) / np.sqrt(288)).astype(f32),
         'gamma1': rng.uniform(0.5, 1.5, 32).astype(f32), 'beta1': (rng.standard_normal(32) * 0.3).astype(f32),
         'gamma2': rng.uniform(0.5, 1.5, 64).astype(f32), 'beta2': (rng.standard_normal(64) * 0.3).astype(f32),
         'r': rng.standard_normal((2, 8, 8, 64)).astype(f32)}
    for a in p.values():
        a.setflags(write=False)
    return p


def valid_forward(x, w, stride, dtype):
    """conv(x, w), 'VALID', one product per tap in `dtype`"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    kh, kw = w.shape[:2]
    Ho, Wo = (x.shape[1] - kh) // stride + 1, (x.shape[2] - kw) // stride + 1
    out = np.zeros((x.shape[0], Ho, Wo, w.shape[3]), dtype)
    for a in range(kh):
        for b in range(kw):
            out += np.matmul(x[:, a:a + (Ho - 1) * stride + 1:stride, b:b + (Wo - 1) * stride + 1:stride], w[a, b])
    return out


def host_chain(p, dtype):
    """-> (the six gradients under NAMES, the six denominators of the metric) of the chain in `dtype`"""
    from xdet.ops import host_conv_backward_strided as conv_bwd, host_batch_norm_forward as bn_fwd, host_batch_norm_backward as bn_bwd
    z1 = valid_forward(p['image'], p['k1'], 2, dtype)
    a1, mean1, inv1 = bn_fwd(z1, p['gamma1'], p['beta1'], EPS, relu=True, dtype=dtype)[:3]
    z2 = valid_forward(a1, p['k2'], 1, dtype)
    a2, mean2, inv2 = bn_fwd(z2, p['gamma2'], p['beta2'], EPS, relu=True, dtype=dtype)[:3]
    r = np.asarray(p['r'], dtype)
    dz2, dg2, db2 = bn_bwd(z2, a2, r, p['gamma2'], mean2, inv2, dtype=dtype)
    da1, dk2, _ = conv_bwd(a1, p['k2'], dz2, dtype=dtype, stride=1, padding='VALID')
    dz1, dg1, db1 = bn_bwd(z1, a1, da1, p['gamma1'], mean1, inv1, dtype=dtype)
    _, dk1, _ = conv_bwd(p['image'], p['k1'], dz1, dtype=dtype, with_dx=False, stride=2, padding='VALID')
    grads = dict(zip(NAMES, (dk1, dg1, db1, dk2, dg2, db2)))

    def bn_den(z, a, dy, mean, inv):
        g = np.where(a > 0, np.abs(dy), 0).reshape(-1, z.shape[-1])
        xhat = np.abs((z - mean) * inv).reshape(-1, z.shape[-1])
        return float((g * xhat).sum(0).max()), float(g.sum(0).max())
    dk_den = lambda x, k, dy, s: float(conv_bwd(np.abs(x), np.abs(np.asarray(k, dtype)), np.abs(dy), dtype=dtype, with_dx=False,
                                                stride=s, padding='VALID')[1].max())
    den = dict(zip(NAMES, (dk_den(p['image'], p['k1'], dz1, 2),) + bn_den(z1, a1, da1, mean1, inv1)
                   + (dk_den(a1, p['k2'], dz2, 1),) + bn_den(z2, a2, r, mean2, inv2)))
    return grads, den


def chain_distances(got, ref, den):
    return {n: float(np.abs(np.asarray(got[n], f64) - ref[n]).max()) / den[n] for n in NAMES}


def f32_chain_distance():
    """the largest distance of the f32 host chain from the float64 one"""
    p = make_chain()
    ref, den = host_chain(p, f64)
    return max(chain_distances(host_chain(p, f32)[0], ref, den).values())


@pytest.mark.gpu
def test_the_op_closes_the_stem():
    from xdet import ops
    from xdet.runtime import DeviceTensor, Stream, get_precision, set_precision, to_host
    p = make_chain()
    ref, den = host_chain(p, f64)
    before = get_precision()
    set_precision('f16x3')
    try:
        conv1, conv2 = ops.Conv2D(p['k1'], stride=2, padding='VALID'), ops.Conv2D(p['k2'], padding='VALID')
    finally:
        set_precision(before)
    st = Stream()
    image = DeviceTensor.from_numpy(p['image'])
    d_r = DeviceTensor.from_numpy(p['r'])
    # forward and backward: device doors on one stream, nothing synchronised or read until the end
    z1 = conv1(image, stream=st)
    a1, mean1, inv1 = ops.batch_norm_forward_device(z1, p['gamma1'], p['beta1'], EPS, relu=True, stream=st)[:3]
    z2 = conv2(a1, stream=st)
    a2, mean2, inv2 = ops.batch_norm_forward_device(z2, p['gamma2'], p['beta2'], EPS, relu=True, stream=st)[:3]
    assert tuple(a1.shape) == (2, 10, 10, 32) and tuple(a2.shape) == (2, 8, 8, 64)
    dz2, dg2, db2 = ops.batch_norm_backward_device(z2, a2, d_r, p['gamma2'], mean2, inv2, stream=st)
    da1, dk2, _ = ops.conv_backward_strided_device(a1, p['k2'], dz2, stream=st, stride=1, padding='VALID')
    dz1, dg1, db1 = ops.batch_norm_backward_device(z1, a1, da1, p['gamma1'], mean1, inv1, stream=st)
    none, dk1, _ = ops.conv_backward_strided_device(image, p['k1'], dz1, with_dx=False, stream=st, stride=2, padding='VALID')
    st.synchronize()
    assert none is None and tuple(da1.shape) == (2, 10, 10, 32) and tuple(dz1.shape) == (2, 10, 10, 32)
    got = {'k1': to_host(dk1.ptr, (3, 3, 3, 32), f32), 'k2': to_host(dk2.ptr, (3, 3, 32, 64), f32),
           'gamma1': to_host(dg1.ptr, (32,), f32), 'beta1': to_host(db1.ptr, (32,), f32),
           'gamma2': to_host(dg2.ptr, (64,), f32), 'beta2': to_host(db2.ptr, (64,), f32)}
    out = a2.numpy()
    assert (out == 0).any() and (out > 0).any()
    bar = CS.chain_bar()
    d = chain_distances(got, ref, den)
    print('stem chain: distance / bar = %s' % ', '.join('%s %.4f' % (n, d[n] / bar) for n in NAMES))
    for n in NAMES:
        assert got[n].any() and d[n] <= bar, (n, d[n] / bar)
