"""The optimizer step's ops on the GPU (csrc/optimizer.hip): xdet_momentum_step against its NumPy statement bit for bit and
its l2 against float64 within the rounding bound of the documented order; xdet_conv_set_kernel_device and
xdet_depthwise_set_kernel_device (csrc/conv_repack.hip) against a layer built from the same values, through every forward door
the layer has (the conv's creation runs the same repack: what its bits must be is tests/test_gpu_conv_operands.py's)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
CHUNK = 4096                                            # xdet_momentum_step's chunk (include/xdet.h)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the momentum step ------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 3] + [2 ** k + d for k in range(5, 15) for d in (-1, 0, 1)] + [6552, 529984]


@pytest.fixture(scope='module')
def table():
    """one packed array per role; slot i starts on a 16-byte boundary unless i % 3 == 1, so both access widths are taken at
    sizes on either side of the vector and the chunk.  Values: normal ones, +-0 and f32 denormals in all three roles"""
    rng = np.random.default_rng(7)
    offs, at = [], 0
    for i, n in enumerate(SIZES):
        if i % 3 != 1:
            at = -(-at // 4) * 4
        offs.append(at)
        at += n
    total = at
    special = np.array([0.0, -0.0, 1e-40, -1e-42, 1.4e-45, -1.17e-38], f32)

    def draw(scale):
        a = (rng.standard_normal(total) * scale).astype(f32)
        idx = rng.choice(total, total // 16, replace=False)
        a[idx] = special[rng.integers(0, len(special), len(idx))]
        return a
    return {'offs': offs, 'total': total, 'var': draw(0.1), 'grad': draw(0.01), 'accum': draw(0.02),
            'decay': [i % 2 == 0 for i in range(len(SIZES))]}


def device_slots(t, var, grad, accum):
    from xdet.runtime import DeviceTensor
    view = lambda b, o, n: DeviceTensor(b.ptr + 4 * o, (n,), n, owner=b)
    return [(view(var, o, n), view(grad, o, n), view(accum, o, n), n, d) for o, n, d in zip(t['offs'], SIZES, t['decay'])]


def test_momentum_step_equals_the_host_statement(table):
    from xdet import host_momentum_step, momentum_step_device
    from xdet.runtime import to_device, to_host, synchronize
    t = table
    var, grad, accum = to_device(t['var']), to_device(t['grad']), to_device(t['accum'])
    slots = device_slots(t, var, grad, accum)
    hv, ha = t['var'].copy(), t['accum'].copy()
    m, wd = 0.9, 2e-4
    for lr in (0.1, 0.01, 0.5):
        momentum_step_device(slots, lr, m, wd)
        synchronize()
        for o, n, d in zip(t['offs'], SIZES, t['decay']):
            hv[o:o + n], ha[o:o + n] = host_momentum_step(hv[o:o + n], t['grad'][o:o + n], ha[o:o + n], lr, m, wd, d)
        gv, ga = to_host(var.ptr, (t['total'],)), to_host(accum.ptr, (t['total'],))
        assert np.array_equal(bits(ga), bits(ha)), ('accum', lr, int((bits(ga) != bits(ha)).sum()))
        assert np.array_equal(bits(gv), bits(hv)), ('var', lr, int((bits(gv) != bits(hv)).sum()))
    assert np.array_equal(bits(to_host(grad.ptr, (t['total'],))), bits(t['grad']))
    # (the gaps between the slots were drawn too: they are nobody's and keep their bits)
    assert (np.abs(ha) > 0).any() and not np.array_equal(hv, t['var'])


def test_l2_is_reproducible_and_within_the_bound_of_its_order(table):
    from xdet import momentum_step_device
    from xdet.runtime import to_device, to_host, synchronize
    t = table
    got = []
    for _ in range(2):
        var, grad, accum = to_device(t['var']), to_device(t['grad']), to_device(t['accum'])
        l2 = momentum_step_device(device_slots(t, var, grad, accum), 0.1, 0.9, 2e-4, l2=True)
        synchronize()
        got.append(to_host(l2.ptr, (1,)))
    assert bits(got[0])[0] == bits(got[1])[0]
    want = sum(float((t['var'][o:o + n].astype(f64) ** 2).sum()) for o, n, d in zip(t['offs'], SIZES, t['decay']) if d) / 2
    # the order of include/xdet.h: a term is squared (1 rounding) and passes 2 levels inside its vector, 2 over the thread's
    # vectors, 8 over the chunk's threads and ceil(log2(chunks)) over the chunk partials; the halving is exact.  All terms
    # are non-negative, so the relative error is at most gamma_k = k u / (1 - k u)
    chunks = sum(-(-n // CHUNK) for n in SIZES)
    k = 1 + 2 + 2 + 8 + math.ceil(math.log2(chunks))
    u = 2.0 ** -24
    bound = k * u / (1 - k * u)
    assert bound <= 64 * u, (k, chunks)
    err = abs(float(got[0][0]) - want) / want
    print('l2 = %.9g, float64 %.9g: relative error %.3g, bound %.3g (%d roundings, %d chunks)' % (got[0][0], want, err, bound, k, chunks))
    assert want > 0 and err <= bound, (err, bound)


def test_momentum_step_refuses_in_the_library(table):
    """the C door's own refusals (the Python door's come first and are tested without a device)"""
    import ctypes
    from xdet._lib import lib, MomentumSlot
    from xdet.runtime import DeviceBuffer
    b = DeviceBuffer(64)
    ok = MomentumSlot(b.ptr, b.ptr, b.ptr, 4, 1)
    for tab, n in (((MomentumSlot * 1)(ok), 0), ((MomentumSlot * 1)(MomentumSlot(b.ptr, None, b.ptr, 4, 1)), 1),
                   ((MomentumSlot * 2)(ok, MomentumSlot(b.ptr, b.ptr, b.ptr, 0, 0)), 2)):
        assert lib().xdet_momentum_step(tab, n, 0.1, 0.9, 0.0, None, b.ptr, None) == -1
    assert lib().xdet_momentum_step(None, 1, 0.1, 0.9, 0.0, None, b.ptr, None) == -1
    assert lib().xdet_momentum_step((MomentumSlot * 1)(ok), 1, 0.1, 0.9, 0.0, None, None, None) == -1
    assert lib().xdet_momentum_step_workspace_bytes((MomentumSlot * 1)(ok), 1) > 0
    assert lib().xdet_momentum_step_workspace_bytes((MomentumSlot * 1)(ok), 0) == 0
    del ctypes


# ---- the conv refresh ----------------------------------------------------------------------------------------------------------

CONV_CASES = {                                          # name: (kh, kw, cin, cout, creation-time scale and a new shift)
    '1x1 24->40': (1, 1, 24, 40, False), '1x1 72->136': (1, 1, 72, 136, False), '1x1 728->728': (1, 1, 728, 728, False),
    '1x1 32->64 scale+shift': (1, 1, 32, 64, True), '3x3 3->32': (3, 3, 3, 32, False), '3x3 40->64': (3, 3, 40, 64, False),
    '15x1 64->32': (15, 1, 64, 32, False)}


def kernels(kh, kw, cin, cout, seed):
    """-> (W0, W1): W1 with a zero row, a row whose maximum is exactly a power of two, a row of magnitude 1e-30 and one of
    1e+30 (a row = an output channel)"""
    rng = np.random.default_rng(seed)
    std = 1.0 / math.sqrt(kh * kw * cin)
    w0 = (rng.standard_normal((kh, kw, cin, cout)) * std).astype(f32)
    w1 = (rng.standard_normal((kh, kw, cin, cout)) * std).astype(f32)
    w1[..., 0] = 0
    w1[..., 1] = np.clip(w1[..., 1], -0.2, 0.2)
    w1[kh // 2, kw // 2, cin // 2, 1] = -0.25
    w1[..., 2] *= f32(1e-30)
    w1[..., 3] *= f32(1e+30)
    return w0, w1


def dense(a):
    from xdet.runtime import DeviceTensor, to_device
    b = to_device(a)
    return DeviceTensor(b.ptr, a.shape, a.shape[-1], owner=b)


def doors(layer, x, mode, pointwise, cin):
    """the layer's output on x through every forward door it has -> {door: bits}"""
    from xdet.runtime import synchronize
    out = {'forward': layer(x)}
    if mode != 'f32' and cin > 4:
        out['planes'] = layer(x, planes=True)
        if mode == 'f16x3' and pointwise:
            m, e = np.frexp(float(np.abs(x.numpy()).max()))               # max|x| 2^-e in (128, 256]
            out['planes_x8'] = layer(x, planes=True, x8_exp=int(e) - 8 - (1 if m == 0.5 else 0))
    synchronize()
    return {k: bits(v.numpy()) for k, v in out.items()}


@pytest.mark.parametrize('mode', ['f32', 'f16', 'f16x3'])
@pytest.mark.parametrize('case', sorted(CONV_CASES))
def test_conv_refresh_equals_a_fresh_layer(case, mode):
    from xdet.ops import Conv2D
    from xdet.runtime import DeviceTensor, get_precision, set_precision, synchronize, to_device
    kh, kw, cin, cout, affine = CONV_CASES[case]
    w0, w1 = kernels(kh, kw, cin, cout, 5)
    rng = np.random.default_rng(9)
    scale = rng.uniform(0.5, 2.0, cout).astype(f32) if affine else None
    sh0, sh1 = ((rng.standard_normal(cout).astype(f32) for _ in range(2)) if affine else (None, None))
    x = DeviceTensor.from_numpy(rng.standard_normal((2, 8, 8, cin)).astype(f32))
    before = get_precision()
    set_precision(mode)
    try:
        layer, fresh = Conv2D(w0, scale=scale, shift=sh0), Conv2D(w1, scale=scale, shift=sh1)
    finally:
        set_precision(before)
    old = doors(layer, x, mode, kh == kw == 1, cin)
    layer.set_kernel_device(dense(w1), shift=to_device(sh1) if affine else None)
    synchronize()
    got, want = doors(layer, x, mode, kh == kw == 1, cin), doors(fresh, x, mode, kh == kw == 1, cin)
    split = mode != 'f32' and cin > 4                    # the layer has K-blocked copies: the planes door, and x8 where pointwise
    assert set(got) == set(want) and len(got) == 1 + split + (split and mode == 'f16x3' and kh == kw == 1)
    for door in want:
        assert np.array_equal(got[door], want[door]), (door, int((got[door] != want[door]).sum()), got[door].size)
        assert not np.array_equal(got[door], old[door]), door
    # a second refresh, back to W0 (and the old shift), gives the first layer again: nothing of W1 is left in any buffer
    layer.set_kernel_device(dense(w0), shift=to_device(sh0) if affine else None)
    synchronize()
    back = doors(layer, x, mode, kh == kw == 1, cin)
    for door in old:
        assert np.array_equal(back[door], old[door]), door


def test_conv_refresh_refusals_leave_the_layer_unchanged():
    import xdet
    from xdet.ops import Conv2D, SpectralConv
    from xdet.runtime import DeviceBuffer, DeviceTensor, get_precision, set_precision, synchronize
    from xdet._lib import lib
    rng = np.random.default_rng(3)
    w0, w1 = kernels(1, 1, 32, 64, 2)
    x = DeviceTensor.from_numpy(rng.standard_normal((1, 8, 8, 32)).astype(f32))
    before = get_precision()
    set_precision('f16x3')
    try:
        layer = Conv2D(w0)
        spectral = SpectralConv((rng.standard_normal((15, 32, 32)) * 0.05).astype(f32), 0, 16)
    finally:
        set_precision(before)
    was = bits(layer(x).numpy())
    # a wrong shape, a host array: the Python door
    for bad in (dense(w1.transpose(0, 1, 3, 2).copy()), w1, DeviceTensor(dense(w1).ptr, w1.shape, 96)):
        with pytest.raises(xdet.InvalidArgumentError, match='Conv2D.set_kernel_device: a dense DeviceTensor of shape'):
            layer.set_kernel_device(bad)
    with pytest.raises(xdet.InvalidArgumentError, match='shift must be a device array'):
        layer.set_kernel_device(dense(w1), shift=np.zeros(64, f32))
    assert np.array_equal(bits(layer(x).numpy()), was)
    # a calibrated layer: a planes exponent set through the emit door
    n_pix = 64
    hi, lo = DeviceBuffer(n_pix * 64 * 2 + 512, zero=True), DeviceBuffer(n_pix * 64 * 2 + 512, zero=True)
    out = DeviceTensor.empty((1, 8, 8, 64))
    layer.emit(x=x, out=out, out_planes=(hi, lo), out_exp=1)
    cal = bits(out.numpy())
    with pytest.raises(xdet.InvalidArgumentError, match='carries an activation or planes exponent'):
        layer.set_kernel_device(dense(w1))
    synchronize()
    assert np.array_equal(bits(layer(x).numpy()), was) and np.array_equal(cal, was)
    # a grouped layer exists only inside a spectral one, whose handle the door refuses
    xs = DeviceTensor.from_numpy(rng.standard_normal((1, 16, 16, 32)).astype(f32))
    s_was = bits(spectral(xs).numpy())
    assert lib().xdet_conv_set_kernel_device(spectral.handle, dense(w1).ptr, None, None) == -1
    assert b'spectral' in lib().xdet_last_error()
    assert np.array_equal(bits(spectral(xs).numpy()), s_was)
    assert lib().xdet_conv_set_kernel_device(layer.handle, None, None, None) == -1


# ---- the depthwise refresh -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dil', [1, 2])
@pytest.mark.parametrize('C', [24, 728])
def test_depthwise_refresh_equals_a_fresh_layer(C, dil):
    import xdet
    from xdet.ops import DepthwiseConv2D
    from xdet.runtime import DeviceTensor, synchronize
    rng = np.random.default_rng(C + dil)
    k0, k1 = ((rng.standard_normal((3, 3, C, 1)) * 0.3).astype(f32) for _ in range(2))
    k1[:, :, 0] = 0
    k1[1, 1, 1] = -0.0
    x = DeviceTensor.from_numpy(rng.standard_normal((2, 8, 8, C)).astype(f32))
    layer, fresh = DepthwiseConv2D(k0, dil), DepthwiseConv2D(k1, dil)
    old = bits(layer(x, relu_in=True).numpy())
    with pytest.raises(xdet.InvalidArgumentError, match='DepthwiseConv2D.set_kernel_device'):
        layer.set_kernel_device(dense(k1.reshape(3, 3, 1, C)))
    layer.set_kernel_device(dense(k1))
    synchronize()
    for relu_in in (False, True):
        got, want = bits(layer(x, relu_in=relu_in).numpy()), bits(fresh(x, relu_in=relu_in).numpy())
        assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(bits(layer(x, relu_in=True).numpy()), old)
