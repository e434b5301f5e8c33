"""xdet_bn_fold and the table door xdet_layers_refresh_device (csrc/conv_repack.hip) at op level.
The fold equals xdet.ops.host_bn_fold bit for bit at channel counts on both sides of the wave and the workgroup.  One table per
precision holds every layer of LAYERS, each created from one set of values and refreshed from another: afterwards its forward,
through every door the layer has (f32 input, split planes, the x8 planes of a pointwise f16x3 layer), equals bit for bit that of
a layer created from the new values (scale and shift included) and that of the same layer refreshed through the per-layer door.
The new kernels hold a zero row, a row whose maximum is a power of two and rows of magnitude 1e-30 and 1e+30 (other pre-scales
than the old rows'), so a word of the old kernel left anywhere in a row or in the padded rows' scale would show.  Every refusal
leaves the layers of the table producing their old bits."""
import numpy as np
import pytest

from test_gpu_optimizer import bits, dense, doors, kernels

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = ['f32', 'f16', 'f16x3']
# name: (kh, kw, cin, cout, padding, new scale, new shift)
LAYERS = {'1x1 32->64': (1, 1, 32, 64, 'SAME', False, False), '1x1 24->40': (1, 1, 24, 40, 'SAME', True, True),
          '1x1 728->728': (1, 1, 728, 728, 'SAME', True, True), '3x3 VALID 3->32': (3, 3, 3, 32, 'VALID', False, False),
          '3x3 SAME 728->512': (3, 3, 728, 512, 'SAME', False, True), '1x1 72->136 zero row': (1, 1, 72, 136, 'SAME', True, False)}
DEPTHWISE = {'dw 24': (24, 1), 'dw 728 dil 2': (728, 2)}


@pytest.mark.parametrize('C', [1, 31, 32, 33, 728, 2048])
@pytest.mark.parametrize('with_bias', [False, True])
def test_bn_fold_equals_the_host_statement(C, with_bias):
    from xdet.ops import bn_fold_device, host_bn_fold
    from xdet.runtime import synchronize, to_device, to_host
    rng = np.random.default_rng(C)
    g, b, m = (rng.standard_normal(C).astype(f32) for _ in range(3))
    v = rng.uniform(1e-6, 4.0, C).astype(f32)
    bias = rng.standard_normal(C).astype(f32) if with_bias else None
    special = np.array([0.0, -0.0, 1e-40, -1e-42], f32)[:min(C, 4)]
    b[:special.size], m[:special.size] = special, special[::-1]         # -0 and denormals in the shift's terms
    g[-1] = f32(-0.0)
    eps = 1e-4
    sc, sh = bn_fold_device(*(to_device(a) for a in (g, b, m, v)), eps, bias=to_device(bias) if with_bias else None, C=C)
    synchronize()
    want_sc, want_sh = host_bn_fold(g, b, m, v, eps, bias)
    assert np.array_equal(bits(to_host(sc.ptr, (C,))), bits(want_sc))
    assert np.array_equal(bits(to_host(sh.ptr, (C,))), bits(want_sh))


def values(name, seed):
    kh, kw, cin, cout, _, _, _ = LAYERS[name]
    w0, w1 = kernels(kh, kw, cin, cout, seed)
    rng = np.random.default_rng(seed + 1)
    return w0, w1, rng.uniform(0.5, 2.0, (2, cout)).astype(f32), rng.standard_normal((2, cout)).astype(f32)


def make(mode):
    """-> per layer name (the layer created from the old values, (kernel, scale, shift) it is to be refreshed with, a layer
    created from the new values, input)"""
    from xdet.ops import Conv2D, DepthwiseConv2D
    from xdet.runtime import DeviceTensor, get_precision, set_precision
    before = get_precision()
    set_precision(mode)
    out = {}
    try:
        for i, name in enumerate(sorted(LAYERS)):
            kh, kw, cin, cout, pad, new_scale, new_shift = LAYERS[name]
            w0, w1, sc, sh = values(name, 20 + i)
            old = lambda w0=w0, pad=pad, sc=sc, sh=sh: Conv2D(w0, padding=pad, scale=sc[0], shift=sh[0])
            fresh = Conv2D(w1, padding=pad, scale=sc[1] if new_scale else sc[0], shift=sh[1] if new_shift else sh[0])
            x = DeviceTensor.from_numpy(np.random.default_rng(40 + i).standard_normal((1, 6, 7, cin)).astype(f32))
            out[name] = (old, (w1, sc[1] if new_scale else None, sh[1] if new_shift else None), fresh, x)
        for i, name in enumerate(sorted(DEPTHWISE)):
            C, dil = DEPTHWISE[name]
            rng = np.random.default_rng(60 + i)
            k0, k1 = (rng.standard_normal((3, 3, C, 1)).astype(f32) for _ in range(2))
            x = DeviceTensor.from_numpy(rng.standard_normal((1, 6, 7, C)).astype(f32))
            out[name] = ((lambda k0=k0, dil=dil: DepthwiseConv2D(k0, dil)), (k1, None, None), DepthwiseConv2D(k1, dil), x)
    finally:
        set_precision(before)
    return out


def run(name, layer, x, mode):
    from xdet.runtime import synchronize
    if name in DEPTHWISE:
        y = layer(x)
        synchronize()
        return {'forward': bits(y.numpy())}
    kh, kw, cin = LAYERS[name][:3]
    return doors(layer, x, mode, kh == kw == 1 and LAYERS[name][4] == 'SAME', cin)


def same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('mode', MODES)
def test_one_table_equals_fresh_layers_and_the_per_layer_door(mode):
    from xdet.ops import refresh_layers_device
    from xdet.runtime import get_precision, set_precision, synchronize, to_device
    before = get_precision()
    set_precision(mode)
    try:
        cases = make(mode)
        table, single = {n: c[0]() for n, c in cases.items()}, {n: c[0]() for n, c in cases.items()}
    finally:
        set_precision(before)
    old = {n: run(n, table[n], cases[n][3], mode) for n in cases}
    dev = {n: tuple(None if a is None else (dense(a) if a.ndim == 4 else to_device(a)) for a in cases[n][1]) for n in cases}
    refresh_layers_device([(table[n],) + dev[n] for n in sorted(cases)])
    for n in cases:
        if n in DEPTHWISE:
            single[n].set_kernel_device(dev[n][0])
        elif dev[n][1] is None:                      # (the per-layer door has no scale: only layers that keep theirs)
            single[n].set_kernel_device(dev[n][0], shift=dev[n][2])
    synchronize()
    for n in sorted(cases):
        got, fresh = run(n, table[n], cases[n][3], mode), run(n, cases[n][2], cases[n][3], mode)
        assert same(got, fresh), (n, mode, {k: int((got[k] != fresh[k]).sum()) for k in got})
        assert not same(got, old[n]), n
        if n in DEPTHWISE or dev[n][1] is None:
            assert same(got, run(n, single[n], cases[n][3], mode)), n


def test_refusals_leave_every_layer_as_it_was():
    import xdet
    from xdet._lib import LayerRefresh, lib
    from xdet.ops import Conv2D, refresh_layers_device
    from xdet.runtime import DeviceBuffer, get_precision, set_precision, to_device
    mode = 'f16x3'
    before = get_precision()
    set_precision(mode)
    try:
        cases = make(mode)
        names = ['1x1 24->40', '1x1 32->64', 'dw 24']
        layers = {n: cases[n][0]() for n in names}
    finally:
        set_precision(before)
    old = {n: run(n, layers[n], cases[n][3], mode) for n in names}
    k = {n: dense(cases[n][1][0]) for n in names}
    good = [(layers[n], k[n]) for n in names]
    sc = to_device(np.ones(64, f32))
    table = (LayerRefresh * 3)(*[LayerRefresh(layers[n].handle, k[n].ptr, None, None) for n in names])
    ws = DeviceBuffer(lib().xdet_layers_refresh_workspace_bytes(table, 3))
    assert ws.nbytes > 0
    null_kernel = (LayerRefresh * 3)(*table)
    null_kernel[2].kernel = None
    null_layer = (LayerRefresh * 3)(*table)
    null_layer[1].layer = None
    for what, call in (('empty', lambda: lib().xdet_layers_refresh_device(table, 0, ws.ptr, None)),
                       ('NULL table', lambda: lib().xdet_layers_refresh_device(None, 3, ws.ptr, None)),
                       ('NULL kernel', lambda: lib().xdet_layers_refresh_device(null_kernel, 3, ws.ptr, None)),
                       ('NULL layer', lambda: lib().xdet_layers_refresh_device(null_layer, 3, ws.ptr, None)),
                       ('NULL workspace', lambda: lib().xdet_layers_refresh_device(table, 3, None, None))):
        assert call() == -1, what
    for what, slots, word in (('twice', good + [good[0]], 'twice'),
                              ('scale on a depthwise slot', good[:2] + [(layers['dw 24'], k['dw 24'], sc)], 'depthwise'),
                              ('a host kernel', good[:2] + [(layers['dw 24'], cases['dw 24'][1][0])], 'device memory'),
                              ('empty', [], 'empty')):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            refresh_layers_device(slots)
        assert word in str(e.value), (what, str(e.value))
    for n in names:
        assert same(run(n, layers[n], cases[n][3], mode), old[n]), n
    # and the per-layer doors keep their own refusals: a refreshed layer still takes them
    refresh_layers_device(good, workspace=ws)
    layers['1x1 24->40'].set_kernel_device(k['1x1 24->40'])
    assert isinstance(layers['1x1 32->64'], Conv2D)


def test_refused_layer_kinds_leave_every_layer_as_it_was():
    """a layer whose planes copy carries a folded batch norm (a Conv2D that has run emit(bn=...)) and a spectral layer, each in a
    table with good layers: refused by name of the reason, through the Python door and through the C table, with every layer
    -- the refused one too -- producing its old bits.  (A grouped layer cannot be built through the C ABI: xdet_conv_create
    takes no group count, and a SpectralConv's grouped GEMM is not a handle.)"""
    import xdet
    from xdet._lib import LayerRefresh, lib
    from xdet.ops import SpectralConv, refresh_layers_device
    from xdet.runtime import DeviceBuffer, DeviceTensor, get_precision, set_precision, synchronize, to_device
    mode = 'f16x3'
    before = get_precision()
    set_precision(mode)
    try:
        cases = make(mode)
        names = ['1x1 24->40', 'dw 24']
        layers = {n: cases[n][0]() for n in names}
        with_bn = cases['1x1 32->64'][0]()
        rng = np.random.default_rng(80)
        spectral = SpectralConv((rng.standard_normal((3, 32, 32)) * 0.1).astype(f32), 0, 16)
    finally:
        set_precision(before)
    x_bn = cases['1x1 32->64'][3]
    n_pix = -(-x_bn.shape[0] * x_bn.shape[1] * x_bn.shape[2] // 16) * 16
    planes = DeviceBuffer(n_pix * 64 * 2 + 512, zero=True), DeviceBuffer(n_pix * 64 * 2 + 512, zero=True)
    with_bn.emit(x=x_bn, out=DeviceTensor.empty(x_bn.shape[:3] + (64,)), out_planes=planes,
                 bn=(rng.uniform(0.5, 2.0, 64).astype(f32), rng.standard_normal(64).astype(f32)))
    x_sp = DeviceTensor.from_numpy(rng.standard_normal((1, 16, 16, 32)).astype(f32))

    def all_bits():
        out = {n: run(n, layers[n], cases[n][3], mode) for n in names}
        out['with_bn'] = run('1x1 32->64', with_bn, x_bn, mode)
        y = spectral(x_sp)
        synchronize()
        out['spectral'] = {'forward': bits(y.numpy())}
        return out
    old = all_bits()
    k = {n: dense(cases[n][1][0]) for n in names}
    good = [(layers[n], k[n]) for n in names]
    refused = {'folded batch norm': (with_bn, dense(cases['1x1 32->64'][1][0])),
               'spectral': (spectral, to_device(np.zeros(3 * 32 * 32, f32)))}
    ws = DeviceBuffer(1 << 20)
    for word, slot in refused.items():
        for slots in (good + [slot], [slot] + good):
            with pytest.raises(xdet.InvalidArgumentError) as e:
                refresh_layers_device(slots, workspace=ws)
            assert word in str(e.value), (word, str(e.value))
            table = (LayerRefresh * len(slots))(*[LayerRefresh(s[0].handle, s[1].ptr, None, None) for s in slots])
            assert lib().xdet_layers_refresh_workspace_bytes(table, len(slots)) == 0
            assert lib().xdet_layers_refresh_device(table, len(slots), ws.ptr, None) == -1
            assert word in lib().xdet_last_error().decode(), (word, lib().xdet_last_error())
    new = all_bits()
    for n in old:
        assert same(new[n], old[n]), n
    # the good layers alone go through, so it was the refused slot that stopped each table
    refresh_layers_device(good, workspace=ws)
    synchronize()
    assert not same(run('dw 24', layers['dw 24'], cases['dw 24'][3], mode), old['dw 24'])
