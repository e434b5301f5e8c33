"""The spectral convolution layer (csrc/spectral.hip: dft_fwd_kernel -> grouped per-bin GEMM of conv_mfma_dma.hip ->
dft_inv_kernel; xdet_spectral_conv_*, the layer LightHeadNet::build_large_sep_spectral is made of) on its own, in f16x3,
against the float64 direct convolution oracle.conv2d(..., 'SAME', dtype=float64) (* scale + shift, ReLU): every supported
map side and both axes, channel counts that leave early-return waves (ld / 32 not a multiple of 4) and padded outputs,
line counts that are no multiple of 8, bins whose padding rows hold poison, an output tensor wider than the layer, and
every launch form of the two transforms (bin deals z = 6 / 4 / 2 / 1, inverse forms ZI = 2 / 1) with image 0 bit-equal
across them.

Tolerance: the NumPy restatement of tests/test_spectral_math.py (tables, weights) evaluated with float32 operands and
float32 accumulation is measured against the float64 direct conv over the cases of this file, relative to
max(1, |ref|.max()); the bar is max(3e-5, 4 x that distance) -- 3e-5 is the f16x3 conv bar of tests/test_gpu_layers.py, the
factor 4 that of tests/test_gpu_losses.py (summation order and the f16x3 cross terms differ from the restatement's).
The restatement's distance, measured on the CPU: 2.8e-07, so the bar is its 3e-5 floor.  The largest distance measured on an
MI355X over all cases of this file is 0.012 of that bar (3.5e-07: the last image of the 35-image launch-form case; the
shape cases reach 0.011)."""

import numpy as np
import pytest

from test_spectral_math import tables, weights

pytestmark = pytest.mark.gpu
f32 = np.float32

# name: (F, axis, N, cin, cout, affine + ReLU, extra channels of the output tensor)
CASES = {}
for _F, _N in ((16, 2), (30, 1), (50, 1)):        # N*F = 32 (m_pad 128), 30 and 50 (not multiples of 8: a ragged last wave row)
    for _ax in (0, 1):
        CASES['F%d_axis%d' % (_F, _ax)] = (_F, _ax, _N, 40, 70, True, 0)       # ld 64: waves 2, 3 of dft_fwd return early; cout -> 96
CASES['F30_n3_96_to_490'] = (30, 0, 3, 96, 490, False, 32)   # N*F = 90; ld 96 (3 blocks), C_ld 512 inside an ld_out of 544
CASES['F50_n1_96_to_490'] = (50, 1, 1, 96, 490, True, 0)
CASES['F30_n5_m_pad_256'] = (30, 1, 5, 40, 70, True, 0)      # N*F = 150 rows live in bins of 256
# The launch forms at F = 30, cin = ld = 512 (ld / 32 = 16 -> 4 workgroups across the channels), cout 490 (C_ld 512 -> 4):
#   launch_fwd_t: wgs = ceil(30 N / 8) * 4;  z = 6 below 128, 4 below 256, 2 below 512, else 1
#   launch_inv_t: the same product;          ZI = 2 below 256, else 1
#   N =  1:   4 * 4 =  16 -> z = 6, ZI = 2        N = 18:  68 * 4 = 272 -> z = 2, ZI = 1
#   N =  9:  34 * 4 = 136 -> z = 4, ZI = 2        N = 35: 132 * 4 = 528 -> z = 1, ZI = 1
FORMS_N = (1, 9, 18, 35)
CASES['forms_image0'] = (30, 0, 1, 512, 490, True, 0)


def make_case(name):
    F, axis, N, cin, cout, affine, extra = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7 + F)
    n_gen = max(FORMS_N) if name == 'forms_image0' else N
    x = rng.standard_normal((n_gen, F, F, cin)).astype(f32)
    w = (rng.standard_normal((15, cin, cout)) / np.sqrt(15 * cin)).astype(f32)
    scale = rng.uniform(0.5, 1.5, cout).astype(f32) if affine else None
    shift = rng.standard_normal(cout).astype(f32) if affine else None
    return x, w, scale, shift


def reference64(oracle, x, w, axis, scale, shift):
    k = w[:, None] if axis == 0 else w[None]                        # (15,1) or (1,15) HWIO
    ref = oracle.conv2d(x, k, padding='SAME', dtype=np.float64)
    if scale is not None:
        ref = np.maximum(ref * scale.astype(np.float64) + shift.astype(np.float64), 0)
    return ref


def restatement32(x, w, axis, scale, shift):
    """tests/test_spectral_math.py's algorithm with float32 operands and float32 accumulation"""
    N, F, _, cin = x.shape
    cout = w.shape[2]
    fwd, inv = tables(F)
    Bm = weights(w, F)
    xm = np.moveaxis(x, axis + 1, 2)                                # [n, other, F, cin]
    A = np.concatenate([np.matmul(fwd[:, 0], xm), np.matmul(fwd[:, 1], xm)], -1)    # [n, other, NB, 2cin]
    A = np.ascontiguousarray(A.reshape(N * F, -1, 2 * cin).transpose(1, 0, 2))
    Y = np.matmul(A, Bm).transpose(1, 0, 2)                         # [m, NB, 2cout]: one real GEMM per bin
    y = np.matmul(inv[:, 0].T, Y[..., :cout]) + np.matmul(inv[:, 1].T, Y[..., cout:])   # [m, F, cout]
    assert y.dtype == f32
    got = np.moveaxis(y.reshape(N, F, F, cout), 2, axis + 1)
    if scale is not None:
        got = np.maximum(got * scale + shift, f32(0))
    return got


def distance(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.fixture(scope='module')
def refs(oracle):
    """name -> (x, w, scale, shift, float64 reference), computed once; 'bar' -> the tolerance"""
    out, worst = {}, 0.
    for name in CASES:
        F, axis, N, cin, cout, affine, extra = CASES[name]
        x, w, scale, shift = make_case(name)
        ref = reference64(oracle, x[:N], w, axis, scale, shift)
        d = distance(restatement32(x[:N], w, axis, scale, shift), ref)
        print('%s: f32 restatement vs float64 direct conv: %.3e' % (name, d))
        worst = max(worst, d)
        out[name] = (x, w, scale, shift, ref)
    assert worst > 0
    out['bar'] = max(3e-5, 4 * worst)
    print('f32 restatement vs float64: %.3e -> bar %.3e' % (worst, out['bar']))
    return out


def make_layer(w, axis, F, scale, shift):
    from xdet import ops
    from xdet.runtime import set_precision
    set_precision('f16x3')
    try:
        return ops.SpectralConv(w, axis, F, scale, shift, relu=scale is not None)
    finally:
        set_precision('f32')


def run(layer, x, extra=0):
    """forward with every byte of the workspace (the bins' padding rows among them) and of the output poisoned first"""
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, DeviceTensor, synchronize
    N, F = x.shape[0], x.shape[1]
    ws = DeviceBuffer(layer.workspace_bytes(N))
    check(lib().xdet_memset(ws.ptr, 0xA5, ws.nbytes, None))
    out = DeviceTensor.empty((N, F, F, layer.cout + extra), ld=-(-layer.cout // 32) * 32 + extra)
    check(lib().xdet_memset(out.ptr, 0xA5, N * F * F * out.ld * 4, None))
    synchronize()
    layer(DeviceTensor.from_numpy(x), out=out, workspace=ws)
    return out.numpy()


@pytest.mark.parametrize('name', [n for n in CASES if n != 'forms_image0'])
def test_spectral_conv_matches_float64_direct_conv(name, refs):
    F, axis, N, cin, cout, affine, extra = CASES[name]
    x, w, scale, shift, ref = refs[name]
    assert m_pad_rows(F, N) > N * F                              # every case has padding rows, poisoned by run()
    got = run(make_layer(w, axis, F, scale, shift), x, extra)
    assert np.isfinite(got).all()
    d = distance(got[..., :cout], ref)
    print('%s: distance / bar = %.4f (bar %.3e)' % (name, d / refs['bar'], refs['bar']))
    assert d <= refs['bar'], (name, d / refs['bar'])
    if extra:
        c_ld = -(-cout // 32) * 32
        # channels beyond round_up(cout, 32) of a wider output tensor are not the layer's: still the poison
        assert (got[..., c_ld:].view(np.uint32) == 0xA5A5A5A5).all()


def m_pad_rows(F, N):
    return 128 if N * F <= 128 else -(-N * F // 256) * 256


def test_every_launch_form_gives_image_0_the_same_bits(refs, oracle):
    """z = 6 / 4 / 2 / 1 and ZI = 2 / 1 (the arithmetic above FORMS_N): the bin deal and the split of the output positions
    change nothing in the results -- what "decided per net, never per call" rests on"""
    F, axis, _, cin, cout, affine, extra = CASES['forms_image0']
    x, w, scale, shift, ref0 = refs['forms_image0']
    layer = make_layer(w, axis, F, scale, shift)
    first = None
    for N in FORMS_N:
        got = run(layer, x[:N])
        d = distance(got[0], ref0[0])
        # the last image of the batch as well: rows far from the first workgroups
        dl = distance(got[N - 1], reference64(oracle, x[N - 1:N], w, axis, scale, shift)[0]) if N > 1 else d
        print('forms N = %d: distance / bar = %.4f (image 0), %.4f (last image)' % (N, d / refs['bar'], dl / refs['bar']))
        assert max(d, dl) <= refs['bar'], (N, d / refs['bar'], dl / refs['bar'])
        if first is None:
            first = got[0]
        assert np.array_equal(got[0].view(np.uint32), first.view(np.uint32)), N


def test_overflow_in_the_dft_domain_is_loud_at_the_op():
    """one input element above the f16 range (65504): its line's DC bin is inf in the hi plane, the GEMM makes NaN of it, and the
    NaN-keeping ReLU of dft_inv_kernel must hand it on -- not zeros (tests/test_gpu_e2e.py's
    test_overflow_in_the_dft_domain_is_loud, localised to the op)"""
    name = 'F16_axis0'
    F, axis, N, cin, cout, affine, extra = CASES[name]
    x, w, scale, shift = make_case(name)
    x[1, 5, 11, 17] = 70000.0                                       # axis 0: the line is (n = 1, x = 11), all y
    got = run(make_layer(w, axis, F, scale, shift), x)
    line = np.zeros(got.shape[:3], bool)
    line[1, :, 11] = True
    assert not np.isfinite(got[line]).any()
    assert np.isfinite(got[~line]).all()


def test_unsupported_map_side_is_refused():
    from xdet._lib import InvalidArgumentError
    w = np.zeros((15, 32, 32), f32)
    with pytest.raises(InvalidArgumentError):
        make_layer(w, 0, 32, None, None)
    from xdet import ops                                            # ... and so is a layer outside a split-precision mode
    with pytest.raises(InvalidArgumentError):
        ops.SpectralConv(w, 0, 30)
