"""A conv layer's operand buffers (csrc/conv_repack.hip: the padded matrix, the per-row power-of-two pre-scale, the f16
hi / lo split, the K-blocked copies, the x8 records, the rescaled epilogue scale) against a reference that shares nothing
with them: convolutions whose arithmetic is exact, so that the output is fixed by the mathematics alone and must equal a
float64 NumPy convolution bit for bit -- for a layer as created and for one created from other values and refreshed to
these (xdet_conv_set_kernel_device), in every precision mode, through every forward door.

Why the arithmetic is exact.  A weight is an integer in [-8, 8] times one power of two 2^p per output channel, an input an
integer in [-4, 4]: a product is at most 32 * 2^p in magnitude and the longest reduction has K = 15 * 64 = 960 terms, so every
partial sum is an integer below 2^24 times 2^p and no f32 addition rounds, in any order.  In the split modes the row's
pre-scale brings its largest weight m * 2^p (m <= 8) into [512, 1024): every weight becomes an integer of at most 1023, which
f16 holds exactly (hi exact, lo zero), the inputs are f16-exact too (their lo plane is zero, so f16x3 drops nothing and the
fp8 cross terms of the x8 door are zero whatever fp8 makes of the hi parts), the partial sums stay below 960 * 4 * 1024 <
2^24, and the epilogue scale undoes the pre-scale by a power of two.  Where a case has an epilogue its scale is a power of
two 2^q, q in -1 .. 2, and its shift an integer J in [-16, 16] times the row's 2^p: (I 2^q + J) 2^p needs at most
24 bits, so the result is exact with or without FMA contraction.  Channels 2 and 3 carry 2^-100 and 2^+100: far from f32's
denormals and its overflow after the 2^15 the sums can add.  An accumulator starts at +0, so a sum that vanishes is +0 on the
device; `+ 0.0` gives the reference's zeros the same sign.

The grouped operands (a SpectralConv's per-bin block matrices) are not exact arithmetic: they are compared with the float64
direct convolution of tests/test_gpu_spectral.py at that file's tolerance."""
import numpy as np
import pytest

from test_gpu_optimizer import CONV_CASES, bits, dense, doors, kernels

f32, f64 = np.float32, np.float64
CASES = sorted(c for c in CONV_CASES if c != '1x1 728->728')
MODES = ['f32', 'f16', 'f16x3']


def exact_case(case):
    """-> (w [kh,kw,cin,cout], scale, shift (None without an epilogue), x [2,8,8,cin]): f32 arrays of the values above"""
    kh, kw, cin, cout, affine = CONV_CASES[case]
    rng = np.random.default_rng(sum(case.encode()))
    ints = rng.integers(-8, 9, (kh, kw, cin, cout))
    ints[..., 0] = 0                                                    # a zero row
    ints[..., 1] = np.clip(ints[..., 1], -5, 5)
    ints[kh // 2, kw // 2, cin // 2, 1] = -8                            # a row whose maximum is exactly a power of two
    p = rng.choice([-3, 0, 5], cout)
    p[2], p[3] = -100, 100
    pow2 = np.ldexp(1.0, p)
    w = (ints * pow2).astype(f32)
    scale = np.ldexp(1.0, rng.integers(-1, 3, cout)).astype(f32) if affine else None
    shift = (rng.integers(-16, 17, cout) * pow2).astype(f32) if affine else None
    x = rng.integers(-4, 5, (2, 8, 8, cin)).astype(f32)
    return w, scale, shift, x


def conv64(x, w, scale, shift):
    """SAME, stride 1, in float64: out[n, y, x] = sum over taps of x[n, y + i - (kh-1)//2, x + j - (kw-1)//2] @ w[i, j]"""
    kh, kw = w.shape[:2]
    N, H, W, _ = x.shape
    xp = np.zeros((N, H + kh - 1, W + kw - 1, x.shape[3]), f64)
    xp[:, (kh - 1) // 2:(kh - 1) // 2 + H, (kw - 1) // 2:(kw - 1) // 2 + W] = x
    out = np.zeros((N, H, W, w.shape[3]), f64)
    for i in range(kh):
        for j in range(kw):
            out += xp[:, i:i + H, j:j + W] @ w[i, j].astype(f64)
    if scale is not None:
        out = out * scale.astype(f64) + shift.astype(f64)
    return out + 0.0


@pytest.fixture(scope='module')
def exact():
    """case -> (w, scale, shift, x, the float64 reference), computed once"""
    out = {}
    for case in CASES:
        w, scale, shift, x = exact_case(case)
        out[case] = (w, scale, shift, x, conv64(x, w, scale, shift))
    return out


def test_the_reference_is_exact_in_f32(exact):
    """no GPU: the float64 convolution of every case survives the cast to float32 unchanged, and its values are the ones the
    docstring's bounds speak of"""
    for case, (w, scale, shift, x, ref) in exact.items():
        kh, kw, cin, cout, affine = CONV_CASES[case]
        assert np.array_equal(ref.astype(f32).astype(f64), ref), case
        assert np.isfinite(ref.astype(f32)).all() and kh * kw * cin <= 960
        m, _ = np.frexp(np.abs(w).max(axis=(0, 1, 2)))
        assert not w[..., 0].any() and m[1] == 0.5 and (m[2:] > 0).all(), case      # the zero row, the power-of-two maximum
        assert np.abs(w[..., 2]).max() <= 2.0 ** -97 and np.abs(w[..., 3]).max() >= 2.0 ** 100
        assert (ref[..., 1:] != 0).mean() > 0.5, case


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES)
def test_created_and_refreshed_layers_equal_the_float64_conv_bit_for_bit(case, mode, exact):
    from xdet.ops import Conv2D
    from xdet.runtime import DeviceTensor, get_precision, set_precision, synchronize, to_device
    kh, kw, cin, cout, affine = CONV_CASES[case]
    w, scale, shift, x, ref = exact[case]
    want = bits(ref.astype(f32))
    other = kernels(kh, kw, cin, cout, 11)[1]                           # rows of other magnitudes: other pre-scales
    before = get_precision()
    set_precision(mode)
    try:
        created = Conv2D(w, scale=scale, shift=shift)
        refreshed = Conv2D(other, scale=scale, shift=None if shift is None else -shift)
    finally:
        set_precision(before)
    refreshed.set_kernel_device(dense(w), shift=to_device(shift) if affine else None)
    synchronize()
    xd = DeviceTensor.from_numpy(x)
    split = mode != 'f32' and cin > 4
    for name, layer in (('created', created), ('refreshed', refreshed)):
        got = doors(layer, xd, mode, kh == kw == 1, cin)
        assert len(got) == 1 + split + (split and mode == 'f16x3' and kh == kw == 1), (name, sorted(got))
        for door, g in got.items():
            bad = g != want
            print('%s %s %s %s: %d of %d words differ from the float64 conv' % (case, mode, name, door, int(bad.sum()), g.size))
            assert g.shape == want.shape and not bad.any(), (name, door, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('axis', [0, 1])
def test_grouped_operands_of_a_spectral_conv(axis, oracle):
    """F = 16, 32 -> 32 channels, 15 taps: the per-bin block matrices are one grouped layer, repacked in one launch"""
    from test_gpu_spectral import distance, make_layer, reference64, restatement32, run
    rng = np.random.default_rng(40 + axis)
    x = rng.standard_normal((2, 16, 16, 32)).astype(f32)
    w = (rng.standard_normal((15, 32, 32)) / np.sqrt(15 * 32)).astype(f32)
    scale, shift = rng.uniform(0.5, 1.5, 32).astype(f32), rng.standard_normal(32).astype(f32)
    ref = reference64(oracle, x, w, axis, scale, shift)
    bar = max(3e-5, 4 * distance(restatement32(x, w, axis, scale, shift), ref))      # test_gpu_spectral.py's bar, for this case
    got = run(make_layer(w, axis, 16, scale, shift), x)
    d = distance(got[..., :32], ref)
    print('spectral F16 axis %d: distance %.3e, bar %.3e' % (axis, d, bar))
    assert np.isfinite(got).all() and d <= bar, (d, bar)
