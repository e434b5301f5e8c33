"""xdet_stem_conv3x3s2_train_forward (csrc/stem_train.hip), block1_conv1 in training mode: the raw f32 conv output from the NCHW
image, through its door (ops.stem_conv3x3s2_train), against the conv in float64.

Sizes, two images each: S = 3 (one output pixel per image), 9 (every pixel under a window), 10 (the last row and column under
none) and 35 (2 * 17 * 17 = 578 output pixels: three workgroups of 256, the last one partly filled), each at the dense pixel
stride 32, at 40 (the eight padding floats of every pixel keep the bytes they held) and at 33 (no multiple of 4: the kernel
stores element by element instead of in 16-byte vectors).

Bar, per element and derived, not measured: the kernel adds the 27 products in one f32 accumulator by fmaf, one rounding per
term, so |z - z64| <= gamma_27 * sum |x| |w| with gamma_27 = 27 u / (1 - 27 u) (the bound of a recursive sum of n terms;
Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); the test asks for 27 * 2^-24 * sum |x| |w|, the bound's
leading term.  Each case prints the largest fraction of it that an element used; on an MI355X: see DESIGN.md 4.46."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENTINEL_BYTE = 0xA5
SENTINEL32 = np.uint32(0xA5A5A5A5)
SIZES = (3, 9, 10, 35)
_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_case(S, N=2):
    """-> (images [N,3,S,S], kernel [3,3,3,32]); image 0 of the N = 1 case is image 0 of the N = 2 case"""
    if S not in _cache:
        rng = np.random.default_rng(7000 + S)
        x = rng.standard_normal((2, 3, S, S)).astype(f32)
        k = (rng.standard_normal((3, 3, 3, 32)) / np.sqrt(27)).astype(f32)
        x.setflags(write=False)
        k.setflags(write=False)
        _cache[S] = (x, k)
    x, k = _cache[S]
    return x[:N], k


def conv64(x_nchw, k):
    """-> (z, sum |x| |w|) of the conv, 3x3 / stride 2 / 'VALID', in float64, [N,Ho,Ho,32] each"""
    x = np.transpose(np.asarray(x_nchw, f64), (0, 2, 3, 1))
    k = np.asarray(k, f64)
    Ho = (x.shape[1] - 3) // 2 + 1
    z, mag = np.zeros((x.shape[0], Ho, Ho, 32)), np.zeros((x.shape[0], Ho, Ho, 32))
    for a in range(3):
        for b in range(3):
            win = x[:, a:a + 2 * Ho - 1:2, b:b + 2 * Ho - 1:2]
            z += np.matmul(win, k[a, b])
            mag += np.matmul(np.abs(win), np.abs(k[a, b]))
    return z, mag


def run(x, k, ld):
    """-> (z [N,Ho,Ho,32], the raw rows [N*Ho*Ho, ld] as uint32) of the door on a tensor that held the sentinel everywhere"""
    from xdet import ops
    from xdet._lib import lib, check
    from xdet.runtime import DeviceTensor, synchronize, to_host
    N, S = x.shape[0], x.shape[2]
    Ho = (S - 3) // 2 + 1
    out = DeviceTensor.empty((N, Ho, Ho, 32), ld=ld)
    check(lib().xdet_memset(out.ptr, SENTINEL_BYTE, N * Ho * Ho * ld * 4, None))
    synchronize()
    z = ops.stem_conv3x3s2_train(x, k, out=out)
    assert z is out and z.ld == ld
    raw = to_host(z.ptr, (N * Ho * Ho, ld), np.uint32)
    return z.numpy(), raw


@pytest.mark.parametrize('ld', [32, 40, 33])
@pytest.mark.parametrize('S', SIZES)
def test_matches_float64_within_the_fma_bound(S, ld):
    x, k = make_case(S)
    ref, mag = conv64(x, k)
    got, raw = run(x, k, ld)
    assert got.shape == ref.shape and got.dtype == f32
    bound = 27 * 2.0 ** -24 * mag
    frac = np.abs(got.astype(f64) - ref) / bound
    print('stem_conv3x3s2_train S=%d ld=%d (%d pixels): largest |z - z64| / bound = %.4f' % (S, ld, raw.shape[0], frac.max()))
    assert np.isfinite(got).all() and (frac <= 1).all(), float(frac.max())
    assert (raw[:, 32:] == SENTINEL32).all()           # the padding floats of every pixel: nobody's
    assert not (raw[:, :32] == SENTINEL32).all(axis=1).any()


def test_pixels_under_no_window_are_never_read():
    """S = 10: NaN in the last row and column changes no output bit"""
    x, k = make_case(10)
    planted = x.copy()
    planted[:, :, 9, :] = np.nan
    planted[:, :, :, 9] = np.nan
    clean, _ = run(x, k, 32)
    got, _ = run(planted, k, 32)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(clean))


@pytest.mark.parametrize('S', [10, 35])
def test_an_image_does_not_depend_on_its_batch(S):
    x, k = make_case(S)
    two, _ = run(x, k, 32)
    one, _ = run(make_case(S, 1)[0], k, 32)
    assert one.shape[0] == 1 and np.array_equal(bits(one[0]), bits(two[0]))
    assert not np.array_equal(two[0], two[1])


def test_the_door_refuses_ahead_of_any_launch():
    """every refusal leaves the sentinel: nothing was launched"""
    from xdet._lib import lib
    from xdet.runtime import DeviceBuffer, synchronize, to_device, to_host
    l = lib()
    x, k = make_case(9)
    d_x, d_k = to_device(np.ascontiguousarray(x)), to_device(np.ascontiguousarray(k))
    z = DeviceBuffer(2 * 4 * 4 * 40 * 4)
    l.xdet_memset(z.ptr, SENTINEL_BYTE, z.nbytes, None)
    synchronize()
    door = l.xdet_stem_conv3x3s2_train_forward
    for what, args, words in (('NULL image', (None, d_k.ptr, 2, 9, z.ptr, 32), 'NULL argument'),
                              ('NULL kernel', (d_x.ptr, None, 2, 9, z.ptr, 32), 'NULL argument'),
                              ('NULL output', (d_x.ptr, d_k.ptr, 2, 9, None, 32), 'NULL argument'),
                              ('S = 2', (d_x.ptr, d_k.ptr, 2, 2, z.ptr, 32), 'S of at least 3'),
                              ('N = 0', (d_x.ptr, d_k.ptr, 0, 9, z.ptr, 32), 'N positive'),
                              ('ld_z = 31', (d_x.ptr, d_k.ptr, 2, 9, z.ptr, 31), 'ld_z is below the 32 output channels'),
                              ('N * S * S = 2^31', (d_x.ptr, d_k.ptr, 1 << 15, 1 << 8, z.ptr, 32), 'below 2^31')):
        rc = door(*args, None)
        err = l.xdet_last_error().decode()
        assert rc == -1 and 'stem_conv3x3s2_train_forward' in err and words in err, (what, rc, err)
    synchronize()
    assert (to_host(z.ptr, (z.nbytes // 4,), np.uint32) == SENTINEL32).all()
    assert door(d_x.ptr, d_k.ptr, 2, 9, z.ptr, 40, None) == 0          # and the same arguments, in range, run
    synchronize()
    assert not (to_host(z.ptr, (2 * 4 * 4, 40), np.uint32)[:, :32] == SENTINEL32).all(axis=1).any()
