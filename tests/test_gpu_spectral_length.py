"""ops.SpectralConv at the shortest alias-free transform length (spectral_points(F) = the smallest even L >= F + 7,
tests/test_spectral_length_math.py) and the grouped GEMM's balanced tile mapping (csrc/conv_mfma_dma.hip, tile_of: the live
tiles numbered group-major, XCD x taking the q = cdiv(live tiles, 8) of them from x * q on).

(a) The inputs wrap-around would hurt most -- x non-zero only in the outermost 7 lines at each end of the convolved axis, w
    only at taps 0 and 14 -- against the float64 direct convolution, workspace and output poisoned first, for F = 16, 30, 50
    and both axes.  Tolerance: tests/test_gpu_spectral.py's rule, max(3e-5, 4 x the distance of the float32 restatement from
    the float64 direct conv over the cases of this file), the restatement evaluated at the library's length.  One point
    of aliasing moves these outputs by O(1) (the CPU file measures 2.3 - 2.9 at F + 6).  The restatement's distance, measured
    on the CPU: 2.4e-07, so the bar is its 3e-5 floor; the largest distance measured on an MI355X is 0.0103 of that bar.
(b) workspace_bytes(N) is the layout [x_hi | x_lo | y] (each part + 512 bytes of slack, rounded up to 256 bytes) of
    NB = spectral_points(F) / 2 bins of m_pad rows.
(c) F = 30, 64 -> 256 channels, the bins' GEMM [19 x m_pad, 128] x [128, 512]:
      115 images: m_pad 3,584 = 14 M tiles, 19 x 14 x 2 = 532 live tiles -> the 256 x 256 tile, 8 x 67 = 536 virtual blocks on
                  one workgroup per compute unit: the walk over the balanced mapping, XCD 7 with 63 tiles and 4 empty slots,
                  groups cut at every XCD boundary (28 tiles per group, 67 per XCD);
       98 images: m_pad 3,072, 19 x 12 x 2 = 456 tiles are not a grid the launch rule gives the 256 x 256 tile (it wants >= 512,
                  whole rounds of 256, or >= 200 with >= 40 K steps), so the layer runs 128 x 128 tiles through the same
                  tile_of, one tile per workgroup: 19 x 23 x 4 = 1,748 live tiles (the 24th M tile of every group is padding
                  only and not enumerated), 219 per XCD, groups of 92 straddling XCDs.
    `launch_form` restates the launcher's rule for 19 groups and both facts are asserted.  The rows of three image pairs
    (first, middle, last) must equal, bit for bit, the same pairs run as a batch of two (m_pad 128: the deep ring's 64 x 64
    tiles, a kernel this mapping does not touch).
    Not covered: a 256-row tile of padding only needs group_live_rows + 256 <= group_rows, which SpectralConv::m_pad never
    produces for the 256 x 256 tile and no xdet.ops entry can ask for directly (the 128 x 128 case above has one per group)."""
import numpy as np
import pytest

from test_spectral_length_math import border_case, direct, points, restate

pytestmark = pytest.mark.gpu
f32 = np.float32
MAX_CUS = 304

BORDER_CASES = [(F, axis) for F in (16, 30, 50) for axis in (0, 1)]
N_B, CIN_B, COUT_B = 2, 40, 70                                      # ld 64: waves 2, 3 of dft_fwd return early; cout -> 96


def _cdiv(a, b):
    return -(-a // b)


def m_pad_rows(F, N):
    return 128 if N * F <= 128 else _cdiv(N * F, 256) * 256


def distance(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.fixture(scope='module')
def refs(oracle):
    """(F, axis) -> (x, w, float64 reference), computed once; 'bar' -> the tolerance"""
    out, worst = {}, 0.
    for F, axis in BORDER_CASES:
        x, w = border_case(np.random.default_rng(1000 + 10 * F + axis), N_B, F, axis, CIN_B, COUT_B)
        ref = direct(oracle, x, w, axis, np.float64)
        d = distance(restate(x, w, axis, points(F)), ref)
        print('F %d axis %d: f32 restatement at L = %d vs float64 direct conv: %.3e' % (F, axis, points(F), d))
        worst = max(worst, d)
        out[F, axis] = (x, w, ref)
    assert worst > 0
    out['bar'] = max(3e-5, 4 * worst)
    print('f32 restatement vs float64: %.3e -> bar %.3e' % (worst, out['bar']))
    return out


def make_layer(w, axis, F, scale=None, shift=None):
    from xdet import ops
    from xdet.runtime import set_precision
    set_precision('f16x3')
    try:
        return ops.SpectralConv(w, axis, F, scale, shift, relu=scale is not None)
    finally:
        set_precision('f32')


def run_poisoned(layer, x):
    """forward with every byte of the workspace (the bins' padding rows among them) and of the output poisoned first"""
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, DeviceTensor, synchronize
    N, F = x.shape[0], x.shape[1]
    ws = DeviceBuffer(layer.workspace_bytes(N))
    check(lib().xdet_memset(ws.ptr, 0xA5, ws.nbytes, None))
    out = DeviceTensor.empty((N, F, F, layer.cout))
    check(lib().xdet_memset(out.ptr, 0xA5, N * F * F * out.ld * 4, None))
    synchronize()
    layer(DeviceTensor.from_numpy(x), out=out, workspace=ws)
    return out.numpy()


@pytest.mark.parametrize('F,axis', BORDER_CASES)
def test_border_inputs_match_float64_direct_conv(F, axis, refs):
    x, w, ref = refs[F, axis]
    assert m_pad_rows(F, N_B) > N_B * F                             # padding rows, poisoned
    got = run_poisoned(make_layer(w, axis, F), x)
    assert np.isfinite(got).all()
    d = distance(got[..., :COUT_B], ref)
    print('F %d axis %d: distance / bar = %.4f (bar %.3e)' % (F, axis, d / refs['bar'], refs['bar']))
    assert d <= refs['bar'], (F, axis, d / refs['bar'])


@pytest.mark.parametrize('F', [16, 30, 50])
def test_workspace_is_the_layout_at_the_new_bin_count(F):
    cin, cout = 40, 70
    layer = make_layer(np.zeros((15, cin, cout), f32), 0, F)
    cin_ld, cout_ld, NB = _cdiv(cin, 32) * 32, _cdiv(cout, 32) * 32, points(F) // 2
    for N in (1, 2, 5, 9, 35):
        rows = NB * m_pad_rows(F, N)
        planes = _cdiv((rows * 2 * cin_ld + 256) * 2, 256) * 256    # x_hi, x_lo: f16, 512 bytes of slack
        y = _cdiv((rows * 2 * cout_ld + 128) * 4, 256) * 256        # the bins' products: f32, 512 bytes of slack
        assert layer.workspace_bytes(N) == 2 * planes + y, (F, N)


def launch_form(groups, group_rows, live_rows, cout, kp):
    """the rule of launch_conv_mfma_dma / launch_d for a grouped f16x3 GEMM of `groups` x group_rows rows:
    -> (M tile, virtual blocks) for the two-stage kernel's 256 x 256 or 128 x 128 tile, (0, 0) for the deep ring's forms"""
    cout_pad = _cdiv(cout, 128) * 128
    M = groups * group_rows
    b256, nk = _cdiv(M, 256) * (cout_pad // 256), kp // 32
    full_rounds = b256 >= 240 and (b256 % 256 == 0 or b256 % 256 >= 240)
    if cout_pad % 256 == 0 and group_rows % 256 == 0 and (b256 >= 512 or full_rounds or (b256 >= 200 and nk >= 40)):
        return 256, _cdiv(groups * _cdiv(live_rows, 256) * (cout_pad // 256), 8) * 8
    if (group_rows % 64 == 0 and live_rows <= 64 and groups * (cout_pad // 64) <= 768) or \
            _cdiv(M, 128) * (cout_pad // 128) <= 128:
        return 0, 0
    return 128, _cdiv(groups * _cdiv(live_rows, 128) * (cout_pad // 128), 8) * 8


@pytest.mark.parametrize('n_img,tile,nvb', [(115, 256, 536), (98, 128, 1752)])
def test_balanced_grouped_tiles_give_every_image_the_bits_of_a_batch_of_two(n_img, tile, nvb):
    from xdet.runtime import DeviceTensor
    F, cin, cout, T = 30, 64, 256, 15
    NB = points(F) // 2
    assert NB == 19
    m_pad = m_pad_rows(F, n_img)
    assert launch_form(NB, m_pad, n_img * F, 2 * cout, 2 * cin) == (tile, nvb)
    assert (nvb > MAX_CUS and tile == 256) == (n_img == 115)       # 115 images walk; 98 run one 128 x 128 tile per workgroup
    assert (nvb // 8) % (_cdiv(n_img * F, tile) * (2 * cout // tile)) != 0   # XCD shares are no whole groups: groups straddle
    assert launch_form(NB, 128, 2 * F, 2 * cout, 2 * cin) == (0, 0)         # the batches of two: the deep ring
    rng = np.random.default_rng(31)
    x = rng.standard_normal((n_img, F, F, cin)).astype(f32)
    w = (rng.standard_normal((T, cin, cout)) / np.sqrt(T * cin)).astype(f32)
    sc = rng.uniform(0.5, 1.5, cout).astype(f32)
    sh = rng.standard_normal(cout).astype(f32)
    layer = make_layer(w, 0, F, sc, sh)
    big = layer(DeviceTensor.from_numpy(x)).numpy()
    for n0 in (0, n_img // 2 - 1, n_img - 2):
        small = layer(DeviceTensor.from_numpy(x[n0:n0 + 2])).numpy()
        assert np.array_equal(small.view(np.uint32), big[n0:n0 + 2].view(np.uint32)), n0
