"""xdet_conv_backward_strided (csrc/conv_backward.hip) against the float64 statement
(ops.host_conv_backward_strided, pinned by tests/test_conv_strided_backward_math.py), with the metric and the bar of
tests/conv_strided_backward_cases.py: per output tensor max |got - ref| / max (|A| . |B|) <= max(4 x the f32 statement's
distance, 3 * 2^-22) = 7.2e-07 (the statement's distance is 1.2e-07, so the floor decides).
The largest distance measured on an MI355X over all cases of this file is 0.25 of that bar (dW of same_s2_odd; the corner-pixel
cases reach 0.23, dx of narrow_two_steps 0.18, db stays under 0.08)."""
import numpy as np
import pytest

import conv_backward_cases as CC
import conv_strided_backward_cases as CS

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-12345.5)
MODES = {'VALID': 0, 'SAME': 1}


@pytest.fixture(scope='module')
def bar():
    return CS.bar()


def run_raw(x, w, dy, y=None, relu_in=False, stride=1, padding='SAME', pad=(0, 0, 0, 0), with_dx=True, poison_ws=False):
    """The C door on padded device copies: pad = extra channels of (x, y, dy, dx), NaN in the inputs' padding and a sentinel
    in dx's.  -> (dx or None, dw, db, dx's padding or None)"""
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, synchronize
    N, H, W, C = x.shape
    kh, kw, _, J = w.shape
    mode = MODES[padding]

    def padded(a, extra, fill=np.nan):
        p = np.full(a.shape[:3] + (a.shape[3] + extra,), fill, f32)
        p[..., :a.shape[3]] = a
        return p
    d_x, d_w, d_dy = to_device(padded(x, pad[0])), to_device(np.ascontiguousarray(w, f32)), to_device(padded(dy, pad[2]))
    d_y = to_device(padded(y, pad[1])) if y is not None else None
    ld_dx = C + pad[3]
    d_dx = to_device(np.full((N, H, W, ld_dx), SENTINEL, f32)) if with_dx else None
    d_dw, d_db = to_device(np.full(w.shape, SENTINEL, f32)), to_device(np.full((max(J, 4),), SENTINEL, f32))
    nb = lib().xdet_conv_backward_strided_workspace_bytes(N, H, W, C, J, kh, kw, stride, mode)
    assert nb > 0
    ws = to_device(np.full((nb // 4,), np.nan, f32)) if poison_ws else DeviceBuffer(nb)
    check(lib().xdet_conv_backward_strided(d_x.ptr, C + pad[0], d_w.ptr, d_y.ptr if y is not None else None, J + pad[1], d_dy.ptr,
                                           J + pad[2], N, H, W, C, J, kh, kw, stride, mode, 1 if relu_in else 0,
                                           d_dx.ptr if with_dx else None, ld_dx, d_dw.ptr, d_db.ptr, ws.ptr, None))
    synchronize()
    dx = tail = None
    if with_dx:
        full = to_host(d_dx.ptr, (N, H, W, ld_dx), f32)
        dx, tail = np.ascontiguousarray(full[..., :C]), full[..., C:]
    return dx, to_host(d_dw.ptr, w.shape, f32), to_host(d_db.ptr, (J,), f32), tail


def judge(what, got, ref_den, bar):
    ref, den = ref_den
    d = CS.distances(got[:3], ref, den)
    print('%s: distance / bar = %s' % (what, ', '.join('%.4f' % (v / bar) for v in d)))
    assert max(d) <= bar, (what, [v / bar for v in d])


def bits(a):
    return np.asarray(a).view(np.uint32)


def same_bits(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


_dense = {}


def dense_run(name):
    """the dense-stride call through the C door, once per case"""
    if name not in _dense:
        _dense[name] = run_raw(*CS.make_case(name))
    return _dense[name]


@pytest.mark.parametrize('name', sorted(CS.CASES))
def test_shapes(name, bar):
    """every shape through the Python door (dense pixels), y with its exact zeros where the case has a ReLU; the C door
    gives the same bits"""
    from xdet.ops import conv_backward_strided
    x, w, dy, y, relu_in, stride, padding = CS.make_case(name)
    got = conv_backward_strided(x, w, dy, y, relu_in, stride=stride, padding=padding)
    assert got[0].shape == x.shape and got[1].shape == w.shape and got[2].shape == (w.shape[3],)
    judge(name, got, CS.case_reference(name), bar)
    assert same_bits(got, dense_run(name)[:3])


@pytest.mark.parametrize('name', sorted(CS.CASES))
def test_without_dx(name):
    """dx = NULL leaves dw and db as they are"""
    dense = dense_run(name)
    no_dx = run_raw(*CS.make_case(name), with_dx=False)
    assert no_dx[0] is None and same_bits(no_dx[1:3], dense[1:3])
    from xdet.ops import conv_backward_strided
    x, w, dy, y, relu_in, stride, padding = CS.make_case(name)
    door = conv_backward_strided(x, w, dy, y, relu_in, with_dx=False, stride=stride, padding=padding)
    assert door[0] is None and same_bits(door[1:], dense[1:3])


@pytest.mark.parametrize('name', sorted(CS.CASES))
def test_padded_strides(name, bar):
    """every ld wider than its width (ld_x = 4 for the 3-channel image) with NaN in the padding, a sentinel behind dx's
    width that survives: the same bits as the dense-stride call"""
    case = CS.make_case(name)
    C = case[0].shape[3]
    pad = (1, 7, 3, 1) if C == 3 else (14, 7, 3, 5)
    wide = run_raw(*case, pad=pad, poison_ws=True)
    judge(name + ' padded', wide, CS.case_reference(name), bar)
    assert wide[3].shape[3] == pad[3] and (wide[3] == SENTINEL).all()
    assert same_bits(wide[:3], dense_run(name)[:3])


def test_nan_under_no_window(bar):
    """stem1_even: NaN in the input row and column that no window covers -- dw is finite with the clean run's bits, dx there
    is exactly 0 (with and without the ReLU in front, whose mask would read x)"""
    x, w, dy, y, relu_in, stride, padding = CS.make_case('stem1_even')
    N, H, W, C = x.shape
    Hc, Wc = CS.geometry(H, W, 3, 3, stride, padding)[4:]
    assert (Hc, Wc) == (H - 1, W - 1)
    dirty = np.array(x)
    dirty[:, Hc:], dirty[:, :, Wc:] = np.nan, np.nan
    for ri in (relu_in, True):
        clean = dense_run('stem1_even') if ri == relu_in else run_raw(x, w, dy, y, ri, stride, padding)
        got = run_raw(dirty, w, dy, y, ri, stride, padding, pad=(1, 0, 0, 1))
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and same_bits(got[:3], clean[:3])
        for edge in (got[0][:, Hc:], got[0][:, :, Wc:]):
            assert np.array_equal(bits(edge), np.zeros(edge.shape, np.uint32))                   # +0, not -0
        assert got[0][:, :Hc, :Wc].any() and (got[3] == SENTINEL).all()
        judge('NaN under no window, relu_in %d' % ri, got, CS.reference64(dirty, w, dy, y, ri, stride, padding), bar)


@pytest.mark.parametrize('name', ['stem1_odd', 'same_s2_odd', 'stem2'])
def test_no_reach_across_the_image_border(name, bar):
    """one non-zero output pixel in the last corner of image 0: dx lives in that window of image 0, image 1 gets exact zeros
    and so do the wrapped-around columns (the first columns of the rows below, the first rows of image 1); the taps that
    would read x outside the image have dw exactly zero"""
    x, w, dy, y, relu_in, stride, padding = CS.make_case(name)
    N, H, W, C = x.shape
    kh, kw = w.shape[:2]
    Ho, Wo, pt, pl = CS.geometry(H, W, kh, kw, stride, padding)[:4]
    one = np.zeros_like(dy)
    j = int(np.argmax(y[0, Ho - 1, Wo - 1] > 0))
    assert y[0, Ho - 1, Wo - 1, j] > 0
    one[0, Ho - 1, Wo - 1, j] = dy[0, Ho - 1, Wo - 1, j]
    xpos = np.abs(x) + f32(0.5)                                  # relu_in: every x > 0, so the input mask hides nothing
    got = run_raw(xpos, w, one, y, relu_in, stride, padding)
    judge('corner pixel', got, CS.reference64(xpos, w, one, y, relu_in, stride, padding), bar)
    dx, dw = got[0], got[1]
    h0, w0 = (Ho - 1) * stride - pt, (Wo - 1) * stride - pl      # the window's first row and column
    inside = np.zeros((H, W), bool)
    inside[h0:h0 + kh, w0:w0 + kw] = True
    assert not dx[1].any() and not dx[0][~inside].any() and dx[0][inside].all()
    live = np.zeros((kh, kw), bool)
    live[:H - h0, :W - w0] = True                                # tap (a, b) read x at (h0 + a, w0 + b)
    assert not dw[~live].any() and all(dw[a, b].any() for a, b in zip(*np.nonzero(live)))
    # and the first corner of image 1, whose taps in front read the padding: nothing in image 0
    one = np.zeros_like(dy)
    j = int(np.argmax(y[1, 0, 0] > 0))
    one[1, 0, 0, j] = dy[1, 0, 0, j]
    got = run_raw(xpos, w, one, y, relu_in, stride, padding)
    inside = np.zeros((H, W), bool)
    inside[:kh - pt, :kw - pl] = True
    assert not got[0][0].any() and not got[0][1][~inside].any() and got[0][1][inside].all()
    live = np.zeros((kh, kw), bool)
    live[pt:, pl:] = True
    assert not got[1][~live].any() and all(got[1][a, b].any() for a, b in zip(*np.nonzero(live)))


@pytest.mark.parametrize('name', sorted(CS.SAME_S1_IS_OLD))
def test_same_s1_is_old(name):
    """stride 1 'SAME' has xdet_conv_backward's bits: that op is this one's stride-1 'SAME' door onto the same kernels"""
    from xdet.ops import conv_backward
    old = conv_backward(*CC.make_case(CS.SAME_S1_IS_OLD[name]))
    assert same_bits(dense_run(name)[:3], old)
    no_dx = conv_backward(*CC.make_case(CS.SAME_S1_IS_OLD[name]), with_dx=False)
    assert same_bits(run_raw(*CS.make_case(name), with_dx=False)[1:3], no_dx[1:])


@pytest.mark.parametrize('name', ['stem1_even', 'stem2', 'ranges', 'same_s2_odd'])
def test_two_calls_give_the_same_bits(name):
    """the second call over a NaN-filled workspace"""
    assert same_bits(dense_run(name)[:3], run_raw(*CS.make_case(name), poison_ws=True)[:3])


@pytest.mark.parametrize('name', ['stem1_odd', 'stem2', 'same_s2_odd'])
@pytest.mark.parametrize('k', [-7, 5])
def test_power_of_two_scaling_is_exact(name, k):
    """dy * 2^k gives 2^k times every output, bit for bit"""
    x, w, dy, y, relu_in, stride, padding = CS.make_case(name)
    s = f32(2.0 ** k)
    a, b = dense_run(name), run_raw(x, w, dy * s, y, relu_in, stride, padding)
    for u, v in zip(a[:3], b[:3]):
        assert u.any() and np.array_equal(bits(u * s), bits(v))


def test_abi_refusals():
    """the refusals of tests/test_conv_strided_backward_math.py with a device present, and through the Python door"""
    import xdet
    from xdet._lib import lib
    import test_conv_strided_backward_math as TM
    TM.test_c_door_refuses_before_any_gpu_work()
    p = 4096
    ok = dict(x=p, ld_x=3, w=p, y=None, ld_y=0, dy=p, ld_dy=32, N=1, H=9, W=9, C=3, J=32, kh=3, kw=3, stride=2, padding=0,
              relu_in=0, dx=None, ld_dx=0, dw=p, db=p, ws=p)
    for kw in (dict(stride=3), dict(padding=2), dict(H=2), dict(kh=4), dict(ws=None)):
        assert TM.c_call(lib(), ok, **kw) == -1, kw                     # XDET_ERR_INVALID_ARG
    assert lib().xdet_conv_backward_strided_workspace_bytes(1, 9, 9, 3, 32, 3, 3, 3, 0) == 0
    assert lib().xdet_conv_backward_strided_workspace_bytes(1, 2, 9, 3, 32, 3, 3, 2, 0) == 0
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.conv_backward_strided(np.zeros((1, 9, 9, 3), f32), np.zeros((3, 3, 3, 5), f32), np.zeros((1, 9, 9, 5), f32), stride=2)
