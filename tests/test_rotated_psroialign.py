"""RotatedPsRoiAlign without a GPU: the NumPy restatement (tests/rotated_psroi_ref.py) against the fixture the
reference's own CPU functors produced (tests/golden/make_rotated_psroi_golden.py), the restatement's gradient as the
adjoint of its forward, the C-ABI symbols, and the argument errors of the Python API."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rotated_psroi_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rotated_psroi_golden.npz')
CASES = ('kat', 'g7', 'g32')
SYMBOLS = ('xdet_rotated_psroialign_fwd', 'xdet_rotated_psroialign_grad')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope='module')
def built():
    from xdet import build
    return build.build()


@pytest.mark.parametrize('method', ['mean', 'max'])
@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference_functors(golden, case, method):
    z = golden
    gw, gh = (int(v) for v in z[case + '_grid'])
    p, i = RR.forward(z[case + '_inputs'], z[case + '_rois'], z[case + '_orders'], gw, gh, method)
    gp, gi = z['%s_%s_pooled' % (case, method)], z['%s_%s_index' % (case, method)]
    assert p.shape == gp.shape and i.dtype == np.int32
    assert np.array_equal(p.view(np.int32), gp.view(np.int32))          # bit for bit
    assert np.array_equal(i, gi)
    g = RR.gradient(z[case + '_inputs'].shape, z[case + '_rois'], z[case + '_orders'], z[case + '_grad'], gi, gw, gh,
                    method)
    gg = z['%s_%s_grad_inputs' % (case, method)]
    assert np.abs(g - gg).max() <= 1e-5


def test_fixture_covers_what_it_claims(golden):
    z = golden
    orders = np.concatenate([z[c + '_orders'].ravel() for c in CASES])
    assert set(orders.tolist()) == {-1, 0, 1, 2, 3}
    for c in CASES:
        H, W = z[c + '_inputs'].shape[2:]
        gw, gh = (int(v) for v in z[c + '_grid'])
        assert not RR.out_of_bounds(z[c + '_rois'], z[c + '_orders'], H, W, gw, gh).any()
    y, x, deg = RR.vertices(z['g7_rois'].reshape(-1, 8), z['g7_orders'].ravel(), 9, 11)
    assert deg.any() and not deg.all()
    assert (z['g32_max_index'] > 0).any()                              # bins with several samples
    assert os.path.getsize(GOLDEN) <= 256 * 1024


def test_known_answers(golden):
    """the reference's CPU functor on test_op.py:133-141 (as the issue quotes them)"""
    z = golden
    mean = [[8.5625, 12.4375, 6.4375, 9.5625], [18.4375, 20.5625, 21.5625, 24.4375], [18.875, 23.875, 13.375, 19.875]]
    for r in range(3):
        for b in range(4):
            assert np.all(z['kat_mean_pooled'][0, r, b] == np.float32(mean[r][b]))
    assert np.all(z['kat_mean_index'] == 0)
    assert np.array_equal(z['kat_max_pooled'][0, :2], z['kat_mean_pooled'][0, :2])
    assert np.allclose(z['kat_max_pooled'][0, 2, :, 0], [19.604166, 23.875, 14.25, 20.020834], rtol=0, atol=1e-5)
    assert z['kat_max_index'][0, :, :, 0].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1]]
    for m in ('mean', 'max'):
        assert abs(float(z['kat_%s_grad_inputs' % m].astype(np.float64).sum()) - 48.) < 1e-4


def _random_case(seed, N=2, C=12, H=9, W=11, R=16):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    rois = rng.uniform(-0.2, 1.2, (N, R, 8)).astype(np.float32)          # in and out of bounds: the clamping rule
    orders = rng.integers(-1, 6, (N, R)).astype(np.int32)
    return rng, x, rois, orders


@pytest.mark.parametrize('grid', [(3, 2), (2, 3), (1, 1)])
def test_mean_gradient_is_the_adjoint_of_the_forward(grid):
    gw, gh = grid
    rng, x, rois, orders = _random_case(11 + gw)
    p, _ = RR.forward(x, rois, orders, gw, gh, 'mean')
    g = rng.uniform(-1, 1, p.shape).astype(np.float32)
    gx = RR.gradient(x.shape, rois, orders, g, np.zeros(p.shape, np.int32), gw, gh, 'mean')
    lhs = float(np.dot(gx.astype(np.float64).ravel(), x.astype(np.float64).ravel()))
    rhs = float(np.dot(g.astype(np.float64).ravel(), p.astype(np.float64).ravel()))
    scale = float(np.dot(np.abs(gx).astype(np.float64).ravel(), np.abs(x).astype(np.float64).ravel())) + 1.
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_max_gradient_is_the_adjoint_with_the_index_held():
    rng, x, rois, orders = _random_case(5)
    p, idx = RR.forward(x, rois, orders, 3, 2, 'max')
    g = rng.uniform(-1, 1, p.shape).astype(np.float32)
    gx = RR.gradient(x.shape, rois, orders, g, idx, 3, 2, 'max')
    # the forward is linear in x for a fixed argmax: <grad(g), y> = <g, pooled(y) at the held sample>
    y = rng.standard_normal(x.shape).astype(np.float32)
    py = _pooled_at(y, rois, orders, 3, 2, idx)
    lhs = float(np.dot(gx.astype(np.float64).ravel(), y.astype(np.float64).ravel()))
    rhs = float(np.dot(g.astype(np.float64).ravel(), py.ravel()))
    assert abs(lhs - rhs) <= 1e-5 * (np.abs(g).sum() * np.abs(y).max() + 1.)
    # and on x itself the held sample is the forward's value
    assert np.allclose(_pooled_at(x, rois, orders, 3, 2, idx), p, rtol=1e-6, atol=1e-6)


def _pooled_at(x, rois, orders, gw, gh, idx):
    """value of the sample `idx` names, per output element (float64), via the restatement's geometry"""
    N, C, H, W = x.shape
    R = rois.shape[1]
    G = gw * gh
    bank = C // G
    y_, x_, deg = RR.vertices(rois.reshape(-1, 8), orders.ravel(), H, W)
    geo = RR.bin_geometry(y_, x_, gw, gh, H + W)
    out = np.zeros((N * R, G, bank))
    for m in range(N * R):
        if deg[m]:
            continue
        for b in range(G):
            fl = {k: v[m:m + 1, b:b + 1] for k, v in geo.items()}
            for ch in range(bank):
                k = int(idx.reshape(N * R, G, bank)[m, b, ch])
                nw = int(fl['nw'][0, 0])
                ys = RR.sample_coord(fl['lty'], fl['rty'], fl['gysl'], fl['gysr'], k // nw)
                xs = RR.sample_coord(fl['ltx'], fl['lbx'], fl['gxst'], fl['gxsb'], k % nw)
                y0, y1, fy, _ = RR.cell(ys, H)
                x0, x1, fx, _ = RR.cell(xs, W)
                fy, fx = float(fy[0, 0]), float(fx[0, 0])
                img = x[m // R, b * bank + ch].astype(np.float64)
                y0, y1, x0, x1 = int(y0[0, 0]), int(y1[0, 0]), int(x0[0, 0]), int(x1[0, 0])
                out[m, b, ch] = ((1 - fx) * (1 - fy) * img[y0, x0] + (1 - fx) * fy * img[y1, x0]
                                 + fx * (1 - fy) * img[y0, x1] + fx * fy * img[y1, x1])
    return out.reshape(N, R, G, bank)


def test_symbols_declared_exported_and_in_the_ctypes_table(built):
    from xdet import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'xdet.h')).read(), flags=re.S)
    out = subprocess.check_output(['nm', '-D', '--defined-only', built]).decode()
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, hdr), s
        assert re.search(r'\sT\s+%s\b' % s, out), s
        assert s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['xdet_rotated_psroialign_fwd'][1]) == 16
    assert len(_lib.SIGNATURES['xdet_rotated_psroialign_grad'][1]) == 16
    blob = open(built, 'rb').read()
    assert b'rotated_psroialign_fwd_kernel' in blob and b'rotated_psroialign_grad_kernel' in blob


def _bad_calls():
    feat = np.zeros((1, 8, 4, 4), np.float32)
    rois = np.zeros((1, 2, 8), np.float32)
    orders = np.zeros((1, 2), np.int32)
    g = np.zeros((1, 2, 4, 2), np.float32)
    gi = np.zeros((1, 2, 4, 2), np.int32)
    fwd = [
        (feat[0], rois, orders, 2, 2, 'max'),                              # rank-4 inputs
        (feat, np.zeros((1, 2, 4), np.float32), orders, 2, 2, 'max'),      # rois [N,R,8]
        (feat, rois[0], orders, 2, 2, 'max'),
        (feat, rois, orders[0], 2, 2, 'max'),                              # orders [N,R]
        (feat, np.zeros((2, 2, 8), np.float32), np.zeros((2, 2), np.int32), 2, 2, 'max'),   # batch match
        (feat, rois, np.zeros((1, 3), np.int32), 2, 2, 'max'),             # ROI-count match
        (feat, rois, np.zeros((2, 2), np.int32), 2, 2, 'max'),
        (feat, rois, orders, -1, 2, 'max'),                                # grid >= 0
        (feat, rois, orders, 2, -2, 'max'),
        (feat, rois, orders, 2, 2, 'median'),                              # mean / max
        (feat, rois, orders, 0, 2, 'max'),                                 # zero grid (reference: division by zero)
        (feat, rois, orders, 3, 1, 'max'),                                 # C % (gh*gw)
    ]
    grad = [(a[0], a[1], a[2], g, gi) + a[3:] for a in fwd]
    grad += [
        (feat, rois, orders, g, gi[..., :1], 2, 2, 'max'),                 # grad and index shapes differ
        (feat, rois, orders, g[..., :1], gi[..., :1], 2, 2, 'max'),        # not [N,R,gs,bank]
    ]
    return fwd, grad


def test_argument_errors_are_raised_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import ops

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    monkeypatch.setattr(ops, 'to_device', no_gpu)
    monkeypatch.setattr(ops, 'lib', no_gpu)
    fwd, grad = _bad_calls()
    for args in fwd:
        with pytest.raises(xdet.InvalidArgumentError):
            xdet.rotated_ps_roi_align(*args)
    for args in grad:
        with pytest.raises(xdet.InvalidArgumentError):
            xdet.rotated_ps_roi_align_grad(*args)


def test_c_abi_rejects_bad_arguments_before_any_gpu_work(built):
    """XDET_ERR_INVALID_ARG with no device pointer touched (host pointers would fault a launch)"""
    from xdet import _lib
    L = _lib.lib()
    a = np.zeros(64, np.float32)
    p = ctypes.c_void_p(a.ctypes.data)
    for gw, gh, C, layout, ldc in ((0, 2, 8, 0, 8), (2, -1, 8, 0, 8), (3, 1, 8, 0, 8), (2, 2, 8, 2, 8), (2, 2, 8, 1, 4)):
        assert L.xdet_rotated_psroialign_fwd(p, p, p, p, p, 1, C, 4, 4, 2, gw, gh, 1, layout, ldc, None) == -1
        assert L.xdet_rotated_psroialign_grad(p, p, p, p, p, 1, C, 4, 4, 2, gw, gh, 1, layout, ldc, None) == -1
    assert L.xdet_rotated_psroialign_fwd(None, p, p, p, None, 1, 8, 4, 4, 2, 2, 2, 1, 0, 8, None) == -1
    assert L.xdet_rotated_psroialign_grad(p, p, p, None, p, 1, 8, 4, 4, 2, 2, 2, 1, 0, 8, None) == -1   # 'max' needs the index


def test_no_cpu_fallback_without_a_gpu(built):
    """On a box without a GPU the op fails loudly (HIP error), never computes on the host."""
    from xdet import _lib
    n = ctypes.c_int(0)
    rc = _lib.lib().xdet_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip('a GPU is present')
    import xdet
    feat = np.zeros((1, 4, 2, 2), np.float32)
    rois = np.zeros((1, 1, 8), np.float32)
    orders = np.zeros((1, 1), np.int32)
    with pytest.raises(xdet.XdetError):
        xdet.rotated_ps_roi_align(feat, rois, orders, 2, 2, 'max')
    with pytest.raises(xdet.XdetError):
        xdet.rotated_ps_roi_align_grad(feat, rois, orders, np.zeros((1, 1, 4, 1), np.float32),
                                       np.zeros((1, 1, 4, 1), np.int32), 2, 2, 'max')
