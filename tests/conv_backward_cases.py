"""Cases, the metric and the bar of the conv backward tests (tests/test_conv_backward_math.py on the CPU,
tests/test_gpu_conv_backward.py on the GPU), after the scheme of tests/dense_backward_cases.py.

Shapes (N, H, W, C, J, kh, kw, ReLU behind the conv, ReLU in front of it) are the smallest that reach every edge of
csrc/conv_backward.hip: a single pixel, where only the centre tap is live; every dimension ragged with J below one MFMA step;
the RPN conv's real channel counts (728 is no multiple of the tile or the step: a dW tile holds columns of two taps; dx
reduces over 9 * 512 = 4608); dW's row ranges (include/xdet.h) cut exactly between two images and inside an image row; the
one-axis kernels of the large-separable block with more taps than rows / columns; and 1 x 1, which is the dense layer.

Metric, per output tensor: max |got - ref| / max (|A| . |B|), the largest entry of the same product taken over the operands'
magnitudes (for db: the largest column sum of |g|).
Bar: max(4 x the f32 statement's distance from the float64 one over CASES, 3 * 2^-22).  The 4 is the margin the dense, loss
and spectral tests give the GPU; the floor is what the split representation can lose.  The f32 statement's distance is
recorded in tests/golden/conv_backward_f32_distance.npz (`python tests/test_conv_backward_math.py --write` rewrites it)."""
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_backward_f32_distance.npz')
FLOOR = 3 * 2.0 ** -22

# name: (N, H, W, C, J, kh, kw, relu_out, relu_in)
CASES = {
    'one_pixel': (1, 1, 1, 16, 16, 3, 3, False, False),
    'ragged_3x3': (2, 5, 7, 50, 25, 3, 3, True, True),
    'ragged_3x3_linear': (2, 5, 7, 50, 25, 3, 3, False, False),
    'rpn_widths': (1, 6, 6, 728, 512, 3, 3, True, True),
    'range_is_image': (2, 8, 16, 16, 16, 3, 3, True, False),
    'range_cuts_row': (3, 7, 7, 16, 16, 3, 3, True, True),
    'tall_15x1': (2, 9, 4, 40, 24, 15, 1, True, False),
    'wide_1x15': (2, 4, 9, 40, 24, 1, 15, False, True),
    'pointwise': (1, 5, 5, 64, 132, 1, 1, True, False),
}
# Beside the cases the recorded f32 distance is taken over: kh kw C = 27 <= 32 and J <= 32, the shape for which
# xdet_conv_backward_strided has a 32-row dW tile -- xdet_conv_backward keeps the 128-row tile's sums
MORE = {'narrow_shape': (2, 5, 7, 3, 20, 3, 3, True, True)}

_cache = {}


def conv_forward64(x, w, relu_in):
    """conv(xe, w), stride 1, 'SAME', in float64"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, H, W, C = x.shape
    kh, kw, _, J = w.shape
    xp = np.pad(np.maximum(x, 0) if relu_in else x, ((0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2), (0, 0)))
    out = np.zeros((N, H, W, J))
    for a in range(kh):
        for b in range(kw):
            out += xp[:, a:a + H, b:b + W] @ w[a, b]
    return out


def make_case(name):
    """-> x [N,H,W,C], w [kh,kw,C,J], dy [N,H,W,J] (gradient-sized: about 1e-4), y = relu(conv(xe, w) + b) with its exact
    zeros or None, relu_in"""
    if name not in _cache:
        N, H, W, C, J, kh, kw, relu_out, relu_in = CASES[name] if name in CASES else MORE[name]
        rng = np.random.default_rng(sum(name.encode()) * 13 + N * H * W)
        x = rng.standard_normal((N, H, W, C)).astype(f32)
        w = (rng.standard_normal((kh, kw, C, J)) / np.sqrt(kh * kw * C)).astype(f32)
        dy = (rng.standard_normal((N, H, W, J)) * 1e-4).astype(f32)
        y = None
        if relu_out:
            y = np.maximum(conv_forward64(x, w, relu_in) + rng.standard_normal(J), 0).astype(f32)
            assert (y == 0).any() and (y > 0).any()
        for a in (x, w, dy, y):
            if a is not None:
                a.setflags(write=False)
        _cache[name] = (x, w, dy, y, relu_in)
    return _cache[name]


def reference64(x, w, dy, y, relu_in):
    """the float64 statement and the three denominators of the metric: the same three sums over the operands' magnitudes"""
    from xdet.ops import host_conv_backward
    ref = host_conv_backward(x, w, dy, y, relu_in, dtype=np.float64)
    g = np.abs(np.asarray(dy, np.float64))
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.)
    ax = np.asarray(x, np.float64)
    ax = np.maximum(ax, 0) if relu_in else np.abs(ax)
    mag = host_conv_backward(ax, np.abs(np.asarray(w, np.float64)), g, None, False, dtype=np.float64)
    return ref, tuple(float(m.max()) for m in mag)


_refs = {}


def case_reference(name):
    if name not in _refs:
        _refs[name] = reference64(*make_case(name))
    return _refs[name]


def distances(got, ref, den):
    """per tensor (dx, dw, db); a None in got is skipped; an all-zero reference demands exact zeros"""
    out = []
    for g, r, d in zip(got, ref, den):
        if g is None:
            continue
        err = float(np.abs(np.asarray(g, np.float64) - r).max())
        out.append(err / d if d > 0 else (0. if err == 0 else np.inf))
    return out


def f32_statement_distance():
    """the largest distance of host_conv_backward in f32 from the float64 statement, over CASES"""
    from xdet.ops import host_conv_backward
    worst = 0.
    for name in CASES:
        ref, den = case_reference(name)
        worst = max([worst] + distances(host_conv_backward(*make_case(name)), ref, den))
    return worst


def bar():
    d = float(np.load(GOLDEN)['f32_distance'])
    return max(4 * d, FLOOR)
