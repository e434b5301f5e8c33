"""Cases, the metric and the bar of the depthwise-backward tests (tests/test_depthwise_backward_math.py on the CPU,
tests/test_gpu_depthwise_backward.py and tests/test_gpu_exit_flow_backward.py on the GPU), after the scheme of
tests/batch_norm_cases.py.

Shapes (N, H, W, C, dilation, ReLU in front of the conv) are the smallest that reach every edge of
csrc/depthwise_backward.hip: one pixel, where only the centre tap exists; an image smaller than the reach of dilation 2, where
every off-centre tap of some pixel is absent; a channel count that is no multiple of the four a lane owns; dilation 2; one
channel; the channel limit; an exit-flow width (six channel blocks); a pixel count past the floor of the chunk rule
max(64, ceil(M / 1024)) (include/xdet.h) -- M = 260 * 260 = 67,600 > 65,536 gives chunks of 67 pixels, so the issue's shape
stands as it is; and two images with dy alive only in the first and x only in the second, where any term that crosses an
image boundary shows as a nonzero.

Inputs: x ~ N(0, 1) (about half of it masked under relu_in), dy ~ 1e-4 N(0, 1), k ~ N(0, 1) / 3 with no symmetry between taps.
dx: no tolerance -- np.array_equal with the f32 host statement (ops.host_depthwise_backward adds the taps in the op's order;
array_equal does not tell -0 from +0, which is not part of the contract).
dw metric, per tensor: max |got - ref64| / max over entries of sum |xe| |g| (an all-zero denominator demands exact zeros).
dw bar: max(4 x the f32 host statement's distance from the float64 one over CASES, 3 * 2^-22); the statement's dw is numpy's
sequential f32 sum.  The distance is recorded in tests/golden/depthwise_backward_f32_distance.npz
(`python tests/test_depthwise_backward_math.py --write` rewrites it)."""
import os

import numpy as np

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'depthwise_backward_f32_distance.npz')
FLOOR = 3 * 2.0 ** -22

# name: (N, H, W, C, dilation, relu_in)
CASES = {
    'one_pixel': (1, 1, 1, 4, 1, False),
    'smaller_than_reach': (1, 2, 3, 5, 2, True),
    'ragged': (2, 5, 7, 50, 1, True),
    'dilated': (2, 6, 5, 36, 2, True),
    'one_channel': (1, 4, 4, 1, 1, True),
    'widest': (1, 2, 2, 4096, 1, False),
    'exit_width': (1, 4, 4, 1536, 2, False),
    'chunk_growth': (1, 260, 260, 4, 1, False),
    'two_images': (2, 3, 3, 8, 1, False),
}

_cache, _refs = {}, {}


def make_case(name):
    """-> dict: x, dy [N,H,W,C], k [3,3,C,1], dilation, relu_in"""
    if name not in _cache:
        N, H, W, C, d, relu_in = CASES[name]
        rng = np.random.default_rng(sum(name.encode()) * 19 + N * H * W)
        x = rng.standard_normal((N, H, W, C)).astype(f32)
        dy = (rng.standard_normal((N, H, W, C)) * 1e-4).astype(f32)
        k = (rng.standard_normal((3, 3, C, 1)) / 3).astype(f32)
        if name == 'two_images':
            dy[1] = 0
            x[0] = 0
        for a in (x, dy, k):
            a.setflags(write=False)
        _cache[name] = dict(x=x, dy=dy, k=k, dilation=d, relu_in=relu_in)
    return _cache[name]


def reference64(x, k, dy, dilation, relu_in):
    """the float64 statement (dx, dw) and the metric's denominator: the largest entry of the dw sum over magnitudes"""
    from xdet.ops import host_depthwise_backward
    ref = host_depthwise_backward(x, k, dy, dilation, relu_in, dtype=f64)
    ax = np.asarray(x, f64)
    ax = np.maximum(ax, 0) if relu_in else np.abs(ax)
    mag = host_depthwise_backward(ax, k, np.abs(np.asarray(dy, f64)), dilation, False, dtype=f64, with_dx=False)[1]
    return ref, float(mag.max())


def case_reference(name):
    if name not in _refs:
        c = make_case(name)
        _refs[name] = reference64(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'])
    return _refs[name]


def dw_distance(got_dw, ref_dw, den):
    err = float(np.abs(np.asarray(got_dw, f64) - ref_dw).max())
    return err / den if den > 0 else (0. if err == 0 else np.inf)


def f32_statement_distance():
    """the largest distance of host_depthwise_backward's dw in f32 from the float64 statement's, over CASES"""
    from xdet.ops import host_depthwise_backward
    worst = 0.
    for name in CASES:
        c = make_case(name)
        (_, ref_dw), den = case_reference(name)
        got = host_depthwise_backward(c['x'], c['k'], c['dy'], c['dilation'], c['relu_in'], with_dx=False)[1]
        worst = max(worst, dw_distance(got, ref_dw, den))
    return worst


def bar():
    d = float(np.load(GOLDEN)['f32_distance'])
    return max(4 * d, FLOOR)
