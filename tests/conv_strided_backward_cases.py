"""Cases, the metric and the bar of the strided conv backward tests (tests/test_conv_strided_backward_math.py on the CPU,
tests/test_gpu_conv_strided_backward.py and tests/test_gpu_stem_chain.py on the GPU), after the scheme of
tests/conv_backward_cases.py.

Shapes (N, H, W, C, J, kh, kw, stride, padding, ReLU behind the conv, ReLU in front of it) are the smallest that reach every
edge of csrc/conv_backward.hip's general geometry: a single output pixel with all nine taps live; the stem's first conv (3 channels, stride
2, 'VALID') on a map every row of which lies under a window, and on one whose last row and column lie under none; the stem's
second conv, whose 288 dW rows straddle tiles and taps; 'SAME' at stride 2 with the padding 1/1 and 0/1; 1 x 1 at stride 2, which
is host_subsample2 in front of the dense layer; 7 x 7; the 32-row dW tile ragged and with two steps per range; dW's ranges
over the OUTPUT pixels (include/xdet.h) cut inside an output row and exactly between two images; and stride 1 'SAME' on two
cases of tests/conv_backward_cases.py, where the op must be xdet_conv_backward.

Metric, per output tensor: max |got - ref| / max (|A| . |B|), the largest entry of the same product taken over the operands'
magnitudes (for db: the largest column sum of |g|).
Bar: max(4 x the f32 statement's distance from the float64 one over CASES, 3 * 2^-22), as tests/conv_backward_cases.py.  The
f32 statement's distance is recorded in tests/golden/conv_strided_backward_f32_distance.npz
(`python tests/test_conv_strided_backward_math.py --write` rewrites it), next to the f32 host chain's distance that
tests/test_gpu_stem_chain.py reads its bar from."""
import os

import numpy as np

import conv_backward_cases as CC

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_strided_backward_f32_distance.npz')
FLOOR = 3 * 2.0 ** -22
V, S = 'VALID', 'SAME'

# name: (N, H, W, C, J, kh, kw, stride, padding, relu_out, relu_in)
CASES = {
    'one_window': (1, 3, 3, 3, 32, 3, 3, 2, V, False, False),
    'stem1_odd': (2, 9, 11, 3, 32, 3, 3, 2, V, True, False),
    'stem1_even': (1, 10, 8, 3, 32, 3, 3, 2, V, True, False),
    'stem2': (2, 7, 6, 32, 64, 3, 3, 1, V, True, False),
    'same_s2_odd': (2, 7, 9, 20, 25, 3, 3, 2, S, True, True),
    'same_s2_even': (1, 8, 6, 16, 16, 3, 3, 2, S, False, True),
    'pointwise_s2': (2, 5, 5, 24, 40, 1, 1, 2, S, False, False),
    'k7_s2': (1, 13, 13, 3, 16, 7, 7, 2, V, True, False),
    # Mo = 5 * 8 * 12 = 480 output pixels, one dW tile: four ranges of 128 (checked below); the cuts at 128 and 256 fall inside
    # an output row (96 pixels per image, 12 per row), the cut at 384 between images 3 and 4; H = 18 leaves its last row uncovered
    'ranges': (5, 18, 25, 8, 16, 3, 3, 2, V, True, False),
    # the 32-row dW tile (kh kw C <= 32 and J <= 32) beyond the stem's own shape: ragged in both, and the smallest map whose
    # ranges hold two of its 128-pixel steps (Mo = 259 * 259 = 67081 > 512 * 128: 263 ranges of 256 pixels, the last of 9)
    'narrow_ragged': (2, 7, 8, 2, 20, 3, 3, 2, V, True, True),
    'narrow_two_steps': (1, 520, 519, 1, 8, 3, 3, 2, V, True, False),
}
# stride 1 'SAME': these cases of tests/conv_backward_cases.py, with its data
SAME_S1_IS_OLD = {'same_s1_ragged_3x3': 'ragged_3x3', 'same_s1_pointwise': 'pointwise'}
for _new, _old in SAME_S1_IS_OLD.items():
    CASES[_new] = CC.CASES[_old][:7] + (1, S) + CC.CASES[_old][7:]


def geometry(H, W, kh, kw, stride, padding):
    """-> (Ho, Wo, pt, pl, Hc, Wc): the output map, the padding in front ('SAME': TensorFlow's, the smaller half), and the
    input rows / columns that lie under a window"""
    def axis(n, k):
        if padding == V:
            o, front = (n - k) // stride + 1, 0
        else:
            o = -(-n // stride)
            front = max((o - 1) * stride + k - n, 0) // 2
        return o, front, min(n, (o - 1) * stride + k - front)
    (Ho, pt, Hc), (Wo, pl, Wc) = axis(H, kh), axis(W, kw)
    return Ho, Wo, pt, pl, Hc, Wc


def dw_ranges(Mo, k_rows, J):
    """include/xdet.h's rule -> (output pixels per range, ranges)"""
    tiles = -(-k_rows // 128) * -(-J // (32 if J <= 32 else 128))
    want = max(1, 512 // tiles)
    per = -(-(-(-Mo // want)) // 128) * 128
    return per, -(-Mo // per)


def _check_ranges_case():
    N, H, W, C, J, kh, kw, s, pad = CASES['ranges'][:9]
    Ho, Wo = geometry(H, W, kh, kw, s, pad)[:2]
    per, n = dw_ranges(N * Ho * Wo, kh * kw * C, J)
    cuts = [per * i for i in range(1, n)]
    assert n >= 3 and any(c % (Ho * Wo) == 0 for c in cuts) and any(c % Wo != 0 for c in cuts), (per, n, Ho, Wo)


_check_ranges_case()
assert dw_ranges(259 * 259, 9, 8) == (256, 263)

_cache = {}


def conv_forward64(x, w, relu_in, stride, padding):
    """conv(xe, w) in float64, one product per tap"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, H, W, C = x.shape
    kh, kw, _, J = w.shape
    Ho, Wo, pt, pl = geometry(H, W, kh, kw, stride, padding)[:4]
    hs, ws = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1
    xp = np.pad(np.maximum(x, 0) if relu_in else x,
                ((0, 0), (pt, max(hs - 1 + kh - H - pt, 0)), (pl, max(ws - 1 + kw - W - pl, 0)), (0, 0)))
    out = np.zeros((N, Ho, Wo, J))
    for a in range(kh):
        for b in range(kw):
            out += xp[:, a:a + hs:stride, b:b + ws:stride] @ w[a, b]
    return out


def make_case(name):
    """-> x [N,H,W,C], w [kh,kw,C,J], dy [N,Ho,Wo,J] (gradient-sized: about 1e-4), y = relu(conv(xe, w) + b) with its exact
    zeros or None, relu_in, stride, padding"""
    if name not in _cache:
        N, H, W, C, J, kh, kw, stride, padding, relu_out, relu_in = CASES[name]
        if name in SAME_S1_IS_OLD:
            _cache[name] = CC.make_case(SAME_S1_IS_OLD[name]) + (stride, padding)
            return _cache[name]
        Ho, Wo = geometry(H, W, kh, kw, stride, padding)[:2]
        rng = np.random.default_rng(sum(name.encode()) * 13 + N * H * W)
        x = rng.standard_normal((N, H, W, C)).astype(f32)
        w = (rng.standard_normal((kh, kw, C, J)) / np.sqrt(kh * kw * C)).astype(f32)
        dy = (rng.standard_normal((N, Ho, Wo, J)) * 1e-4).astype(f32)
        y = None
        if relu_out:
            y = np.maximum(conv_forward64(x, w, relu_in, stride, padding) + rng.standard_normal(J), 0).astype(f32)
            assert (y == 0).any() and (y > 0).any()
        for a in (x, w, dy, y):
            if a is not None:
                a.setflags(write=False)
        _cache[name] = (x, w, dy, y, relu_in, stride, padding)
    return _cache[name]


def reference64(x, w, dy, y, relu_in, stride, padding):
    """the float64 statement and the three denominators of the metric: the same three sums over the operands' magnitudes"""
    from xdet.ops import host_conv_backward_strided as host
    ref = host(x, w, dy, y, relu_in, dtype=np.float64, stride=stride, padding=padding)
    g = np.abs(np.asarray(dy, np.float64))
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.)
    ax = np.asarray(x, np.float64)
    with np.errstate(invalid='ignore'):
        ax = np.nan_to_num(np.where(ax > 0, ax, 0.) if relu_in else np.abs(ax), nan=0.)   # a pixel under no window may hold NaN
    mag = host(ax, np.abs(np.asarray(w, np.float64)), g, None, False, dtype=np.float64, stride=stride, padding=padding)
    return ref, tuple(float(m.max()) for m in mag)


_refs = {}


def case_reference(name):
    if name not in _refs:
        _refs[name] = reference64(*make_case(name))
    return _refs[name]


distances = CC.distances


def f32_statement_distance():
    """the largest distance of host_conv_backward_strided in f32 from the float64 statement, over CASES"""
    from xdet.ops import host_conv_backward_strided as host
    worst = 0.
    for name in CASES:
        x, w, dy, y, relu_in, stride, padding = make_case(name)
        ref, den = case_reference(name)
        worst = max([worst] + distances(host(x, w, dy, y, relu_in, stride=stride, padding=padding), ref, den))
    return worst


def bar():
    d = float(np.load(GOLDEN)['f32_distance'])
    return max(4 * d, FLOOR)


def chain_bar():
    """tests/test_gpu_stem_chain.py: 4 x the f32 host chain's distance from the float64 chain"""
    return 4 * float(np.load(GOLDEN)['stem_chain_f32_distance'])
