"""Cases, the metric and the bar of the dense-layer backward tests (tests/test_dense_backward_math.py on the CPU,
tests/test_gpu_dense_backward.py on the GPU).

Shapes (M, K, J) are the smallest that reach every edge of csrc/dense_backward.hip: one row; ragged in all three dimensions
with J below one MFMA K step; the head's real K one row over a tile; the head's true widths at a small M; and for K = J = 16
(one tile, so dW's row ranges are 128 rows, include/xdet.h) an M that leaves a single row in the last range and one that
ends on a range boundary.

Metric, per output tensor: max |got - ref| / max (|A| . |B|), the largest entry of the product of the operands' magnitudes
(for db: the largest column sum of |g|).  It stays meaningful for tiny gradients and for sums that cancel.
Bar: max(4 x the f32 statement's distance from the float64 one over CASES, 3 * 2^-22).  The 4 is the margin the loss and
spectral tests give the GPU; the floor is what the split representation can lose: each operand is kept to 2^-22 relative
and the lo * lo term is dropped.  The f32 statement's distance is recorded in tests/golden/dense_backward_f32_distance.npz
(`python tests/test_dense_backward_math.py --write` rewrites it)."""
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dense_backward_f32_distance.npz')
FLOOR = 3 * 2.0 ** -22

# name: (M, K, J, ReLU)
CASES = {
    'one_row': (1, 16, 16, False),
    'ragged': (70, 50, 25, True),
    'ragged_linear': (70, 50, 25, False),
    'real_k_row_over_tile': (257, 490, 96, True),
    'cls_loc_widths': (130, 2048, 25, False),
    'subnet_fc_widths': (130, 490, 2048, True),
    'last_range_single_row': (129, 16, 16, True),
    'range_boundary': (256, 16, 16, True),
}

_cache = {}


def make_case(name):
    """-> x [M,K], w [K,J], dy [M,J] (gradient-sized: about 1e-4), y [M,J] = relu(x w + b) with its exact zeros, or None"""
    if name not in _cache:
        M, K, J, relu = CASES[name]
        rng = np.random.default_rng(sum(name.encode()) * 13 + M)
        x = rng.standard_normal((M, K)).astype(f32)
        w = (rng.standard_normal((K, J)) / np.sqrt(K)).astype(f32)
        dy = (rng.standard_normal((M, J)) * 1e-4).astype(f32)
        y = np.maximum(x @ w + rng.standard_normal(J).astype(f32), f32(0)).astype(f32) if relu else None
        assert y is None or ((y == 0).any() and (y > 0).any())
        for a in (x, w, dy, y):
            if a is not None:
                a.setflags(write=False)
        _cache[name] = (x, w, dy, y)
    return _cache[name]


def reference64(x, w, dy, y):
    """the float64 statement and the three denominators of the metric"""
    from xdet.ops import host_dense_backward
    dx, dw, db = host_dense_backward(x, w, dy, y, dtype=np.float64)
    g = np.abs(np.asarray(dy, np.float64))
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.)
    ax, aw = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64))
    den = (float((g @ aw.T).max()), float((ax.T @ g).max()), float(g.sum(0).max()))
    return (dx, dw, db), den


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
    """the largest distance of host_dense_backward in f32 from the float64 statement, over CASES"""
    from xdet.ops import host_dense_backward
    worst = 0.
    for name in CASES:
        ref, den = case_reference(name)
        worst = max([worst] + distances(host_dense_backward(*make_case(name)), ref, den))
    return worst


def bar():
    d = float(np.load(GOLDEN)['f32_distance'])
    return max(4 * d, FLOOR)
