"""Cases, the metric and the bar of the batch-norm tests (tests/test_batch_norm_math.py on the CPU,
tests/test_gpu_batch_norm.py on the GPU), after the scheme of tests/conv_backward_cases.py.

Shapes (M rows, C channels, ReLU) are the smallest that reach every edge of csrc/batchnorm.hip: one row (var = 0, the
max(M - 1, 1) guard of the unbiased variance, dx exactly 0 in training mode); ragged sizes; a last row chunk of one row; a row
count at which the chunk rule max(64, ceil(M / 1024)) leaves its floor; the large-separable block's own width (490 channels
in rows of 512); one channel; the channel limit; inputs far from zero (x = 100 + N(0, 1)), where an E[x^2] - E[x]^2 variance
is lost; and a constant channel (var 0 next to ordinary channels).

Metric, per tensor: max |got - ref| / max |magnitude|, the magnitude being the same formula over absolute values (for dx:
|gamma| invstd (|g| + sum|g| / M + |xhat| sum|g xhat| / M)).
Each check measures ONE step: the statistics are judged against the float64 statement of x (the variance as var + eps =
1 / invstd^2, what the op keeps); y against the float64 statement evaluated with the statistics the forward under test
returned; the backward against the float64 statement fed those statistics and the forward's own y.  (With float64's own
statistics the f32 statement's y is 1.7e-5 off on `offset`, and a recomputed ReLU mask flips signs next to zero.)
Bar: max(4 x the f32 host statement's distance from the float64 one over CASES and both modes, 3 * 2^-22).  The distance is
recorded in tests/golden/batch_norm_f32_distance.npz (`python tests/test_batch_norm_math.py --write` rewrites it)."""
import os

import numpy as np

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'batch_norm_f32_distance.npz')
FLOOR = 3 * 2.0 ** -22
EPS, MOMENTUM = 1e-5, 0.997           # the large-separable block's constants (net/resnet_v2.py)

# name: (M, C, relu)
CASES = {
    'one_row': (1, 8, False),
    'ragged': (70, 50, True),
    'chunk_tail': (129, 4, True),
    'chunk_growth': (65537, 5, False),
    'large_sep_widths': (512, 490, True),
    'one_channel': (33, 1, True),
    'widest': (3, 4096, False),
    'offset': (512, 48, True),
    'constant_channel': (64, 8, True),
}

_cache = {}


def make_case(name):
    """-> dict: x, dy [M,C], gamma, beta, moving_mean, moving_var [C], relu"""
    if name not in _cache:
        M, C, relu = CASES[name]
        rng = np.random.default_rng(sum(name.encode()) * 17 + M)
        x = rng.standard_normal((M, C)).astype(f32)
        if name == 'offset':
            x = (100 + rng.standard_normal((M, C))).astype(f32)
        if name == 'constant_channel':
            x[:, 3] = f32(0.75)
        c = dict(x=x, dy=(rng.standard_normal((M, C)) * 1e-4).astype(f32),
                 gamma=(1 + 0.1 * rng.standard_normal(C)).astype(f32), beta=(0.1 * rng.standard_normal(C)).astype(f32),
                 moving_mean=(x.mean(axis=0) + 0.1 * rng.standard_normal(C)).astype(f32),
                 moving_var=rng.uniform(0.5, 1.5, C).astype(f32))
        for a in c.values():
            a.setflags(write=False)
        c['relu'] = relu
        _cache[name] = c
    return _cache[name]


def _dist(got, ref, mag):
    err = float(np.abs(np.asarray(got, f64) - ref).max())
    d = float(np.max(mag))
    return err / d if d > 0 else (0. if err == 0 else np.inf)


def _case(name):
    """a case's name, or a dict like make_case's with tensors of any leading shape (the net's own buffers)"""
    if isinstance(name, str):
        return make_case(name)
    c = dict(name)
    C = np.shape(c['x'])[-1]
    for k in ('x', 'dy'):
        if c.get(k) is not None:
            c[k] = np.asarray(c[k]).reshape(-1, C)
    return c


def _rows(a, C):
    return None if a is None else np.asarray(a).reshape(-1, C)


def forward_distances(name, training, got):
    """got = (y, save_mean, save_invstd, moving_mean, moving_var) of a forward under test on the case -> {tensor: distance}.
    The moving statistics are judged in training mode only (None: not judged)."""
    from xdet.ops import host_batch_norm_forward
    c = _case(name)
    got = (_rows(got[0], c['x'].shape[1]),) + tuple(got[1:])
    y, mean, invstd, mm, mv = got
    x = np.asarray(c['x'], f64)
    M = x.shape[0]
    ax, ga, be = np.abs(x), np.abs(np.asarray(c['gamma'], f64)), np.abs(np.asarray(c['beta'], f64))
    out = {}
    if training:
        _, rmean, rinv, rmm, rmv = host_batch_norm_forward(c['x'], c['gamma'], c['beta'], EPS, True, MOMENTUM, c['moving_mean'],
                                                           c['moving_var'], c['relu'], f64)
        out['mean'] = _dist(mean, rmean, ax.sum(axis=0) / M)
        # var + eps as the op keeps it; its magnitude is itself (a sum of squares, plus eps)
        out['var'] = _dist(1. / np.asarray(invstd, f64) ** 2, 1. / rinv ** 2, 1. / rinv ** 2)
        if mm is not None:
            keep = 1 - MOMENTUM
            amm, amv = np.abs(np.asarray(c['moving_mean'], f64)), np.abs(np.asarray(c['moving_var'], f64))
            out['moving_mean'] = _dist(mm, rmm, amm + (amm + ax.sum(axis=0) / M) * keep)
            out['moving_var'] = _dist(mv, rmv, amv + (amv + (1. / rinv ** 2 - EPS) * (M / max(M - 1, 1))) * keep)
    else:
        out['mean'] = _dist(mean, np.asarray(c['moving_mean'], f64), np.abs(np.asarray(c['moving_mean'], f64)))
        ref = np.asarray(c['moving_var'], f64) + EPS
        out['var'] = _dist(1. / np.asarray(invstd, f64) ** 2, ref, ref)
    m64, i64 = np.asarray(mean, f64), np.asarray(invstd, f64)       # the statistics the forward under test used
    ry = ((x - m64) * i64) * np.asarray(c['gamma'], f64) + np.asarray(c['beta'], f64)
    if c['relu']:
        ry = np.maximum(ry, 0)
    out['y'] = _dist(y, ry, ((ax + np.abs(m64)) * i64) * ga + be)
    return out


def backward_distances(name, training, y, mean, invstd, got):
    """got = (dx or None, dgamma, dbeta) of a backward under test that was fed the case's x, dy, gamma and the given y (None
    without ReLU), mean and invstd -> {tensor: distance}"""
    from xdet.ops import host_batch_norm_backward
    c = _case(name)
    y, got = _rows(y, c['x'].shape[1]), (_rows(got[0], c['x'].shape[1]),) + tuple(got[1:])
    rdx, rdg, rdb = host_batch_norm_backward(c['x'], y, c['dy'], c['gamma'], mean, invstd, training, f64)
    x, g = np.asarray(c['x'], f64), np.abs(np.asarray(c['dy'], f64))
    M = x.shape[0]
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.)
    i64 = np.asarray(invstd, f64)
    axhat = np.abs((x - np.asarray(mean, f64)) * i64)
    mb, mg = g.sum(axis=0), (g * axhat).sum(axis=0)
    out = {'dgamma': _dist(got[1], rdg, mg), 'dbeta': _dist(got[2], rdb, mb)}
    if got[0] is not None:
        scale = np.abs(np.asarray(c['gamma'], f64)) * i64
        out['dx'] = _dist(got[0], rdx, scale * (g + mb / M + axhat * (mg / M)) if training else scale * g)
    return out


def statement_distances(name, training, forward=None, backward=None, dtype=f32):
    """the distances of a pair of host statements (default: xdet.ops' own, in f32) on one case: forward, then backward fed
    that forward's statistics and y -> {tensor: distance}"""
    from xdet import ops
    forward, backward = forward or ops.host_batch_norm_forward, backward or ops.host_batch_norm_backward
    c = make_case(name)
    fw = forward(c['x'], c['gamma'], c['beta'], EPS, training, MOMENTUM, c['moving_mean'], c['moving_var'], c['relu'], dtype)
    out = forward_distances(name, training, fw)
    y = fw[0] if c['relu'] else None
    out.update(backward_distances(name, training, y, fw[1], fw[2],
                                  backward(c['x'], y, c['dy'], c['gamma'], fw[1], fw[2], training, dtype)))
    return out


def f32_statement_distance():
    """the largest distance of the f32 host statements from the float64 ones, over CASES and both modes"""
    return max(max(statement_distances(name, training).values()) for name in CASES for training in (True, False))


def bar():
    d = float(np.load(GOLDEN)['f32_distance'])
    return max(4 * d, FLOOR)
