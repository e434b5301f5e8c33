"""Cases of the max-pool-backward tests (tests/test_max_pool_backward_math.py on the CPU, tests/test_gpu_max_pool_backward.py on
the GPU), after the scheme of tests/depthwise_backward_cases.py.

There is no tolerance anywhere: in float64 the statement ops.host_max_pool_backward equals torch.autograd through
F.max_pool2d on the -inf-padded input exactly, and in float32 the op equals the statement bit for bit.

Shapes (N, H, W, C) are the smallest that reach every edge of csrc/pool_backward.hip: both parities of each extent (front
padding 1 on an odd extent, 0 on an even one), maps of one and two pixels where most taps are padding, channel counts that are
no multiple of the four a thread owns (3, 5), one channel block and more (8, 64, 728 -- the entry flow's widest), more than one
workgroup of 256 (pixel, quad) pairs, and two images with the largest values planted in the rows on both sides of the image
boundary, where a window that crossed it would choose a pixel of the wrong image.

Kinds of x: 'random' ~ N(0, 1), tie-free; 'ties' integer-valued in 0..2, so every window has several maxima and the first in
row-major order must take the share; 'equal' all one value; 'positions' channel k carries, in every window, its largest value
at window position k (row-major, 0..8) wherever that position is inside the image and does not collide with a neighbouring
window's plant -- all nine positions win somewhere; 'boundary_*' as above.  dy ~ N(0, 1), no zeros."""
import numpy as np

f32, f64 = np.float32, np.float64

# the maps of the float64 test against torch.autograd (N = 2, C = 3 there)
MATH_MAPS = ((1, 1), (1, 4), (2, 2), (2, 3), (5, 5), (6, 6), (7, 4))

# name: (N, H, W, C, kind)
CASES = {
    'odd_odd': (1, 7, 5, 8, 'random'),
    'even_even': (1, 6, 8, 8, 'random'),
    'mixed': (1, 5, 6, 8, 'random'),
    'one_pixel': (1, 1, 1, 8, 'random'),
    'one_row': (1, 1, 5, 8, 'random'),
    'two_by_two': (1, 2, 2, 8, 'random'),
    'boundary_even': (2, 6, 5, 8, 'boundary_even'),
    'boundary_odd': (2, 5, 6, 8, 'boundary_odd'),
    'c3': (2, 5, 4, 3, 'random'),
    'c5': (2, 4, 5, 5, 'ties'),
    'c64': (1, 9, 10, 64, 'random'),
    'c728': (1, 5, 4, 728, 'random'),
    'ties': (2, 7, 6, 8, 'ties'),
    'all_equal': (1, 6, 5, 8, 'equal'),
    'positions_odd': (1, 9, 9, 9, 'positions'),
    'positions_even': (1, 8, 8, 9, 'positions'),
}

_cache = {}


def out_extent(n):
    """-> (outputs, padding in front) of a 3-wide window at stride 2 under TensorFlow's 'SAME' rule, written out here on its
    own: total = max((out - 1) * 2 + 3 - n, 0), the smaller half in front"""
    out = (n + 1) // 2
    total = max((out - 1) * 2 + 3 - n, 0)
    return out, total // 2


def make_x(rng, shape, kind):
    N, H, W, C = shape
    if kind == 'ties':
        return rng.integers(0, 3, shape).astype(f64)
    if kind == 'equal':
        return np.full(shape, 1.5, f64)
    x = rng.standard_normal(shape)
    if kind == 'boundary_even':      # H even: the last window of image 0 reaches one row past it, into image 1's first row
        x[0, H - 1] = 50 + rng.random((W, C))
        x[1, 0] = 100 + rng.random((W, C))
    elif kind == 'boundary_odd':     # H odd: the first window of image 1 reaches one row in front of it, into image 0's last row
        x[0, H - 1] = 100 + rng.random((W, C))
        x[1, 0] = 50 + rng.random((W, C))
    elif kind == 'positions':
        (Ho, pt), (Wo, pl) = out_extent(H), out_extent(W)
        for k in range(C):
            a, b = divmod(k % 9, 3)
            for oh in range(Ho):
                for ow in range(Wo):
                    r, c = 2 * oh - pt + a, 2 * ow - pl + b
                    if 0 <= r < H and 0 <= c < W:
                        x[:, r, c, k] = 10 + rng.random(N)
    return x


def make_case(name):
    """-> dict: x [N,H,W,C], dy [N,Ho,Wo,C], float32, read-only"""
    if name not in _cache:
        N, H, W, C, kind = CASES[name]
        rng = np.random.default_rng(sum(name.encode()) * 23 + N * H * W * C)
        x = make_x(rng, (N, H, W, C), kind).astype(f32)
        dy = rng.standard_normal((N, out_extent(H)[0], out_extent(W)[0], C)).astype(f32)
        dy[dy == 0] = 1
        x.setflags(write=False)
        dy.setflags(write=False)
        _cache[name] = dict(x=x, dy=dy)
    return _cache[name]


def torch_max_pool_backward(x, dy):
    """d (max_pooling2d(3, 2, 'same')(x) * dy).sum() / dx by torch.autograd in the dtype of x: F.max_pool2d without padding of
    its own on the input padded with -inf by the 'SAME' rule"""
    import torch
    import torch.nn.functional as F
    x, dy = np.asarray(x), np.asarray(dy)
    N, H, W, C = x.shape
    (Ho, pt), (Wo, pl) = out_extent(H), out_extent(W)
    xp = np.full((N, C, 2 * Ho + 1, 2 * Wo + 1), -np.inf, x.dtype)
    xp[:, :, pt:pt + H, pl:pl + W] = np.transpose(x, (0, 3, 1, 2))
    t = torch.tensor(xp, requires_grad=True)
    y = F.max_pool2d(t, 3, 2)
    assert tuple(y.shape) == (N, C, Ho, Wo)
    (y * torch.tensor(np.transpose(dy, (0, 3, 1, 2)).astype(x.dtype))).sum().backward()
    return np.ascontiguousarray(np.transpose(t.grad.numpy()[:, :, pt:pt + H, pl:pl + W], (0, 2, 3, 1)))
