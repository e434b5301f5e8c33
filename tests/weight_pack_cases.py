"""What the pack op's tests share (tests/test_weight_pack_math.py, tests/test_gpu_weight_pack.py): the slot shapes, sources made of
distinct bit patterns, and the merges of the detector stated with the op's own words."""
import numpy as np

f32 = np.float32

# (name, outer, widths, misalign): misalign = floats by which one part's base is moved off its 16-byte boundary
CASES = [
    ('head 21|4', 7, (21, 4), 0),                       # nc | 4: neither width nor the merged row a multiple of 4
    ('rpn 44|88', 5, (44, 88), 0),                      # 2A | 4A: all multiples of 4, the 16-byte path
    ('ka 2|2', 15 * 3, (2, 2), 0),                      # the large-separable K_a at cin = 3, mid = 2
    ('outer 1', 1, (512, 512), 0),                      # a bias
    ('outer 1 odd', 1, (21, 4), 0),
    ('one part', 6, (40,), 0),
    ('four parts', 9, (8, 12, 4, 36), 0),
    ('four parts odd', 3, (5, 1, 7, 2), 0),
    ('more than one run', 33, (256, 128), 0),           # 8448 and 4224 elements: three and two runs of 4096, short last runs
    ('more than one run odd', 41, (203, 3), 0),
    ('misaligned part', 5, (44, 88), 1),                # widths allow the 16-byte path, the base does not
    ('misaligned part 3', 4, (16, 16), 3),
]


def patterns(n, seed):
    """n distinct f32 bit patterns: a seeded walk through the whole 32-bit space, so NaNs with payloads, infinities, denormals
    and both zeros come along; -0, +0, a quiet and a signalling NaN with payloads are planted at the front"""
    rng = np.random.default_rng(seed)
    start = int(rng.integers(0, 1 << 32))
    bits = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(start)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    special = np.array([0x80000000, 0x00000000, 0x7FC12345, 0xFF812345, 0x7F800000, 0x00000001], np.uint32)
    k = min(n, special.size)
    bits[:k] = special[:k]
    return bits.view(f32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def parts_of(outer, widths, seed):
    """the parts of one slot as [outer, width] arrays, cut from one run of distinct patterns (no value occurs in two parts)"""
    flat = patterns(outer * sum(widths), seed)
    offs = np.cumsum([0] + [outer * w for w in widths])
    return [flat[a:b].reshape(outer, w).copy() for a, b, w in zip(offs[:-1], offs[1:], widths)]


def large_sep_weights(cin=3, mid=2, co=5, seed=0):
    """the eight conv tensors of the large-separable block under the checkpoint's names, at small sizes"""
    rng = np.random.default_rng(seed)
    w = {}
    for br in ('Branch_0', 'Branch_1'):
        p = 'large_sep_feature/%s/' % br
        w[p + 'conv2d/kernel'] = rng.standard_normal((15, 1, cin, mid)).astype(f32)
        w[p + 'conv2d/bias'] = rng.standard_normal(mid).astype(f32)
        w[p + 'conv2d_1/kernel'] = rng.standard_normal((1, 15, mid, co)).astype(f32)
        w[p + 'conv2d_1/bias'] = rng.standard_normal(co).astype(f32)
    return w


def large_sep_slots(w, cin, mid, co):
    """merge_large_sep's three concatenations as (outer, parts) of the pack op: K_a, b_a, K_b"""
    g = lambda br, name: w['large_sep_feature/%s/%s' % (br, name)]
    return {'ka': (15 * cin, [g('Branch_0', 'conv2d/kernel'), g('Branch_1', 'conv2d/kernel')]),
            'ba': (1, [g('Branch_0', 'conv2d/bias'), g('Branch_1', 'conv2d/bias')]),
            'kb': (15, [g('Branch_0', 'conv2d_1/kernel'), g('Branch_1', 'conv2d_1/kernel')])}
